"""Plain references of the inference post-process - kodhip_nms_ex's options (best-class candidates, class filter after the
argmax, class-agnostic suppression, max_det, boxes back into the source image) - and the constructed inputs that
tests/test_predict_reference.py (CPU) and tests/test_hip_predict.py (GPU) run.

Nothing here touches the HIP library.  Written from the definitions (YOLOv5 general.py non_max_suppression with
multi_label=False / classes / agnostic / max_det, and scale_boxes + clip_boxes with one gain per axis), not from the kernels:

* `best_class_det`   the detections with every class column but the row's best one zeroed: best = the largest
                     fp32(cls_c * obj), the LOWEST class index among equal maxima (start at class 0, replace only on `>`); a
                     row whose best class is not in `classes` loses that column too (the filter comes after the argmax).
                     A zeroed column never passes `cls * obj > conf` (conf >= 0), so the multi-label reference on this
                     array is the best-class NMS: at most one candidate per row, listed in row order, same keys.
* `nms_ex_ref`       `val_reference.nms_ref` on it (fp32, every operation rounded on its own, score descending then candidate
                     index ascending), then `unletterbox_ref` on the kept rows.
* `unletterbox_ref`  x' = min(max(fp32(fp32(x - left) * scale_x), 0), width), y' alike with top, scale_y, height.

Every case builder returns its inputs together with facts computed from the references alone; the CPU test asserts them,
which keeps a GPU test from passing on an input that no longer reaches what it was built for.
"""
from __future__ import annotations

import numpy as np

import val_reference as V

_f32 = V._f32


def best_class_det(det, classes=None):
    """[B, rows, 5+nc] fp32 -> a copy with all class columns zeroed except each row's best class (and that one too when
    `classes` does not list it)."""
    det = _f32(det)
    nc = det.shape[2] - 5
    score = det[..., 5:] * det[..., 4:5]                       # fp32 product, rounded once
    best, arg = score[..., 0].copy(), np.zeros(det.shape[:2], np.int64)
    for c in range(1, nc):
        m = score[..., c] > best
        best[m], arg[m] = score[..., c][m], c
    on = np.arange(nc)[None, None, :] == arg[..., None]
    if classes is not None:
        on &= np.isin(arg, np.asarray(list(classes)))[..., None]
    out = det.copy()
    out[..., 5:] = np.where(on, det[..., 5:], np.float32(0))
    return out


def unletterbox_ref(rows, lb):
    """rows [n, 6] fp32, lb = (left, top, scale_x, scale_y, width, height) -> rows with the box in source-image pixels"""
    out = _f32(rows).copy().reshape(-1, 6)
    left, top, sx, sy, w, h = (np.float32(v) for v in _f32(lb))
    zero = np.float32(0)
    for k, (o, s, hi) in enumerate(((left, sx, w), (top, sy, h), (left, sx, w), (top, sy, h))):
        out[:, k] = np.minimum(np.maximum((out[:, k] - o) * s, zero), hi)
    return out


def nms_ex_ref(det, conf, thr, max_det=300, max_nms=30000, max_wh=4096, best_class=False, classes=None, letterbox=None,
               key_cap=None, info=None):
    """-> list of [n <= max_det, 6] fp32 rows.  best_class False: val_reference.nms_ref with the class filter on the
    candidates.  letterbox [B, 6]: the kept rows mapped back.  Class-agnostic suppression is max_wh = 0."""
    assert conf >= 0
    if best_class:
        rows = V.nms_ref(best_class_det(det, classes), conf, thr, max_det, max_nms, max_wh, key_cap=key_cap, info=info)
    else:
        rows = V.nms_ref(det, conf, thr, max_det, max_nms, max_wh, key_cap=key_cap, classes=classes, info=info)
    if letterbox is not None:
        rows = [unletterbox_ref(r, lb) for r, lb in zip(rows, _f32(letterbox).reshape(-1, 6))]
    return rows


def keys_ex_ref(det, conf, best_class=False, classes=None):
    """per image (keys in candidate order, sorted keys) - val_reference.nms_keys_ref under the options"""
    if best_class:
        return V.nms_keys_ref(best_class_det(det, classes), conf)
    return V.nms_keys_ref(det, conf, classes)


def cap_for(n):
    cap = 64
    while cap < n:
        cap <<= 1
    return cap


# ------------------------------------------------------------------------------------------------------------ cases
def _scene(rng, B, rows, nc, obj_lo=0.1, canvas=600.0):
    """random boxes on a canvas, continuous obj and class probabilities (tie-free with overwhelming probability)"""
    det = np.zeros((B, rows, 5 + nc), np.float32)
    c = rng.uniform(60, canvas, (B, rows, 2)); wh = rng.uniform(15, 110, (B, rows, 2))
    det[..., 0:2], det[..., 2:4] = c - wh / 2, c + wh / 2
    det[..., 4] = rng.uniform(obj_lo, 1.0, (B, rows))
    det[..., 5:] = rng.uniform(0.0, 1.0, (B, rows, nc))
    return det


def _tie_free(det, conf):
    return all(len(np.unique(k >> np.uint64(32))) == len(k) for k, _ in V.nms_keys_ref(det, conf))


def random_case(nc, seed=None):
    """[2, 1300, 5+nc] (two iterations of the 1024-row compaction), conf 0.25, thr 0.45 -> (det, conf, thr, facts)"""
    rng = np.random.default_rng(100 + nc if seed is None else seed)
    det = _scene(rng, 2, 1300, nc)
    conf, thr = 0.25, 0.45
    multi, best = keys_ex_ref(det, conf), keys_ex_ref(det, conf, True)
    score = det[..., 5:] * det[..., 4:5]
    facts = dict(multi=[len(k) for k, _ in multi], best=[len(k) for k, _ in best], tie_free=_tie_free(best_class_det(det), conf),
                 rows_with_two_over_conf=int((((score > np.float32(conf)) & (det[..., 4:5] > np.float32(conf))).sum(-1) >= 2).sum()),
                 best_beyond_1024=[int(((k & np.uint64(0xFFFFFFFF)) // np.uint64(nc) >= 1024).sum()) for k, _ in best])
    return det, conf, thr, facts


def hand_cases():
    """name -> (det [1, rows, 5+3], conf, thr, classes, facts)"""
    out = {}
    A, Bx, Cx = [0, 0, 10, 10], [50, 50, 60, 60], [100, 0, 110, 10]
    # a row with two classes over conf: multi-label lists both, best-class the larger one
    d = V._det_from([A, Bx], [1.0, 1.0], [[0.5, 0.1, 0.75], [0.1, 0.5, 0.1]])[None]
    out["two_over_conf"] = (d, 0.25, 0.45, None, dict(multi=3, best=2, best_classes=[2, 1]))
    # the two best products are equal (0.5 * 0.75 on classes 1 and 2; 0.5 * 0.5 on class 0): the lower index wins
    d = V._det_from([A, Bx], [0.5, 0.5], [[0.5, 0.75, 0.75], [0.75, 0.5, 0.75]])[None]
    out["equal_products"] = (d, 0.2, 0.45, None, dict(multi=6, best=2, best_classes=[1, 0]))
    # row 0: best class 0 unlisted, class 1 listed and over conf -> gone; row 1: best class 1 listed; row 2: best class 2 unlisted
    d = V._det_from([A, Bx, Cx], [1.0, 1.0, 1.0], [[0.875, 0.625, 0.1], [0.1, 0.5, 0.3], [0.1, 0.1, 0.9]])[None]
    out["best_unlisted"] = (d, 0.25, 0.45, [1], dict(multi=2, best=1, best_classes=[1]))
    for d, _, _, _, f in out.values():
        top2 = np.sort(d[0, :, 5:] * d[0, :, 4:5], -1)[:, -2:]
        f["rows_with_equal_best_products"] = int((top2[:, 0] == top2[:, 1]).sum())
    return out


BIG_ROWS, BIG_NC, BIG_KEY_CAP = 5000, 80, 8192


def big_case(seed=31):
    """[1, 5000, 5+80], conf 0.05: more than 4096 best-class candidates in a key_cap = 8192 workspace - two sort chunks and
    a merge pass - where the multi-label form needs 2^19 keys (64 x as many).  -> (det, conf, thr, facts)"""
    rng = np.random.default_rng(seed)
    det = _scene(rng, 1, BIG_ROWS, BIG_NC, obj_lo=0.02)
    conf, thr = 0.05, 0.45
    info = []
    res = nms_ex_ref(det, conf, thr, best_class=True, key_cap=BIG_KEY_CAP, info=info)
    facts = dict(best=[len(k) for k, _ in keys_ex_ref(det, conf, True)], multi_key_cap=cap_for(BIG_ROWS * BIG_NC),
                 survivors=[len(r) for r in res], last_rank=[i["last_rank"] for i in info])
    return det, conf, thr, facts


COUNTS_KEY_CAP = 2048
COUNTS = (0, 1, 64, 65, COUNTS_KEY_CAP)


def counts_case(seed=37):
    """[5, 2048, 5+4], conf 0.1, key_cap 2048: image b has exactly COUNTS[b] best-class candidates on scattered rows, the
    last one a candidate on EVERY row (count = rows = key_cap).  Rows that are off have obj = 0."""
    rng = np.random.default_rng(seed)
    B, rows, nc = len(COUNTS), COUNTS_KEY_CAP, 4
    det = _scene(rng, B, rows, nc, canvas=2000.0)
    det[..., 4] = 0
    for b, n in enumerate(COUNTS):
        on = rng.permutation(rows)[:n]
        det[b, on, 4] = rng.uniform(0.6, 1.0, n)
        det[b, on, 5 + rng.integers(0, nc, n)] = rng.uniform(0.5, 1.0, n)      # one class surely over conf
    conf, thr = 0.1, 0.45
    facts = dict(best=[len(k) for k, _ in keys_ex_ref(det, conf, True)], multi=[len(k) for k, _ in keys_ex_ref(det, conf)])
    return det, conf, thr, facts


def agnostic_case():
    """two overlapping boxes (IoU 81 / 119) of classes 0 and 2: the class offset keeps both, max_wh = 0 the higher-scored one"""
    det = V._det_from([[0, 0, 10, 10], [1, 1, 11, 11], [200, 200, 220, 220]], [1.0, 1.0, 1.0],
                      [[0.5, 0.1, 0.1], [0.1, 0.1, 0.75], [0.1, 0.625, 0.1]])[None]
    off, agn = nms_ex_ref(det, 0.25, 0.45, best_class=True)[0], nms_ex_ref(det, 0.25, 0.45, max_wh=0, best_class=True)[0]
    facts = dict(with_offset=len(off), agnostic=len(agn), agnostic_scores=agn[:, 4].tolist(), agnostic_classes=agn[:, 5].tolist())
    return det, 0.25, 0.45, facts


MAX_DETS = (1, 5, 300)


def max_det_case():
    """[1, 320, 5+2]: 320 disjoint boxes, descending scores on alternating classes - more survivors than any cap"""
    n = 320
    sc = 0.99 - 0.002 * np.arange(n)
    det = V._one_hot_det(V._grid_boxes(n), sc, list(np.arange(n) % 2), 2)
    facts = dict(uncapped=len(nms_ex_ref(det, 0.25, 0.45, max_det=300, best_class=True)[0]),
                 candidates=len(keys_ex_ref(det, 0.25, True)[0][0]))
    return det, 0.25, 0.45, facts


def letterbox_case():
    """[3, 6, 5+2], three different transforms in one batch (upscaled + padded left / top, downscaled + padded, a narrow
    strip); in every image rows 0 .. 3 cross the left, top, right and bottom border of the content, row 4 lies inside and
    row 5 lies wholly in the padding (clipping makes it degenerate; it stays).  -> (det, conf, thr, letterbox, facts)"""
    lbs = _f32([[80.0, 0.0, 375 / 480.0, 500 / 640.0, 375.0, 500.0],                 # 500 x 375 (h x w) source as 640 x 480, left pad 80
                [0.0, 140.0, 1333 / 640.0, 750 / 360.0, 1333.0, 750.0],              # 750 x 1333 source as 360 x 640, top pad 140
                [14.0, 0.0, 17 / 35.0, 31 / 64.0, 17.0, 31.0]])                      # 31 x 17 source as 64 x 35 in a 64 px frame
    dets = []
    for left, top, sx, sy, w, h in lbs.astype(np.float64):
        cw, ch = w / sx, h / sy                                    # content size in the letterboxed frame
        x0, y0, x1, y1 = left, top, left + cw, top + ch
        boxes = [[x0 - 0.3 * cw, y0 + 0.2 * ch, x0 + 0.2 * cw, y0 + 0.4 * ch],      # left
                 [x0 + 0.3 * cw, y0 - 0.3 * ch, x0 + 0.5 * cw, y0 + 0.15 * ch],     # top
                 [x0 + 0.7 * cw, y0 + 0.5 * ch, x1 + 0.2 * cw, y0 + 0.7 * ch],      # right
                 [x0 + 0.1 * cw, y0 + 0.8 * ch, x0 + 0.25 * cw, y1 + 0.3 * ch],     # bottom
                 [x0 + 0.52 * cw, y0 + 0.2 * ch, x0 + 0.68 * cw, y0 + 0.45 * ch],   # inside
                 [x1 + 0.5 * cw + 5, y1 + 0.5 * ch + 5, x1 + 0.6 * cw + 9, y1 + 0.6 * ch + 9]]      # in the padding
        sc = [0.9, 0.85, 0.8, 0.75, 0.7, 0.65]
        dets.append(V._one_hot_det(boxes, sc, [0, 1, 0, 1, 0, 1], 2)[0])
    det = np.stack(dets)
    conf, thr = 0.25, 0.45
    plain = nms_ex_ref(det, conf, thr, best_class=True)
    far = lbs.copy(); far[:, 4:] = 1e9                              # the same transform without the upper clip
    mapped, unclipped_hi = nms_ex_ref(det, conf, thr, best_class=True, letterbox=lbs), nms_ex_ref(det, conf, thr, best_class=True, letterbox=far)
    clipped = []
    for p, m, u, lb in zip(plain, mapped, unclipped_hi, lbs):
        lo = (p[:, :4] - lb[[0, 1, 0, 1]]) < 0                      # the lower clip acted
        hi = u[:, :4] != m[:, :4]                                   # the upper clip acted
        clipped.append(dict(left=bool(lo[0, 0]), top=bool(lo[1, 1]), right=bool(hi[2, 2]), bottom=bool(hi[3, 3]),
                            inside_untouched=not (lo[4].any() or hi[4].any()),
                            degenerate=bool(m[5, 0] == m[5, 2] and m[5, 1] == m[5, 3])))
    facts = dict(rows=[len(p) for p in plain], clipped=clipped, transforms_differ=len({tuple(lb) for lb in lbs.tolist()}) == len(lbs))
    return det, conf, thr, lbs, facts


def identity_letterbox(B, extent=1e6):
    """left = top = 0, scale 1, an image larger than every coordinate: (x - 0) * 1 is x, and no clip acts on 0 <= x <= extent"""
    return np.tile(_f32([0, 0, 1, 1, extent, extent]), (B, 1))
