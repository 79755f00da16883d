"""Plain fp64 reference of the device validation metrics (csrc/val_metrics.hip, DeviceDetectionMetrics) and the inputs that
tests/test_val_metrics_reference.py (CPU) and tests/test_hip_val_metrics.py (GPU) run.  Nothing here touches the HIP library.

MATCHER, two forms of YOLOv5's val.py `process_batch` made deterministic.  A pair (detection, ground truth) is a candidate
when the classes are equal and in [0, nc), and IoU = inter / (area_d + area_g - inter) (fp64, width / height of the
intersection clamped at 0, no +1, no epsilon) has a union that is neither zero nor NaN and is itself not NaN.
* `match_closed` (what the kernel does): detection d picks its candidate of largest IoU (equal IoUs -> the lower ground-truth
  index); with run_d the largest IoU among LOWER-index detections that picked the same ground truth (-1 if none), d is
  correct at threshold t iff run_d < t <= IoU_d.  -> one bitmask per detection.
* `match_literal`: the per-threshold procedure - the candidates with IoU >= t sorted by IoU descending, the first pair per
  detection kept (the list is then in detection order), then the first pair per ground truth.
They agree whenever IoUs do not tie (asserted on random scenes by the CPU test); with ties the closed form IS the definition.
Every detection whose class is in [0, nc) yields one record (score fp32, class, mask), in image order then detection order.

CURVES: utils/metrics.py `ap_per_class` with `np.interp` itself, records ordered by (class ascending, score descending, arrival
ascending); a class without ground truth or without records gets zero rows.  The tail (F1, smoothing, argmax, means) is
`summarize` of the package: shared code, so the device path is compared on p / r / ap and must then report the same index.

Exactness of the matcher comparison: coordinates of every GPU case are multiples of 1/4 below 2048 (areas, intersections and
unions exact in fp64, the IoU one correctly rounded division on either side) - masks, order and nt are compared for equality.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from confusion_reference import det_class, snap
from val_reference import _f32, _grid_boxes, random_scene

PX = np.linspace(0, 1, 1000)
X101 = np.linspace(0, 1, 101)
IOUS10 = np.linspace(0.5, 0.95, 10)
IOUS16 = np.linspace(0.2, 0.95, 16)
IOUS1 = np.array([0.5])


# ---- matcher -------------------------------------------------------------------------------------------------------------

def pair_iou(d, g):
    """fp64 IoU of two xyxy boxes, or None when the pair is no candidate (zero / NaN union, NaN IoU)"""
    x1, y1, x2, y2 = (np.float64(v) for v in d)
    gx1, gy1, gx2, gy2 = (np.float64(v) for v in g)
    w = min(x2, gx2) - max(x1, gx1)
    h = min(y2, gy2) - max(y1, gy1)
    w = w if w > 0 else np.float64(0)
    h = h if h > 0 else np.float64(0)
    inter = w * h
    uni = (x2 - x1) * (y2 - y1) + (gx2 - gx1) * (gy2 - gy1) - inter
    if uni == 0 or np.isnan(uni):
        return None
    iou = inter / uni
    return None if np.isnan(iou) else iou


def _image(d_img, g_box, g_lab, nc):
    d_img = _f32(d_img).reshape(-1, 6)
    g_box = np.asarray(g_box, dtype=np.float64).reshape(-1, 4)
    g_lab = np.asarray(g_lab, dtype=np.int64).reshape(-1)
    cls = []
    for row in d_img:
        c = det_class(row[5])
        cls.append(c if c is not None and 0 <= c < nc and row[5] > -1 else -1)
    cand = {}                                              # (d, g) -> IoU
    for d, c in enumerate(cls):
        if c < 0:
            continue
        for g in range(len(g_lab)):
            if int(g_lab[g]) != c:
                continue
            v = pair_iou(d_img[d, :4], g_box[g])
            if v is not None:
                cand[(d, g)] = v
    return d_img, g_lab, cls, cand


def match_closed(d_img, g_box, g_lab, nc, thrs, events=None):
    """-> (classes per detection (-1: takes no part), masks per detection)"""
    d_img, g_lab, cls, cand = _image(d_img, g_box, g_lab, nc)
    ev = events if events is not None else {}
    pick, iou = {}, {}
    for d in range(len(cls)):
        for g in range(len(g_lab)):
            v = cand.get((d, g))
            if v is None:
                continue
            if d in pick and v == iou[d] and v >= min(thrs):          # (ties below every threshold decide nothing)
                ev["tie_gt"] = ev.get("tie_gt", 0) + 1
            if d not in pick or v > iou[d]:
                pick[d], iou[d] = g, v
    run_of = {}
    masks = [0] * len(cls)
    for d in range(len(cls)):
        if d not in pick:
            continue
        run = run_of.get(pick[d], np.float64(-1))
        for t, thr in enumerate(thrs):
            if run < thr <= iou[d]:
                masks[d] |= 1 << t
            ev["exact_thr"] = ev.get("exact_thr", 0) + int(iou[d] == thr)
        low = [t for t in range(len(thrs)) if not masks[d] >> t & 1 and any(masks[d] >> u & 1 for u in range(t + 1, len(thrs)))]
        ev["holes"] = ev.get("holes", 0) + int(bool(low))
        ev["lost"] = ev.get("lost", 0) + int(run >= iou[d])
        if pick[d] in run_of and iou[d] == run and run >= min(thrs):
            ev["tie_det"] = ev.get("tie_det", 0) + 1
        run_of[pick[d]] = max(run, iou[d])
    return cls, masks


def match_literal(d_img, g_box, g_lab, nc, thrs):
    """the per-threshold procedure of process_batch -> (classes, masks)"""
    d_img, g_lab, cls, cand = _image(d_img, g_box, g_lab, nc)
    masks = [0] * len(cls)
    for t, thr in enumerate(thrs):
        pairs = [(d, g, v) for (d, g), v in cand.items() if v >= thr]
        pairs.sort(key=lambda x: (-x[2], x[1], x[0]))                       # by IoU, descending
        first, seen = [], set()
        for d, g, v in pairs:                                               # the first pair of every detection ...
            if d not in seen:
                seen.add(d); first.append((d, g, v))
        first.sort(key=lambda x: x[0])                                      # ... which leaves the list in detection order
        seen = set()
        for d, g, v in first:                                               # the first pair of every ground truth
            if g not in seen:
                seen.add(g); masks[d] |= 1 << t
    return cls, masks


def process(dets, gts, nc, thrs, matcher=match_closed, events=None):
    """per-image lists -> (scores fp32 [n], classes i64 [n], masks i64 [n], nt i64 [nc]): the record store after one batch"""
    scores, classes, masks = [], [], []
    nt = np.zeros(nc, np.int64)
    for d_img, (g_box, g_lab) in zip(dets, gts):
        d_img = _f32(d_img).reshape(-1, 6)
        kw = {"events": events} if matcher is match_closed else {}
        cls, m = matcher(d_img, g_box, g_lab, nc, thrs, **kw)
        for d, c in enumerate(cls):
            if c >= 0:
                scores.append(d_img[d, 4]); classes.append(c); masks.append(m[d])
        for l in np.asarray(g_lab, dtype=np.int64).reshape(-1):
            if 0 <= l < nc:
                nt[l] += 1
    return np.asarray(scores, np.float32), np.asarray(classes, np.int64), np.asarray(masks, np.int64), nt


# ---- curves --------------------------------------------------------------------------------------------------------------

def curves_ref(scores, classes, masks, nt, nc, T, px=PX, xr=X101):
    """-> dict p [nc, len(px)], r, ap [nc, T], nt, n_p"""
    scores = np.asarray(scores, np.float32)
    classes, masks, nt = np.asarray(classes, np.int64), np.asarray(masks, np.int64), np.asarray(nt, np.int64)
    n = len(scores)
    order = np.lexsort((np.arange(n), -scores.astype(np.float64), classes))
    p, r, ap = np.zeros((nc, len(px))), np.zeros((nc, len(px))), np.zeros((nc, T))
    n_p = np.zeros(nc, np.int64)
    for c in range(nc):
        sel = order[classes[order] == c]
        n_p[c] = len(sel)
        n_l = int(nt[c])
        if len(sel) == 0 or n_l == 0:
            continue
        conf = scores[sel].astype(np.float64)
        tp = ((masks[sel][:, None] >> np.arange(T)[None, :]) & 1).astype(bool)
        tpc = tp.cumsum(0)
        fpc = (1 - tp).cumsum(0)
        recall = tpc / (n_l + 1e-16)
        precision = tpc / (tpc + fpc)
        r[c] = np.interp(-px, -conf, recall[:, 0], left=0)
        p[c] = np.interp(-px, -conf, precision[:, 0], left=1)
        for j in range(T):
            mrec = np.concatenate(([0.0], recall[:, j], [1.0]))
            mpre = np.concatenate(([1.0], precision[:, j], [0.0]))
            mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
            q = np.interp(xr, mrec, mpre)
            ap[c, j] = ((q[:-1] + q[1:]) / 2 * (xr[1:] - xr[:-1])).sum()
    return {"p": p, "r": r, "ap": ap, "nt": nt, "n_p": n_p}


# ---- matcher cases -------------------------------------------------------------------------------------------------------

class MatchCase(NamedTuple):
    nc: int
    thrs: np.ndarray
    dets: list                 # per image [n, 6] fp32
    gts: list                  # per image ([m, 4] fp64, [m] int64)


def _one(nc, thrs, det_rows, gt_boxes, gt_labels):
    return MatchCase(nc, thrs, [_f32(det_rows).reshape(-1, 6)],
                     [(np.asarray(gt_boxes, dtype=np.float64).reshape(-1, 4), np.asarray(gt_labels, dtype=np.int64))])


FULL = (1 << 10) - 1
# name -> (case, expected masks of the records, expected nt) - one image each, thresholds 0.5 : 0.05 : 0.95, worked by hand
# below; the CPU test holds both matchers (and the GPU test the kernel) to them


def hand_cases():
    out = {}
    # A: one class, two ground truths.  d0 sits on G0 exactly (IoU 1: correct at all ten thresholds); d1 overlaps nothing: its
    # candidates have IoU 0, it picks G0 (lower index) and is correct nowhere; d2 covers 7.75 / 10 of G1's height: IoU 0.775,
    # correct at 0.5 .. 0.75 = bits 0 - 5.
    out["A_tp_fp_tp"] = (_one(1, IOUS10, [[0, 0, 10, 10, 0.9, 0], [50, 50, 60, 60, 0.8, 0], [20, 0, 30, 7.75, 0.7, 0]],
                              [[0, 0, 10, 10], [20, 0, 30, 10]], [0, 0]), [FULL, 0, 0b111111], [2])
    # B: d0 has IoU 0.625 with G0 (bits 0 - 2: 0.5, 0.55, 0.6), d1 has IoU 0.875 and picks G0 too.  d0 has the lower index, so
    # it keeps the thresholds it reaches; d1 is correct where 0.625 < t <= 0.875: 0.65 .. 0.85 = bits 3 - 7 - a hole at the
    # bottom, although d1's IoU is the larger one.
    out["B_hole_at_the_bottom"] = (_one(1, IOUS10, [[0, 0, 10, 6.25, 0.9, 0], [0, 0, 10, 8.75, 0.8, 0]], [[0, 0, 10, 10]], [0]),
                                   [0b111, 0b11111000], [1])
    # C: [0, 0, 2, 2] against [0, 0, 2, 1] is IoU 0.5 exactly: correct at 0.5 (t <= IoU), bit 0 only
    out["C_exactly_on_a_threshold"] = (_one(1, IOUS10, [[0, 0, 2, 1, 0.9, 0]], [[0, 0, 2, 2]], [0]), [1], [1])
    # D: duplicate ground truths and duplicate detections.  Both detections have IoU 1 with G0 and G1: both pick G0 (tie ->
    # lower ground-truth index); d0 takes every threshold, d1 (run = 1 = its IoU) none.  G1 stays unmatched.
    out["D_duplicates"] = (_one(1, IOUS10, [[0, 0, 8, 8, 0.9, 0], [0, 0, 8, 8, 0.9, 0]], [[0, 0, 8, 8], [0, 0, 8, 8]], [0, 0]),
                           [FULL, 0], [2])
    # E: classes outside [0, nc): detection class 3 (= nc) and -1 give no record, label 7 is not counted and never matched;
    # the class-1 detection on the label-7 box finds no candidate (mask 0), the class-2 pair matches
    out["E_class_outside"] = (_one(3, IOUS10, [[0, 0, 10, 10, 0.9, 3], [0, 0, 10, 10, 0.8, 1], [30, 30, 40, 40, 0.7, 2],
                                               [30, 30, 40, 40, 0.6, -1]],
                                   [[0, 0, 10, 10], [30, 30, 40, 40]], [7, 2]), [0, FULL], [0, 0, 1])
    # F: a loser is not offered its second best.  d0 and d1 both pick G0 (IoU 1 and 0.9); d1 overlaps G1 with IoU 2 / 3 but never
    # asks for it: mask 0, and G1 stays unmatched
    out["F_loser_not_rematched"] = (_one(1, IOUS10, [[0, 0, 10, 10, 0.9, 0], [0, 1, 10, 10, 0.8, 0]],
                                         [[0, 0, 10, 10], [0, 4, 10, 10]], [0, 0]), [FULL, 0], [2])
    return out


def shape_cases():
    """name -> MatchCase for the GPU test's shapes (all on the 1/4 lattice)"""
    out = {}
    g3 = _grid_boxes(3).astype(np.float64)
    out["no_detections"] = _one(2, IOUS10, [], g3, [0, 1, 0])
    out["no_ground_truth"] = _one(2, IOUS10, [[0, 0, 10, 10, 0.9, 0], [20, 20, 40, 40, 0.8, 1]], [], [])
    out["both_empty"] = _one(2, IOUS10, [], [], [])
    # 300 detections against 3 ground truths: more detections than threads.  Detection i sits on ground truth i % 3 with k quarter
    # pixels cut off its height (IoU 1 - k / 40); over q = i // 3 the cut shrinks by one every third detection, with a deeper
    # cut in between: the running maximum of a ground truth climbs through the thresholds (holes) and two in three lose
    rows = []
    for i in range(300):
        q = i // 3
        b = g3[i % 3].copy()
        b[3] -= 0.25 * (max(0, 15 - q // 3) + (2 if q % 3 == 1 else 0))
        rows.append([*b, 0.99 - 0.003 * i, i % 3 % 2])
    out["det300_gt3"] = _one(2, IOUS10, rows, g3, [0, 1, 0])
    # 5 detections against 300 ground truths (beyond the block's threads and map_match's 256): exact fits on 0, 255, 256, 299
    g300 = _grid_boxes(300).astype(np.float64)
    lab = (np.arange(300) % 3).astype(np.int64)
    rows = [[*g300[k], 0.9 - 0.1 * i, lab[k]] for i, k in enumerate((0, 255, 256, 299))] + [[*g300[299], 0.4, lab[299]]]
    out["det5_gt300"] = _one(3, IOUS10, rows, g300, lab)
    return out


def random_batch(nc, seed, n_img=16, thrs=IOUS10, step=0.25, size=320):
    dets, gts = snap(*random_scene(np.random.default_rng(seed), nc, n_img, size=size), step=step)
    return MatchCase(nc, thrs, dets, gts)


def continuous_batch(nc, seed, n_img):
    """random_scene as it comes (continuous coordinates: IoUs do not tie)"""
    dets, gts = random_scene(np.random.default_rng(seed), nc, n_img)
    return MatchCase(nc, IOUS10, dets, [(np.asarray(g, np.float64), np.asarray(l, np.int64)) for g, l in gts])


def pack(case: MatchCase, max_det=None):
    """-> (det [B, max_det, 6] fp32, ndet [B] i32, gt [n, 4] f64, labels [n] i64, start [B+1] i32)"""
    from confusion_reference import pack as _pack
    return _pack(case.dets, case.gts, max_det)


# ---- curve cases ---------------------------------------------------------------------------------------------------------

class CurveCase(NamedTuple):
    nc: int
    T: int
    feeds: list                # [(scores fp32, classes, masks, nt [nc])]: one add_records call each

    def merged(self):
        s = np.concatenate([f[0] for f in self.feeds]).astype(np.float32)
        c = np.concatenate([f[1] for f in self.feeds]).astype(np.int64)
        m = np.concatenate([f[2] for f in self.feeds]).astype(np.int64)
        return s, c, m, sum(np.asarray(f[3], np.int64) for f in self.feeds)


def _feed(scores, classes, masks, nt):
    return (np.asarray(scores, np.float32), np.asarray(classes, np.int64), np.asarray(masks, np.int64), np.asarray(nt, np.int64))


def _random_feed(rng, n, class_ids, nc, T, quantum=None, p_tp=0.5):
    scores = rng.uniform(0.001, 1.0, n).astype(np.float32)
    if quantum:
        scores = (np.ceil(scores / np.float32(quantum)) * np.float32(quantum)).astype(np.float32)
    classes = rng.choice(np.asarray(class_ids), n)
    # like a real matcher: correct at the low thresholds up to a random one, sometimes with a hole at the bottom
    hi = np.where(rng.random(n) < p_tp, rng.integers(1, T + 1, n), 0)
    lo = np.where(rng.random(n) < 0.1, rng.integers(0, T, n), 0)
    masks = np.array([sum(1 << t for t in range(l, h)) for l, h in zip(lo, hi)], np.int64)
    nt = np.zeros(nc, np.int64)
    for c in class_ids:
        nt[c] = int((classes == c).sum()) + int(rng.integers(0, 5))           # >= the true positives of any threshold
    return _feed(scores, classes, masks, nt)


def curve_cases():
    rng = np.random.default_rng(41)
    out = {}
    out["single_record"] = CurveCase(1, 10, [_feed([0.5], [0], [0b11111], [1])])
    # class 0: ground truth, no record; class 1: records, no ground truth; class 2: both
    out["gt_only_and_records_only"] = CurveCase(3, 10, [_feed([0.9, 0.8, 0.7, 0.6], [1, 2, 1, 2], [FULL, FULL, 0, 0b11], [3, 0, 2])])
    out["all_tp_and_all_fp"] = CurveCase(2, 10, [_feed(np.linspace(0.95, 0.05, 12), [0, 1] * 6, [FULL, 0] * 6, [6, 4])])
    out["every_score_equal"] = CurveCase(2, 10, [_feed([0.25] * 9, [0, 0, 1, 0, 1, 0, 0, 1, 0], [FULL, 0, 1, 0b111, 0, FULL, 0, 0b11, 1], [5, 3])])
    # the same scores in two feeds: within a tie the first feed's records come first (arrival order)
    a = _feed([0.5, 0.75, 0.5, 0.25], [0, 0, 0, 0], [0, FULL, FULL, 0], [2])
    b = _feed([0.5, 0.75, 0.5, 0.25], [0, 0, 0, 0], [FULL, 0, 0, FULL], [2])
    out["ties_across_two_feeds"] = CurveCase(1, 10, [a, b])
    out["grid_ends"] = CurveCase(1, 10, [_feed([1.0, 1.0, 0.5, 0.001, 0.001], [0] * 5, [FULL, 0, 0b1111, 1, 0], [4])])
    out["one_class_5000"] = CurveCase(2, 10, [_random_feed(rng, 5000, [1], 2, 10, quantum=1 / 512)])
    out["nc80_9000_in_two_feeds"] = CurveCase(80, 10, [_random_feed(rng, 4500, [0, 3, 17, 41, 42, 63, 79], 80, 10, quantum=1 / 256),
                                                       _random_feed(rng, 4500, [0, 3, 17, 41, 42, 63, 79], 80, 10)])
    out["T1"] = CurveCase(3, 1, [_random_feed(rng, 300, [0, 2], 3, 1, quantum=1 / 64)])
    out["T16"] = CurveCase(3, 16, [_random_feed(rng, 300, [0, 1, 2], 3, 16)])
    return out
