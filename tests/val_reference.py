"""Plain references of the validation path's three device stages - prediction decode, batched NMS, COCO matching - and
the constructed inputs that the validation tests (tests/test_val_reference.py, tests/test_hip_val_edges.py) run.

Nothing here touches the HIP library.  The references are written from the operations' definitions
(kod/lightning/experiments/yv5_baseline/layers.py, kod/core/nms.py + torchvision.ops.nms, COCOeval.evaluateImg), not
from the kernels:

* `decode_ref`     fp64 from the fp32 logits.
* `nms_keys_ref`   the candidate list in (row, class) order as the sort keys that `kodhip_nms` documents, and its order.
* `nms_ref`        greedy NMS in numpy fp32, every operation rounded on its own (the library is built without
                   contraction and with IEEE division, so each decision is reproducible bit for bit), ties ordered
                   (score descending, candidate index ascending).
* `match_ref`      fp64, the loop order of COCOeval.evaluateImg.

tests/test_val_reference.py pins them to the oracle (oracle/detection.py, oracle/map_eval.py) on tie-free inputs, so that
the GPU tests compare the kernels with torch's / pycocotools' semantics.  Every case builder returns its inputs together
with facts computed from the references alone (how many candidates, which rank the last survivor had, which matching
events occurred ...); the CPU test asserts them, which is what keeps a GPU test from passing on an input that no longer
reaches the code it was built for.

Decode tolerance.  The yardstick is the fp32 CPU oracle (`oracle.detection.decode`) against `decode_ref` on the decode
cases below: box error per row in fp32 ulps of max(|cx|, |cy|, w, h), score error relative with an absolute floor of
one smallest normal fp32 (a result below it may be flushed to zero).  The device gets twice the measured maximum (another
expf implementation may differ by 1-2 ulp); the CPU test keeps the oracle within half the constant.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from oracle import detection as D

STRIDES = D.STRIDES
ANCHORS = tuple(D.ANCHORS[s] for s in STRIDES)
FLT_MIN = float(np.finfo(np.float32).tiny)

# fp32 CPU oracle vs decode_ref, max over `decode_cases()` (all three rectangular shapes, nc 1 / 2 / 80, B 1 / 3, logits
# with +-20, +-88, +-100, +-inf in every field), measured on an x86-64 host with torch's vectorised CPU sigmoid:
#   box    2.83 ulp32 of the row's max(|cx|, |cy|, w, h)  (worst case 96x64_nc1_b3; every case lies in 1.98 .. 2.83)
#   score  1.178e-7 relative beyond the FLT_MIN floor     (worst case 96x64_nc80_b3; every case in 1.05e-7 .. 1.18e-7)
# Both are recorded rounded UP to the unit they are measured in - 3 ulp, and 2^-23 (one fp32 ulp of a value just above a
# power of two) - so that half the constant, which the CPU test holds the oracle to, does not sit exactly on one
# machine's figure.  The device tolerance is twice the recorded value.
DECODE_BOX_ULP_MEASURED = 3.0
DECODE_SCORE_REL_MEASURED = 2.0 ** -23
DECODE_BOX_ULP = 2 * DECODE_BOX_ULP_MEASURED            # 6 ulp32
DECODE_SCORE_REL = 2 * DECODE_SCORE_REL_MEASURED        # 2^-22 = 2.38e-7

SPECIAL_LOGITS = (20.0, -20.0, 88.0, -88.0, 100.0, -100.0, float("inf"), float("-inf"))


def ulp32(x):
    """spacing of fp32 at |x| (fp64 array in, fp64 array out; the smallest subnormal at 0)"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------ decode
def decode_ref(raws, strides, anchors, img_w, img_h):
    """raws: three [B, A, h, w, 5+nc] fp32 tensors.  -> [B, rows, 5+nc] fp64, rows ordered (level, anchor, y, x):
    xy = (sigmoid * 2 + grid - .5) * stride, wh = (sigmoid * 2)^2 * anchor_px, xyxy corners, sigmoid(obj), sigmoid(cls)."""
    out = []
    for raw, s, anc in zip(raws, strides, anchors):
        B, A, h, w, P = raw.shape
        assert (h, w) == (img_h // s, img_w // s) and A == len(anc)
        sg = torch.sigmoid(raw.double())
        gy = torch.arange(h, dtype=torch.float64).view(1, 1, h, 1)
        gx = torch.arange(w, dtype=torch.float64).view(1, 1, 1, w)
        aw = torch.tensor([a[0] for a in anc], dtype=torch.float64).view(1, A, 1, 1)
        ah = torch.tensor([a[1] for a in anc], dtype=torch.float64).view(1, A, 1, 1)
        cx = (sg[..., 0] * 2 + gx - 0.5) * s
        cy = (sg[..., 1] * 2 + gy - 0.5) * s
        bw = (sg[..., 2] * 2) ** 2 * aw
        bh = (sg[..., 3] * 2) ** 2 * ah
        box = torch.stack((cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), -1)
        out.append(torch.cat((box, sg[..., 4:]), -1).reshape(B, A * h * w, P))
    return torch.cat(out, 1)


def decode_errors(got, ref):
    """got fp32 / ref fp64 [B, rows, 5+nc] tensors -> (max box error in ulp32 of the row's max(|cx|, |cy|, w, h),
    max score error relative beyond the FLT_MIN floor, count of exact-0 / exact-1 scores that `got` misses)."""
    got, ref = got.double().numpy(), ref.numpy()
    b = ref[..., :4]
    cx, cy, w, h = (b[..., 0] + b[..., 2]) / 2, (b[..., 1] + b[..., 3]) / 2, b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]
    scale = ulp32(np.maximum(np.maximum(np.abs(cx), np.abs(cy)), np.maximum(w, h)))
    box = float((np.abs(got[..., :4] - b).max(-1) / scale).max())
    s, g = ref[..., 4:], got[..., 4:]
    over = np.maximum(np.abs(g - s) - FLT_MIN, 0.0)
    rel = float(np.where(over > 0, over / np.where(s != 0, np.abs(s), 1.0), 0.0).max())
    r32 = s.astype(np.float32)
    exact = (r32 == 0) | (r32 == 1)
    missed = int((g[exact] != r32[exact].astype(np.float64)).sum())
    return box, rel, missed


class DecodeCase(NamedTuple):
    width: int
    height: int
    nc: int
    raws: list            # three [B, 3, h, w, 5+nc] fp32
    facts: dict


def decode_case(width, height, nc, B, seed) -> DecodeCase:
    """Random logits (x 2) with each of SPECIAL_LOGITS written once into EVERY field of every level."""
    g = torch.Generator().manual_seed(seed)
    P = 5 + nc
    raws, planted = [], 0
    for s in STRIDES:
        h, w = height // s, width // s
        r = torch.randn(B, 3, h, w, P, generator=g) * 2.0
        flat = r.view(-1, P)
        n = flat.shape[0]
        assert n >= len(SPECIAL_LOGITS)
        for f in range(P):
            for k, v in enumerate(SPECIAL_LOGITS):
                flat[(f * len(SPECIAL_LOGITS) + k) % n, f] = v
                planted += 1
        raws.append(r)
    ref = decode_ref(raws, STRIDES, ANCHORS, width, height)
    r32 = ref[..., 4:].float()
    per_field = min(int((r[..., f] == v).sum()) for r in raws for f in range(P) for v in SPECIAL_LOGITS)
    facts = dict(rectangular=width != height, planted=planted, min_specials_per_field_value=per_field,
                 exact_zero=int((r32 == 0).sum()), exact_one=int((r32 == 1).sum()),
                 subnormal=int(((r32 != 0) & (r32.abs() < FLT_MIN)).sum()), finite=bool(torch.isfinite(ref).all()),
                 rows=ref.shape[1], level_rows=[3 * (height // s) * (width // s) for s in STRIDES])
    return DecodeCase(width, height, nc, raws, facts)


DECODE_SHAPES = ((96, 64), (64, 160), (160, 96))


def decode_cases():
    """name -> (width, height, nc, B, seed): every rectangular shape x nc {1, 2, 80} x B {1, 3}"""
    out = {}
    for i, (w, h) in enumerate(DECODE_SHAPES):
        for j, nc in enumerate((1, 2, 80)):
            for B in (1, 3):
                out[f"{w}x{h}_nc{nc}_b{B}"] = (w, h, nc, B, 100 + 10 * i + 3 * j + B)
    return out


def oracle_decode(case: DecodeCase):
    """the fp32 CPU oracle on a case's logits"""
    from oracle.network import HeadOut, NetOut
    net = NetOut(*[HeadOut(r[..., :4], r[..., 4:5], r[..., 5:]) for r in case.raws])
    return D.decode(net, case.width, case.height)


# --------------------------------------------------------------------------------------------------------------- NMS
def _f32(x):
    return np.asarray(x, dtype=np.float32)


def nms_keys_ref(det, conf, classes=None):
    """det [B, rows, 5+nc] fp32 -> per image (keys, sorted keys), uint64: high word 0xFFFFFFFF - bits(fp32 score), low
    word row * nc + class; score = fp32(cls * obj), kept if obj > conf and score > conf (one class: the same test on its
    only column), candidates listed in (row, class) order.  `classes`: keep the listed class ids only."""
    det = _f32(det)
    conf = np.float32(conf)
    nc = det.shape[2] - 5
    out = []
    for x in det:
        obj = x[:, 4:5]
        score = x[:, 5:] * obj                                        # fp32 product, rounded once
        ok = (obj > conf) & (score > conf)
        if classes is not None:
            ok &= np.isin(np.arange(nc), np.asarray(list(classes)))[None, :]
        row, cls = np.nonzero(ok)                                     # row-major: (row, class) order
        hi = np.uint64(0xFFFFFFFF) - score[row, cls].view(np.uint32).astype(np.uint64)
        keys = (hi << np.uint64(32)) | (row.astype(np.uint64) * np.uint64(nc) + cls.astype(np.uint64))
        out.append((keys, np.sort(keys)))
    return out


def _order(keys, index_desc=False):
    """(score desc, candidate index asc) - or index desc, the rule the tie cases are told apart from"""
    if not index_desc:
        return np.sort(keys)
    hi, lo = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
    return keys[np.lexsort((-lo.astype(np.int64), hi))]


def nms_ref(det, conf, thr, max_det=300, max_nms=30000, max_wh=4096, key_cap=None, classes=None, index_desc=False,
            info=None):
    """Greedy NMS, fp32.  -> list of [n <= max_det, 6] fp32 rows (x1, y1, x2, y2, score, class).  `key_cap`: only the
    first key_cap candidates in (row, class) order take part.  `info` (a list) receives per image a dict: candidates,
    last_rank (sorted rank of the last survivor, -1 without one), consumed_all (the walk reached the last candidate)."""
    det = _f32(det)
    nc = det.shape[2] - 5
    thr, max_wh = np.float32(thr), np.float32(max_wh)
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for x, (keys, _) in zip(det, nms_keys_ref(det, conf, classes)):
            if key_cap is not None:
                keys = keys[:key_cap]
            order = _order(keys, index_desc)[:max_nms]
            idx = (order & np.uint64(0xFFFFFFFF)).astype(np.int64)
            row, cls = idx // nc, idx % nc
            raw = x[row, :4]
            score = x[row, 5 + cls] * x[row, 4]
            box = raw + (cls.astype(np.float32) * max_wh)[:, None]     # fp32(box + fp32(cls * max_wh))
            area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
            kb = np.zeros((max_det, 4), np.float32)
            ka = np.zeros(max_det, np.float32)
            kept, last = [], -1
            i = 0
            for i in range(len(idx)):
                if len(kept) == max_det:
                    break
                n = len(kept)
                w = np.maximum(np.float32(0), np.minimum(kb[:n, 2], box[i, 2]) - np.maximum(kb[:n, 0], box[i, 0]))
                h = np.maximum(np.float32(0), np.minimum(kb[:n, 3], box[i, 3]) - np.maximum(kb[:n, 1], box[i, 1]))
                inter = w * h
                if bool((inter / (ka[:n] + area[i] - inter) > thr).any()):            # NaN never suppresses
                    continue
                kb[n], ka[n] = box[i], area[i]
                kept.append(i)
                last = i
            else:
                i = len(idx)
            k = np.asarray(kept, dtype=np.int64)
            out.append(np.concatenate((raw[k], score[k, None], cls[k, None].astype(np.float32)), 1).reshape(-1, 6))
            if info is not None:
                info.append(dict(candidates=len(keys), last_rank=last, consumed_all=i >= len(idx), kept_ranks=k))
    return out


def _grid_boxes(n, size=10.0, pitch=20.0, per_row=25):
    """n mutually non-overlapping boxes on a grid"""
    k = np.arange(n)
    x, y = (k % per_row) * pitch, (k // per_row) * pitch
    return np.stack((x, y, x + size, y + size), 1).astype(np.float32)


def _det_from(rows_boxes, obj, cls):
    """[rows, 4], [rows], [rows, nc] -> [rows, 5+nc] fp32"""
    return np.concatenate((_f32(rows_boxes), _f32(obj)[:, None], _f32(cls)), 1)


SORT_COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8193, 9600)


def sort_reach_case(seed=5):
    """[10, 1200, 5+8], conf 0.1: image b has exactly SORT_COUNTS[b] candidates, on rows scattered over both
    1024-row iterations of the compaction; rows that are switched off have obj = 0, the ragged last row of an image has
    obj > conf with cls * obj <= conf on the classes left out.  -> (det, conf, thr, facts)"""
    rng = np.random.default_rng(seed)
    B, rows, nc, conf = len(SORT_COUNTS), 1200, 8, 0.1
    det = np.zeros((B, rows, 5 + nc), np.float32)
    c = rng.uniform(40, 600, (B, rows, 2)); wh = rng.uniform(8, 90, (B, rows, 2))
    det[..., 0:2], det[..., 2:4] = c - wh / 2, c + wh / 2
    for b, n in enumerate(SORT_COUNTS):
        full, rest = divmod(n, nc)
        on = rng.permutation(rows)[:full + (1 if rest else 0)]
        det[b, on, 4] = rng.uniform(0.6, 1.0, len(on))
        det[b, on, 5:] = rng.uniform(0.3, 1.0, (len(on), nc))
        if rest:
            drop = rng.permutation(nc)[:nc - rest]
            det[b, on[-1], 5 + drop] = 0.01
    keys = nms_keys_ref(det, conf)
    info = []
    nms_ref(det, conf, 0.45, info=info)
    low = (det[..., 4:5] > np.float32(conf)) & (det[..., 5:] * det[..., 4:5] <= np.float32(conf))
    facts = dict(counts=[len(k) for k, _ in keys], tie_pairs=sum(int(len(k) - len(np.unique(k >> np.uint64(32)))) for k, _ in keys),
                 obj_passes_score_fails=int(low.sum()),
                 rows_used_beyond_1024=[int((det[b, 1024:, 4] > 0).sum()) for b in range(B)],
                 last_rank=[i["last_rank"] for i in info])
    return det, conf, 0.45, facts


def _cluster_image(rng, rows, nc, n_early, n_late, clusters_early, clusters_late, jitters):
    """rows x one passing class each: `n_early` rows with scores in (0.3, 1) over `clusters_early` (centre, class) clusters
    and `n_late` rows with scores in (0.02, 0.05) over `clusters_late` further ones; a row's box is its cluster's 50 px
    box moved by a jitter drawn from `jitters` (px)."""
    x = np.zeros((rows, 5 + nc), np.float32)
    x[:, 0:4] = (0, 0, 1, 1)
    n = n_early + n_late
    assert n <= rows and clusters_early + clusters_late <= 40 * nc
    where = rng.permutation(rows)[:n]
    cl = np.concatenate((np.arange(n_early) % clusters_early, clusters_early + np.arange(n_late) % max(clusters_late, 1)))
    cl[:n_early] = rng.permutation(cl[:n_early])
    centre, cls = cl // nc, cl % nc
    cx, cy = 40 + (centre % 8) * 75.0, 40 + (centre // 8) * 75.0
    j = rng.choice(np.asarray(jitters, dtype=np.float64), n)[:, None] * rng.uniform(-1, 1, (n, 4))
    box = np.stack((cx - 25, cy - 25, cx + 25, cy + 25), 1) + j
    x[where, 0:4] = box
    x[where, 4] = np.concatenate((rng.uniform(0.6, 1.0, n_early), rng.uniform(0.2, 0.25, n_late)))
    x[where, 5 + cls] = np.concatenate((rng.uniform(0.5, 1.0, n_early), rng.uniform(0.1, 0.2, n_late)))
    return x


def cluster_case(seed=7):
    """[4, 10000, 5+8], conf 0.01, thr 0.45; boxes clustered around 40 centres per class:
    image 0  290 tight clusters in 9000 high-scoring rows, 30 more in 600 low-scoring ones: survivors 291..300 come after
             rank 9000 (> 8192), the walk stops at exactly 300;
    image 1  the same with 4500 + 300 rows: the last survivor beyond rank 4096;
    image 2  200 clusters, mixed jitter, 3000 rows: every candidate consumed, fewer than 300 survivors;
    image 3  320 clusters, mixed jitter, 6000 rows: 300 reached early.          -> (det, conf, thr, facts)"""
    rng = np.random.default_rng(seed)
    rows, nc = 10000, 8
    det = np.stack((_cluster_image(rng, rows, nc, 9000, 600, 290, 30, (1.0,)),
                    _cluster_image(rng, rows, nc, 4500, 300, 290, 30, (1.0,)),
                    _cluster_image(rng, rows, nc, 3000, 0, 200, 0, (0.5, 4.0, 9.0)),
                    _cluster_image(rng, rows, nc, 6000, 0, 320, 0, (0.5, 4.0, 9.0))))
    info = []
    res = nms_ref(det, 0.01, 0.45, info=info)
    facts = dict(candidates=[i["candidates"] for i in info], last_rank=[i["last_rank"] for i in info],
                 consumed_all=[i["consumed_all"] for i in info], survivors=[len(r) for r in res],
                 suppressed_before_last=[i["last_rank"] + 1 - len(r) for i, r in zip(info, res)])
    return det, 0.01, 0.45, facts


def ties_case(seed=11):
    """[2, 600, 5+4], conf 0.25, thr 0.45: obj and cls are multiples of 1/16 (scores collide all the time), boxes
    clustered so that which of two equal-scored candidates goes first decides who survives.  -> (det, conf, thr, facts)"""
    rng = np.random.default_rng(seed)
    B, rows, nc = 2, 600, 4
    det = np.zeros((B, rows, 5 + nc), np.float32)
    centre = rng.integers(0, 24, (B, rows))
    cx, cy = 60 + (centre % 6) * 90.0, 60 + (centre // 6) * 90.0
    j = rng.integers(-12, 13, (B, rows, 4)).astype(np.float64)
    det[..., 0:4] = np.stack((cx - 30, cy - 30, cx + 30, cy + 30), -1) + j
    det[..., 4] = rng.integers(6, 17, (B, rows)) / 16.0
    det[..., 5:] = rng.integers(0, 17, (B, rows, nc)) / 16.0
    conf, thr = 0.25, 0.45
    keys = nms_keys_ref(det, conf)
    tied = total = 0
    for k, _ in keys:
        _, inv, cnt = np.unique(k >> np.uint64(32), return_inverse=True, return_counts=True)
        tied += int((cnt[inv] > 1).sum()); total += len(k)
    asc, desc = nms_ref(det, conf, thr), nms_ref(det, conf, thr, index_desc=True)
    facts = dict(candidates=total, tied=tied, tied_share=tied / total,
                 rule_changes_survivors=[not np.array_equal(a, d) for a, d in zip(asc, desc)],
                 score_equals_conf=int(((det[..., 5:] * det[..., 4:5] == np.float32(conf)) & (det[..., 4:5] > conf)).sum()))
    return det, conf, thr, facts


class HandCase(NamedTuple):
    det: np.ndarray        # [1, rows, 5+nc]
    conf: float
    thr: float
    kept_rows: list        # the det rows expected to survive, in output order (the issue's table)
    kwargs: dict           # max_nms ...


def _one_hot_det(boxes, scores, classes, nc, obj=1.0):
    """rows with obj = `obj` and cls = score / obj on one class (obj 1.0: the score passes through exactly)"""
    boxes = _f32(boxes).reshape(-1, 4)
    n = len(boxes)
    cls = np.zeros((n, nc), np.float32)
    cls[np.arange(n), np.asarray(classes)] = _f32(scores) / np.float32(obj)
    return _det_from(boxes, np.full(n, obj, np.float32), cls)[None]


def _offset_pair(seed=3):
    """Two class-79 boxes with fractional coordinates whose suppression decision at thr 0.45 differs between the fp32
    arithmetic on offset boxes (79 * 4096 = 323584: fp32 spacing 1/32 px) and exact arithmetic on the raw boxes."""
    rng = np.random.default_rng(seed)
    for _ in range(200000):
        a = np.array([100.3, 200.7, 150.9, 260.1]) + rng.uniform(-1, 1, 4)
        d = rng.uniform(9.0, 12.5, 2)
        b = a + np.array([d[0], d[1], d[0], d[1]]) + rng.uniform(-0.5, 0.5, 4)
        a32, b32 = _f32(a), _f32(b)
        A, Bx = a32.astype(np.float64), b32.astype(np.float64)
        iw, ih = min(A[2], Bx[2]) - max(A[0], Bx[0]), min(A[3], Bx[3]) - max(A[1], Bx[1])
        inter = max(iw, 0) * max(ih, 0)
        exact = inter / ((A[2] - A[0]) * (A[3] - A[1]) + (Bx[2] - Bx[0]) * (Bx[3] - Bx[1]) - inter)
        if abs(exact - 0.45) > 5e-4:
            continue
        det = _one_hot_det([a32, b32], [0.9, 0.8], [79, 79], 80)
        if (len(nms_ref(det, 0.25, 0.45)[0]) == 1) != (exact > np.float64(np.float32(0.45))):
            return det, exact
    raise AssertionError("no pair found")


def hand_cases():
    """name -> HandCase: the decisions of the issue's table, one or two boxes each"""
    pair = [[0, 0, 10, 10], [0, 0, 10, 20]]                            # IoU = 100 / 200 exactly
    out = {
        "iou_equals_thr": HandCase(_one_hot_det(pair, [0.9, 0.8], [1, 1], 3), 0.25, 0.5, [0, 1], {}),
        "iou_above_thr": HandCase(_one_hot_det(pair, [0.9, 0.8], [1, 1], 3), 0.25, 0.49, [0], {}),
        "same_box_two_classes": HandCase(_one_hot_det([pair[0], pair[0]], [0.9, 0.8], [0, 2], 3), 0.25, 0.45, [0, 1], {}),
        "score_equals_conf": HandCase(_one_hot_det([pair[0], [50, 50, 60, 60]], [0.25, 0.5], [1, 1], 3, obj=0.5), 0.25, 0.45, [1], {}),
        "obj_passes_score_fails": HandCase(_one_hot_det([pair[0], [50, 50, 60, 60]], [0.18, 0.45], [1, 1], 3, obj=0.9), 0.25, 0.45, [1], {}),
        # two identical zero-area boxes (0 / 0) inside a real one (0 / area), a degenerate line on its edge
        "zero_area": HandCase(_one_hot_det([[5, 5, 5, 5], [0, 0, 10, 10], [5, 5, 5, 5], [0, 3, 0, 8]], [0.9, 0.8, 0.7, 0.6], [1] * 4, 3),
                              0.25, 0.45, [0, 1, 2, 3], {}),
    }
    det, _ = _offset_pair()
    out["class79_offset_rounding"] = HandCase(det, 0.25, 0.45, list(range(len(nms_ref(det, 0.25, 0.45)[0]))), {})
    # ranks 0 .. 69 disjoint, descending scores; rank 5 overlaps rank 2 (same 64-lane batch), rank 69 overlaps rank 0
    # (kept in the batch before) and rank 68 overlaps rank 66 (second batch, same batch)
    b = _grid_boxes(70)
    b[5] = b[2] + np.float32(1)
    b[69] = b[0] + np.float32(1)
    b[68] = b[66] + np.float32(1)
    sc = 0.95 - 0.01 * np.arange(70)
    out["batches"] = HandCase(_one_hot_det(b, sc, [1] * 70, 3), 0.2, 0.45, [r for r in range(70) if r not in (5, 68, 69)], {})
    return out


def cap_cases():
    """name -> HandCase around max_det (299 / 300 / 301 disjoint candidates), max_nms and nc = 1"""
    out = {}
    for n in (299, 300, 301):
        sc = 0.99 - 0.002 * np.arange(n)
        out[f"disjoint_{n}"] = HandCase(_one_hot_det(_grid_boxes(n), sc, [0] * n, 2), 0.25, 0.45, list(range(min(n, 300))), {})
    n = 120
    sc = 0.99 - 0.002 * np.arange(n)
    out["max_nms_100"] = HandCase(_one_hot_det(_grid_boxes(n), sc, [0] * n, 2), 0.25, 0.45, list(range(100)), dict(max_nms=100))
    # one class: rows 0 / 1 overlap (1 suppressed), row 2 has obj > conf and cls * obj <= conf, row 3 obj <= conf
    d = _det_from([[0, 0, 10, 10], [1, 1, 11, 11], [30, 30, 40, 40], [60, 60, 70, 70], [90, 90, 99, 99]],
                  [0.9, 0.8, 0.5, 0.2, 0.6], [[0.9], [0.9], [0.4], [1.0], [0.5]])[None]
    out["one_class"] = HandCase(d, 0.25, 0.45, [0, 4], {})
    return out


def key_cap_case(seed=13):
    """[2, 200, 5+6], conf 0.2: about 1000 candidates per image against key_cap = 256; the high-scoring rows sit at the END
    of the image, so dropping the candidates beyond the cap (instead of the lowest scores) changes the result."""
    rng = np.random.default_rng(seed)
    B, rows, nc = 2, 200, 6
    det = np.zeros((B, rows, 5 + nc), np.float32)
    c = rng.uniform(40, 600, (B, rows, 2)); wh = rng.uniform(20, 120, (B, rows, 2))
    det[..., 0:2], det[..., 2:4] = c - wh / 2, c + wh / 2
    det[..., 4] = np.linspace(0.6, 1.0, rows)[None, :]
    det[..., 5:] = rng.uniform(0.25, 1.0, (B, rows, nc))
    capped, free = nms_ref(det, 0.2, 0.45, key_cap=256), nms_ref(det, 0.2, 0.45)
    facts = dict(candidates=[len(k) for k, _ in nms_keys_ref(det, 0.2)],
                 cap_changes_result=[not np.array_equal(a, b) for a, b in zip(capped, free)])
    return det, 0.2, 0.45, facts


def wrapper_case(seed=17):
    """[3, 500, 5+6] clustered, for the wrapper's `classes=` filter and a non-contiguous input"""
    rng = np.random.default_rng(seed)
    B, rows, nc = 3, 500, 6
    det = np.zeros((B, rows, 5 + nc), np.float32)
    centre = rng.integers(0, 30, (B, rows))
    cx, cy = 60 + (centre % 6) * 90.0, 60 + (centre // 6) * 90.0
    det[..., 0:4] = np.stack((cx - 30, cy - 30, cx + 30, cy + 30), -1) + rng.uniform(-10, 10, (B, rows, 4))
    det[..., 4] = rng.uniform(0.1, 1.0, (B, rows))
    det[..., 5:] = rng.uniform(0.0, 1.0, (B, rows, nc))
    return det, 0.25, 0.45


# ---------------------------------------------------------------------------------------------------------- matching
def match_ref(det, ndet, gt, gt_label, gt_start, nc, thrs, max_per_class, events=None):
    """COCOeval.evaluateImg per image and class, fp64: detections in the given (descending score) order, the first
    `max_per_class` of a class are counted; each takes the still-free ground truth of its class with the highest
    IoU >= min(thr, 1 - 1e-10), the LATER one of equals.  det [B, max_det, 6] fp32, ndet [B], gt [n, 4] fp64,
    gt_label [n], gt_start [B+1].  -> tp [B, max_det, T] uint8, counted [B, max_det] uint8.
    `events` (a dict) counts: exact_thr, equal_iou, stolen, over_budget, matched_index (set of in-image gt indices)."""
    det = _f32(det)
    B, max_det, _ = det.shape
    T = len(thrs)
    tp = np.zeros((B, max_det, T), np.uint8)
    counted = np.zeros((B, max_det), np.uint8)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    gt_label = np.asarray(gt_label, dtype=np.int64)
    ev = events if events is not None else {}
    for k in ("exact_thr", "equal_iou", "stolen", "over_budget"):
        ev.setdefault(k, 0)
    ev.setdefault("matched_index", set())
    for b in range(B):
        nd = min(int(ndet[b]), max_det)
        g0, g1 = int(gt_start[b]), int(gt_start[b + 1])
        d = det[b, :nd].astype(np.float64)
        cls = det[b, :nd, 5].astype(np.int64)
        for c in np.unique(cls):
            di = np.nonzero(cls == c)[0]
            counted[b, di[:max_per_class]] = 1
            ev["over_budget"] += max(len(di) - max_per_class, 0)
            di = di[:max_per_class]
            gi = g0 + np.nonzero(gt_label[g0:g1] == c)[0]
            if not len(gi):
                continue
            G = gt[gi]
            ad = (d[di, 2] - d[di, 0]) * (d[di, 3] - d[di, 1])
            ag = (G[:, 2] - G[:, 0]) * (G[:, 3] - G[:, 1])
            w = np.clip(np.minimum(d[di, None, 2], G[None, :, 2]) - np.maximum(d[di, None, 0], G[None, :, 0]), 0, None)
            h = np.clip(np.minimum(d[di, None, 3], G[None, :, 3]) - np.maximum(d[di, None, 1], G[None, :, 1]), 0, None)
            inter = w * h
            with np.errstate(invalid="ignore", divide="ignore"):
                iou = inter / (ad[:, None] + ag[None, :] - inter)
            for ti, t in enumerate(thrs):
                used = np.zeros(len(gi), bool)
                for a in range(len(di)):
                    best, m = min(t, 1 - 1e-10), -1
                    for q in range(len(gi)):
                        if used[q]:
                            continue
                        if iou[a, q] < best:
                            continue
                        if m >= 0 and iou[a, q] == best:
                            ev["equal_iou"] += 1
                        best, m = iou[a, q], q
                    if m >= 0:
                        used[m] = True
                        tp[b, di[a], ti] = 1
                        ev["matched_index"].add(int(gi[m] - g0))
                        ev["exact_thr"] += int(iou[a, m] == t)
                    top = int(np.argmax(iou[a]))
                    if iou[a, top] >= min(t, 1 - 1e-10) and used[top] and m != top:
                        ev["stolen"] += 1
    return tp, counted


def per_image_records(det, ndet, tp, counted, gt_label, gt_start, nc):
    """(tp, counted) -> the per-image records oracle.map_eval.accumulate takes: per class (scores, matched [T, m], n_gt)"""
    det = _f32(det)
    gt_label = np.asarray(gt_label, dtype=np.int64)
    out = []
    for b in range(det.shape[0]):
        nd = min(int(ndet[b]), det.shape[1])
        lab = gt_label[int(gt_start[b]):int(gt_start[b + 1])]
        img = []
        for c in range(nc):
            r = np.nonzero((det[b, :nd, 5].astype(np.int64) == c) & (counted[b, :nd] != 0))[0]
            img.append((det[b, r, 4].astype(np.float64), tp[b, r].T.astype(bool), int((lab == c).sum())))
        out.append(img)
    return out


THRS4 = (0.3, 0.5, 0.75, 0.9)
THRS8 = (0.3, 0.4, 0.5, 0.55, 0.6, 0.75, 0.9, 0.95)
BITMAP_INDICES = (0, 63, 64, 127, 128, 255)


class MatchCase(NamedTuple):
    nc: int
    thrs: tuple
    dets: list             # per image [n, 6] fp32, descending score
    gts: list              # per image ([m, 4] fp64, [m] int64)
    facts: dict


def _pack(dets, gts, max_det=None, ndet=None):
    """per-image lists -> the arrays of the kodhip_map_match ABI"""
    B = len(dets)
    max_det = max_det or max([len(d) for d in dets] + [1])
    det = np.zeros((B, max_det, 6), np.float32)
    for b, d in enumerate(dets):
        det[b, :min(len(d), max_det)] = d[:max_det]
    nd = np.asarray([len(d) for d in dets] if ndet is None else ndet, dtype=np.int32)
    gt = np.concatenate([g.reshape(-1, 4) for g, _ in gts]).astype(np.float64)
    lab = np.concatenate([l.reshape(-1) for _, l in gts]).astype(np.int64)
    start = np.concatenate(([0], np.cumsum([len(l) for _, l in gts]))).astype(np.int32)
    return det, nd, gt, lab, start


def match_case(nc, thrs) -> MatchCase:
    """The hand-built batch.  Four class ids (0, 63, 64, 79 with 80 classes; 0, 1, 0, 1 with two) and per image:
    0  one ground truth and one detection per threshold with IoU = that threshold exactly (10 x 10 t inside 10 x 10);
    1  two ground truths with the same IoU to the first detection, a second detection that fits only the EARLIER one;
       a ground truth that a higher-scoring detection takes (IoU 0.8) from a better-fitting later one (IoU 0.95);
    2  130 detections of one class interleaved with 40 of another, each on its own ground truth: 101 .. 130 uncounted;
    3  256 ground truths; two detections (the second a lower-scoring duplicate) on each of BITMAP_INDICES and some others;
    4  ground truths, no detections;
    5  detections, no ground truths (the last image)."""
    cA, cB, cC, cD = (0, 63, 64, 79) if nc >= 80 else (0, 1 % nc, 0, 1 % nc)
    f64, i64 = np.float64, np.int64
    dets, gts = [], []
    # image 0
    g = np.array([[100.0 * i, 0, 100.0 * i + 10, 10] for i in range(len(thrs))], f64)
    d = [[100.0 * i, 0, 100.0 * i + 10, 10 * t, 0.9 - 0.01 * i, cB] for i, t in enumerate(thrs)]
    assert all(float(np.float32(10 * t)) == 10 * t for t in thrs)
    dets.append(_f32(d)); gts.append((g, np.full(len(g), cB, i64)))
    # image 1
    g = np.array([[5, 0, 15, 10], [15, 0, 25, 10], [100, 100, 200, 200]], f64)
    d = [[10, 0, 20, 10, 0.9, cC], [4, 0, 14, 10, 0.8, cC],
         [100, 100, 200, 180, 0.7, cD], [100, 100, 200, 195, 0.6, cD], [300, 300, 310, 310, 0.5, cA]]
    dets.append(_f32(d)); gts.append((g, np.array([cC, cC, cD], i64)))
    # image 2: class cA 130 times, class cD 40 times in between, scores descending over the whole list
    n = 170
    kind = np.where(np.arange(n) % 4 == 3, cD, cA)[:n]
    kind[160:] = cA
    boxes = _grid_boxes(n).astype(f64)
    d = np.concatenate((boxes, (0.95 - 0.005 * np.arange(n))[:, None], kind[:, None].astype(f64)), 1)
    dets.append(_f32(d)); gts.append((boxes.copy(), kind.astype(i64)))
    # image 3
    g = _grid_boxes(256, per_row=16).astype(f64)
    lab = np.where(np.arange(256) % 3 == 0, cA, cC).astype(i64)
    hit = list(BITMAP_INDICES) + [1, 31, 32, 65, 191, 192, 254]
    lab[list(BITMAP_INDICES)] = cB
    d = [[*g[k], 0.9 - 0.001 * i, lab[k]] for i, k in enumerate(hit)] + [[*g[k], 0.5 - 0.001 * i, lab[k]] for i, k in enumerate(hit)]
    dets.append(_f32(d)); gts.append((g, lab))
    # images 4, 5
    dets.append(np.zeros((0, 6), np.float32)); gts.append((np.array([[0, 0, 10, 10], [20, 20, 40, 40]], f64), np.array([cA, cD], i64)))
    dets.append(_f32([[0, 0, 10, 10, 0.9, cA], [20, 20, 40, 40, 0.8, cD]])); gts.append((np.zeros((0, 4), f64), np.zeros(0, i64)))
    ev = {}
    det, nd, gt, lab, start = _pack(dets, gts)
    tp, counted = match_ref(det, nd, gt, lab, start, nc, thrs, 100, events=ev)
    facts = dict(ev, classes=sorted({cA, cB, cC, cD}), lanes=nc * len(thrs), tp=int(tp.sum()), counted=int(counted.sum()),
                 over_budget_tp=int(tp[2][counted[2] == 0].sum()), duplicates_tp=int(tp[3, len(hit):2 * len(hit)].sum()),
                 firsts_tp=int(tp[3, :len(hit)].sum()), expected_firsts=len(hit) * len(thrs),
                 equal_pair_second_tp=int(tp[1, 1, 0]), max_gt=max(len(l) for _, l in gts))
    return MatchCase(nc, tuple(thrs), dets, gts, facts)


def random_scene(rng, nc, n_img, size=320, quantum=None):
    """Random ground truths, jittered detections of them (some with the wrong class) and false positives; scores
    continuous, or multiples of `quantum` (ties within and across images).  -> (dets, gts) per image"""
    dets, gts = [], []
    for _ in range(n_img):
        n = int(rng.integers(0, 8))
        c = rng.uniform(20, size - 20, (n, 2)); wh = rng.uniform(10, 120, (n, 2))
        gt = np.concatenate((c - wh / 2, c + wh / 2), 1)
        lab = rng.integers(0, nc, n)
        rows = []
        for b, l in zip(gt, lab):
            for _ in range(int(rng.integers(0, 3))):
                rows.append([*(b + rng.normal(0, 6, 4)), rng.uniform(0.05, 1.0), l if rng.random() < 0.8 else rng.integers(0, nc)])
        for _ in range(int(rng.integers(0, 150))):
            c2 = rng.uniform(0, size, 2); wh2 = rng.uniform(5, 80, 2)
            rows.append([*(c2 - wh2 / 2), *(c2 + wh2 / 2), rng.uniform(0.001, 0.6), rng.integers(0, min(nc, 2))])
        d = np.array(rows, dtype=np.float32).reshape(-1, 6)
        if quantum:
            d[:, 4] = np.ceil(d[:, 4] / quantum) * quantum
        d = d[np.argsort(-d[:, 4], kind="mergesort")][:300]
        dets.append(d); gts.append((gt, lab.astype(np.int64)))
    return dets, gts


def evaluator_batches(seed=19, nc=5):
    """Three batches of four images for DeviceMAPEvaluator: scores are multiples of 1/8 (ties across images and batches),
    class 3 has detections and no ground truth anywhere, class 4 ground truths and no detection.
    -> (batches [(dets, gts)], facts)"""
    from oracle import map_eval as M
    rng = np.random.default_rng(seed)
    batches = []
    for _ in range(3):
        dets, gts = random_scene(rng, 3, 4, quantum=0.125)
        for i, (g, l) in enumerate(gts):                                  # class 4: ground truth only
            gts[i] = (np.concatenate((g, [[5.0, 5, 50, 50]])), np.concatenate((l, [4])))
        for i, d in enumerate(dets):                                      # class 3: detections only
            extra = _f32([[10, 10, 60, 60, 0.5, 3], [100, 100, 160, 160, 0.25, 3]])
            d = np.concatenate((d, extra))
            dets[i] = d[np.argsort(-d[:, 4], kind="mergesort")]
        batches.append((dets, gts))
    per_image = []
    for dets, gts in batches:
        det, nd, gt, lab, start = _pack(dets, gts)
        tp, counted = match_ref(det, nd, gt, lab, start, nc, THRS4, 100)
        per_image += per_image_records(det, nd, tp, counted, lab, start, nc)
    ap, ap_rev = M.accumulate(per_image, nc), M.accumulate(per_image[::-1], nc)
    mixed = 0
    for c in range(nc):
        seen = {}
        for i, img in enumerate(per_image):
            for s, t in zip(img[c][0], img[c][1][1]):
                seen.setdefault(float(s), set()).add((i, bool(t)))
        mixed += sum(1 for v in seen.values() if len({i for i, _ in v}) > 1 and len({t for _, t in v}) > 1)
    facts = dict(cross_image_tie_groups_with_mixed_tp=mixed, order_matters=not np.array_equal(ap, ap_rev, equal_nan=True),
                 dets_without_gt=bool(np.isnan(ap[:, 3]).all()) and sum(len(img[3][0]) for img in per_image) > 0,
                 gt_without_dets=bool((ap[:, 4] == 0).all()) and sum(len(img[4][0]) for img in per_image) == 0)
    return batches, per_image, facts
