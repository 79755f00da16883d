"""Plain reference of weighted boxes fusion (WBF; Solovyev, Wang, Gabruseva 2021) as kodhip_fuse_detections defines it, and the
constructed inputs that tests/test_fusion_reference.py (CPU) and tests/test_hip_fusion.py (GPU) run.

Nothing here touches the HIP library.  `fuse_ref` is written from the definition, not from the kernel: a plain loop over the
sorted candidates, fp32 with every operation rounded on its own (numpy float32 arithmetic, element by element over the
clusters that exist).  Per image:

* W = the sum of the image's view weights, added in view order.
* a row of view v with score s is a candidate iff t = fl(s * w[v]) > 0; candidates by t descending, equal t by view, then rank.
* a candidate (box b, class c) meets every cluster of class c (every cluster when agnostic) through the cluster's CURRENT
  fused box F: inter = fl(w * h) with w, h clamped at 0, an empty intersection never matches, iou = fl(inter / fl(fl(area_F +
  area_b) - inter)); it joins the cluster of largest iou > thr (strict; NaN never; equal IoUs: the cluster created first):
  acc = fl(acc + fl(t * x)) per coordinate, st = fl(st + t), n += 1, F = fl(acc / st).
* without a match it opens a cluster: F = its own floats, acc = fl(t * x), st = t, n = 1, class c.
* final score = fl(fl(st / n) * fl(min(n, W) / W)); output by that score descending, equal scores by creation order, the first
  max_det.

Every case builder returns its inputs together with facts computed from the reference alone; the CPU test asserts them,
which keeps a GPU test from passing on an input that no longer reaches what it was built for.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

F32 = np.float32


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def fuse_ref(rows, counts, view_start, weights=None, thr=0.55, agnostic=False, max_det=300, info=None):
    """rows [V, max_rows, 6] fp32, counts [V], view_start [n_images + 1], weights [V] or None -> list of [n <= max_det, 6]
    fp32.  `info` (a list) receives per image dict(candidates, clusters, not_first: joins whose cluster was not the first one
    over the threshold, crowded: clusters with more members than W, reordered: final order differs from creation order,
    cut: clusters beyond max_det)."""
    rows, thr = _f32(rows), F32(thr)
    V, max_rows = rows.shape[:2]
    wts = np.ones(V, F32) if weights is None else _f32(weights).reshape(-1)
    out = []
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(len(view_start) - 1):
            v0, v1 = int(view_start[i]), int(view_start[i + 1])
            W = F32(0)
            cand = []                                              # (key, t, row)
            for v in range(v0, v1):
                W = F32(W + wts[v])
                for r in range(max(0, min(int(counts[v]), max_rows))):
                    t = F32(rows[v, r, 4] * wts[v])
                    if t > 0:                                      # (False for NaN)
                        hi = 0xFFFFFFFF - int(np.asarray(t).view(np.uint32))
                        cand.append(((hi << 32) | ((v - v0) * max_rows + r), t, rows[v, r]))
            cand.sort(key=lambda c: c[0])
            cap = max(1, len(cand))
            F, acc = np.zeros((cap, 4), F32), np.zeros((cap, 4), F32)
            st, cnt, cls = np.zeros(cap, F32), np.zeros(cap, np.int64), np.zeros(cap, F32)
            nc = not_first = 0
            for _, t, row in cand:
                b, c = row[:4], row[5]
                best = -1
                if nc:
                    f = F[:nc]
                    w = np.maximum(F32(0), np.minimum(f[:, 2], b[2]) - np.maximum(f[:, 0], b[0]))
                    h = np.maximum(F32(0), np.minimum(f[:, 3], b[3]) - np.maximum(f[:, 1], b[1]))
                    inter = w * h
                    area_f = (f[:, 2] - f[:, 0]) * (f[:, 3] - f[:, 1])
                    area_b = F32(F32(b[2] - b[0]) * F32(b[3] - b[1]))
                    iou = inter / ((area_f + area_b) - inter)
                    ok = (inter > 0) & (iou > thr)                 # NaN never matches
                    if not agnostic:
                        ok &= cls[:nc] == c
                    if ok.any():
                        best = int(np.argmax(np.where(ok, iou, F32(-1))))      # the first of equal maxima
                        not_first += best != int(np.nonzero(ok)[0][0])
                if best >= 0:
                    acc[best] = acc[best] + t * b
                    st[best] = st[best] + t
                    cnt[best] += 1
                    F[best] = acc[best] / st[best]
                else:
                    F[nc], acc[nc], st[nc], cnt[nc], cls[nc] = b, t * b, t, 1, c
                    nc += 1
            n = cnt[:nc].astype(F32)
            score = (st[:nc] / n) * (np.minimum(n, W) / W)
            keys = ((np.uint64(0xFFFFFFFF) - score.view(np.uint32).astype(np.uint64)) << np.uint64(32)) | np.arange(nc, dtype=np.uint64)
            order = np.argsort(keys, kind="stable")
            res = np.concatenate((F[:nc], score[:, None], cls[:nc, None]), 1)[order][:max_det]
            out.append(_f32(res).reshape(-1, 6))
            if info is not None:
                info.append(dict(candidates=len(cand), clusters=nc, not_first=int(not_first), crowded=int((n > W).sum()),
                                 reordered=bool((order != np.arange(nc)).any()), cut=max(0, nc - max_det)))
    return out


def pack_views(views, max_rows, fill=np.nan):
    """list of [n_v, 6] arrays -> (rows [V, max_rows, 6] with `fill` beyond each count, counts int32 [V])"""
    rows = np.full((len(views), max_rows, 6), fill, np.float32)
    counts = np.zeros(len(views), np.int32)
    for v, r in enumerate(views):
        r = _f32(r).reshape(-1, 6)
        rows[v, :len(r)], counts[v] = r, len(r)
    return rows, counts


class FuseCase(NamedTuple):
    rows: np.ndarray
    counts: np.ndarray
    view_start: np.ndarray
    max_rows: int


THR = 0.55
MIXED = (1.0, 0.5, 2.0, 0.75, 1.25, 1.0, 0.6, 1.5)
OPTIONS = [(weights, agnostic, max_det) for weights in ("unit", "mixed") for agnostic in (False, True) for max_det in (300, 7)]


def case_weights(case: FuseCase, kind):
    """one weight per view: all ones, or MIXED by the view's position in its image"""
    if kind == "unit":
        return np.ones(len(case.counts), np.float32)
    s = case.view_start
    return _f32([MIXED[(v - s[i]) % len(MIXED)] for i in range(len(s) - 1) for v in range(s[i], s[i + 1])])


def _ensemble_views(rng, n_models, n_objects, canvas, max_rows, nc=3, lo=None, twice=0.25):
    """n_models views of the same n_objects: every model jitters box and score, misses some objects, reports some twice and adds
    false positives; every third object sits about a third of its width beside a neighbour of its class.  `lo`: at least that
    many rows per view (padded with false positives), at most max_rows; `twice`: the share of objects a model reports twice."""
    size = rng.uniform(40, 160, (n_objects, 2))
    centre = rng.uniform(100, canvas, (n_objects, 2))
    cls = rng.integers(0, nc, n_objects)
    for k in range(1, n_objects, 3):                               # the neighbour: same class and size, shifted along x
        size[k], cls[k] = size[k - 1], cls[k - 1]
        centre[k] = centre[k - 1] + (size[k - 1][0] * rng.uniform(0.27, 0.36), 0.0)
    base = rng.uniform(0.3, 0.95, n_objects)
    views = []
    for _ in range(n_models):
        rows = []
        for k in range(n_objects):
            if rng.uniform() < 0.1:
                continue                                           # missed
            for rep in range(2 if rng.uniform() < twice else 1):    # reported twice: a weaker, looser second box
                c = centre[k] + rng.normal(0, 0.02 + 0.02 * rep, 2) * size[k]
                wh = size[k] * rng.uniform(0.94, 1.06, 2)
                s = np.clip(base[k] + rng.uniform(-0.08, 0.08) - 0.15 * rep, 0.05, 0.99)
                rows.append([*(c - wh / 2), *(c + wh / 2), s, cls[k]])
        n_fp = max(n_objects // 10, (lo or 0) - len(rows))
        for _ in range(n_fp):                                      # false positives
            c, wh = rng.uniform(100, canvas, 2), rng.uniform(20, 120, 2)
            rows.append([*(c - wh / 2), *(c + wh / 2), rng.uniform(0.05, 0.4), rng.integers(0, nc)])
        rows = _f32(rows).reshape(-1, 6)
        rows = rows[np.argsort(-rows[:, 4], kind="stable")][:max_rows]       # best first, as an NMS leaves them
        views.append(rows)
    return views


def random_case(name) -> FuseCase:
    """'three': three images - 3 views; 2 views without a row; 1 view with one row.  'two': 4 views and 2 views.
    'big': one image, 8 views of 250..300 rows (260 objects)."""
    max_rows = 300
    rng = np.random.default_rng({"three": 51, "two": 52, "big": 53}[name])
    if name == "three":
        groups = [_ensemble_views(rng, 3, 40, 1500.0, max_rows), [np.zeros((0, 6))] * 2, [[[5, 6, 50, 60, 0.7, 1]]]]
    elif name == "two":
        groups = [_ensemble_views(rng, 4, 60, 2000.0, max_rows), _ensemble_views(rng, 2, 30, 1200.0, max_rows)]
    else:
        groups = [_ensemble_views(rng, 8, 260, 5000.0, max_rows, lo=250, twice=0.12)]
    views, start = [], [0]
    for g in groups:
        views += list(g)
        start.append(len(views))
    rows, counts = pack_views(views, max_rows)
    return FuseCase(rows, counts, np.asarray(start, np.int32), max_rows)


RANDOM_CASES = ("three", "two", "big")


def random_facts(case: FuseCase):
    """per option: the per-image info dicts of fuse_ref"""
    facts = {}
    for weights, agnostic, max_det in OPTIONS:
        info = []
        fuse_ref(case.rows, case.counts, case.view_start, case_weights(case, weights), THR, agnostic, max_det, info=info)
        facts[(weights, agnostic, max_det)] = info
    return facts


def hand_cases():
    """name -> (views: list of [n, 6] row lists for ONE image, options dict (weights, thr, agnostic, max_det), expected rows from
    the closed form in fp64)"""
    A, B = [0, 0, 100, 100], [10, 0, 110, 100]
    out = {}
    # two models, IoU 90 / 110: x = (0.9 * 0 + 0.6 * 10) / 1.5, score = (1.5 / 2) * (2 / 2)
    out["pair"] = ([[A + [0.9, 0]], [B + [0.6, 0]]], {}, [[4, 0, 104, 100, 0.75, 0]])
    # one of two models: the box stays, the score is halved
    L = [3.3, 7.7, 91.1, 55.5]
    out["lonely"] = ([[L + [0.9, 2]], []], {}, [L + [0.45, 2]])
    # a lonely 0.9 (0.45) opened first, a pair of 0.6s (0.6) ranked first
    C = [500, 0, 600, 100]
    out["outranked"] = ([[A + [0.9, 0], C + [0.6, 0]], [C + [0.6, 0]]], {}, [C + [0.6, 0], A + [0.45, 0]])
    # three members from two models: x = (0 + 0.6 * 10 + 0.5 * 10) / 2, score = (2 / 3) * (min(3, 2) / 2)
    out["overflow"] = ([[A + [0.9, 0], B + [0.5, 0]], [B + [0.6, 0]]], {}, [[5.5, 0, 105.5, 100, 2 / 3, 0]])
    # weights [2, 1]: t = 1.8 and 0.6, x = 6 / 2.4, score = (2.4 / 2) * (min(2, 3) / 3)
    out["weights"] = ([[A + [0.9, 0]], [B + [0.6, 0]]], dict(weights=[2, 1]), [[2.5, 0, 102.5, 100, 0.8, 0]])
    # the weight reverses the order: t = 0.5 and 0.8, the agnostic cluster keeps the class of B, now first
    out["weights_reverse"] = ([[A + [0.5, 0]], [B + [0.4, 1]]], dict(weights=[1, 2], agnostic=True),
                              [[8 / 1.3, 0, 100 + 8 / 1.3, 100, (1.3 / 2) * (2 / 3), 1]])
    out["weights_reverse_unit"] = ([[A + [0.5, 0]], [B + [0.4, 1]]], dict(agnostic=True),
                                   [[4 / 0.9, 0, 100 + 4 / 0.9, 100, 0.45, 0]])
    # the fused box moves away: D has IoU 0.6 with A, 0.49 with fused(A, E) = [16 / 1.7, .., 100 + 16 / 1.7, ..]
    E, D = [20, 0, 120, 100], [-25, 0, 75, 100]
    out["drift"] = ([[A + [0.9, 0], D + [0.3, 0]], [E + [0.8, 0]]], {}, [[16 / 1.7, 0, 100 + 16 / 1.7, 100, 0.85, 0], D + [0.15, 0]])
    # P and Q (IoU 70 / 130) are two clusters; R has IoU 78 / 122 with P and 92 / 108 with Q: the later one
    P, Q, R = [0, 0, 100, 100], [30, 0, 130, 100], [22, 0, 122, 100]
    x = (0.8 * 30 + 0.5 * 22) / 1.3
    out["best_not_first"] = ([[P + [0.9, 0], Q + [0.8, 0]], [R + [0.5, 0]]], {}, [[x, 0, x + 100, 100, 0.65, 0], P + [0.45, 0]])
    # equal t: the earlier view, then the earlier rank, opens the cluster (agnostic: its class shows who did)
    A1, A2 = [1, 0, 101, 100], [2, 0, 102, 100]
    out["tie_t"] = ([[A + [0.7, 0], A1 + [0.7, 1]], [A2 + [0.7, 2]]], dict(agnostic=True), [[1, 0, 101, 100, 0.7, 0]])
    out["tie_t_other_order"] = ([[A2 + [0.7, 2]], [A1 + [0.7, 1], A + [0.7, 0]]], dict(agnostic=True), [[1, 0, 101, 100, 0.7, 2]])
    # equal IoU (40 / 160 with both): the cluster created first
    Q2, R2 = [120, 0, 220, 100], [60, 0, 160, 100]
    out["tie_iou"] = ([[P + [0.9, 0], Q2 + [0.8, 0]], [R2 + [0.5, 0]]], dict(thr=0.2),
                      [[30 / 1.4, 0, 100 + 30 / 1.4, 100, 0.7, 0], Q2 + [0.4, 0]])
    # equal final scores (0.9 / 2 and (0.45 + 0.45) / 2): the cluster created first
    out["tie_score"] = ([[A + [0.9, 0], C + [0.45, 0]], [C + [0.45, 0]]], {}, [A + [0.45, 0], C + [0.45, 0]])
    # IoU exactly 0.5 at thr 0.5: no join
    H = [0, 0, 50, 100]
    out["at_thr"] = ([[A + [0.9, 0]], [H + [0.8, 0]]], dict(thr=0.5), [A + [0.45, 0], H + [0.4, 0]])
    # the same box under two classes
    v = [[A + [0.9, 0]], [A + [0.8, 1]]]
    out["class_aware"] = (v, {}, [A + [0.45, 0], A + [0.4, 1]])
    out["class_agnostic"] = (v, dict(agnostic=True), [A + [0.85, 0]])
    # a zero-area box and its copy never match
    Z = [10, 10, 10, 50]
    out["zero_area"] = ([[Z + [0.95, 0], A + [0.9, 0]], [Z + [0.5, 0]]], {}, [Z + [0.475, 0], A + [0.45, 0], Z + [0.25, 0]])
    # score 0, a negative score and NaN are no candidates: what is left is `pair`
    out["dropped"] = ([[A + [0.9, 0], B + [0.0, 0], B + [-0.5, 0], B + [np.nan, 0]], [B + [0.6, 0], A + [-0.0, 0]]], {},
                      [[4, 0, 104, 100, 0.75, 0]])
    # 904 + 1 * 4096 = 5000: a class offset would lay the class-1 box over the class-0 ones
    x = (0.9 * 5000 + 0.7 * 5004) / 1.6
    out["beyond_4096"] = ([[[5000, 0, 5100, 100, 0.9, 0], [904, 0, 1004, 100, 0.8, 1]], [[5004, 0, 5104, 100, 0.7, 0]]], {},
                          [[x, 0, x + 100, 100, 0.8, 0], [904, 0, 1004, 100, 0.4, 1]])
    # ten disjoint boxes, the even ones found by both models: final score = score (even) or score / 2 (odd); max_det 3
    boxes = [[200 * k, 0, 200 * k + 100, 100, 0.9 - 0.05 * ((k * 3) % 10), 0] for k in range(10)]
    final = [b[:4] + [b[4] if k % 2 == 0 else b[4] / 2, 0] for k, b in enumerate(boxes)]
    out["max_det"] = ([boxes, boxes[::2]], dict(max_det=3), sorted(final, key=lambda r: -r[4])[:3])
    return out


def hand_case(name):
    """-> (FuseCase, dict(weights, thr, agnostic, max_det), expected float64 [n, 6])"""
    views, opt, want = hand_cases()[name]
    rows, counts = pack_views(views, 12)
    opt = dict(dict(weights=None, thr=THR, agnostic=False, max_det=300), **opt)
    return FuseCase(rows, counts, np.asarray([0, len(views)], np.int32), 12), opt, np.asarray(want, np.float64).reshape(-1, 6)
