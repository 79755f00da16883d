"""Plain references of tiled inference - the tile plan, the tile cut (fp32 and bf16 pixel pairs) and the cross-view merge - and
the constructed inputs that tests/test_tiles_reference.py (CPU) and tests/test_hip_tiles.py (GPU) run.

Nothing here touches the HIP library.  Written from the definitions, not from the kernels:

* `plan_ref`      origins along an axis from the closed form (ceil((n - S) / step) + 1 of them, the last one n - S), tiles
                  row-major, then the letterboxed whole image unless it would be the same pixels.
* `tile_ref`      slot = the S x S window at (x0, y0): fp32(u8) / fp32(255) inside the image, fp32(114) / fp32(255) outside.
                  `pairs_ref` rounds to bf16 (nearest, ties to even) into [S, S, 4] with a zero fourth channel.
* `merge_ref`     the greedy pass as a plain loop over the sorted candidates, keeper by keeper, fp32 with every operation
                  rounded on its own: a candidate not yet absorbed is kept and absorbs every later candidate, not yet
                  absorbed, of its class (any class when agnostic) whose metric against its ORIGINAL box exceeds thr.

Every case builder returns its inputs together with facts computed from the reference alone; the CPU test asserts them,
which keeps a GPU test from passing on an input that no longer reaches what it was built for.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

PAD = 114


def _f32(x):
    return np.asarray(x, dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------ plan
class ViewRef(NamedTuple):
    full: bool
    x0: int
    y0: int
    letterbox: np.ndarray       # float32 [6]


def origins_ref(n, S, o):
    step = S - o
    if n <= S:
        return [0]
    count = math.ceil((n - S) / step) + 1
    return [k * step for k in range(count - 1)] + [n - S]


def plan_ref(h, w, S, overlap=0.2, full_view=True, letterbox_row=None):
    """-> list of ViewRef.  `letterbox_row(h, w, S)` gives the full view's row (the GPU tests pass the product's
    letterbox_table; without it the full view carries NaNs)."""
    o = int(S * overlap)
    views = [ViewRef(False, x0, y0, _f32([-x0, -y0, 1, 1, w, h])) for y0 in origins_ref(h, S, o) for x0 in origins_ref(w, S, o)]
    if full_view and not (len(views) == 1 and max(h, w) == S):
        row = letterbox_row(h, w, S) if letterbox_row else np.full(6, np.nan)
        views.append(ViewRef(True, 0, 0, _f32(row)))
    return views


# -------------------------------------------------------------------------------------------------------- tile cut
def tile_ref(img, x0, y0, S):
    """img u8 [h, w, 3] -> fp32 [3, S, S]"""
    h, w = img.shape[:2]
    win = np.full((S, S, 3), PAD, np.uint8)
    ys, xs = slice(max(y0, 0), min(y0 + S, h)), slice(max(x0, 0), min(x0 + S, w))
    win[ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0] = img[ys, xs]
    return np.ascontiguousarray((win.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def bf16_bits(x):
    """fp32 -> bf16 bit patterns (uint16), round to nearest, ties to even (finite inputs)"""
    u = _f32(x).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def pairs_ref(f32):
    """fp32 [T, 3, S, S] -> int16 [T, S, S, 4]: the network's input layout ([T][S][S/2][8] seen pixel by pixel)"""
    T, _, S, _ = f32.shape
    out = np.zeros((T, S, S, 4), np.uint16)
    out[..., :3] = bf16_bits(f32).transpose(0, 2, 3, 1)
    return out.view(np.int16)


# ----------------------------------------------------------------------------------------------------------- merge
def merge_ref(rows, counts, view_start, thr, metric="ios", mode="nmm", agnostic=False, max_det=300, info=None):
    """rows [V, max_rows, 6] fp32, counts [V], view_start [n_images + 1] -> list of [n <= max_det, 6] fp32.  `info` (a list)
    receives per image dict(candidates, absorbed, kept, grown: keepers whose hull differs from their own box)."""
    rows, thr = _f32(rows), np.float32(thr)
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(len(view_start) - 1):
            views = range(int(view_start[i]), int(view_start[i + 1]))
            cand = np.concatenate([rows[v, :max(0, min(int(counts[v]), rows.shape[1]))] for v in views] + [np.zeros((0, 6), np.float32)])
            n = len(cand)
            hi = np.uint64(0xFFFFFFFF) - cand[:, 4].copy().view(np.uint32).astype(np.uint64)
            key = (hi << np.uint64(32)) | np.arange(n, dtype=np.uint64)               # score descending, then the index
            c = cand[np.argsort(key, kind="stable")]
            area = (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1])
            absorbed = np.zeros(n, bool)
            kept, n_abs, grown = [], 0, 0
            for j in range(n):
                if absorbed[j]:
                    continue
                if len(kept) == max_det:
                    break
                later = np.nonzero(~absorbed[j + 1:] & (agnostic | (c[j + 1:, 5] == c[j, 5])))[0] + j + 1
                b = c[later]
                w = np.maximum(np.float32(0), np.minimum(c[j, 2], b[:, 2]) - np.maximum(c[j, 0], b[:, 0]))
                h = np.maximum(np.float32(0), np.minimum(c[j, 3], b[:, 3]) - np.maximum(c[j, 1], b[:, 1]))
                inter = w * h
                m = inter / np.minimum(area[j], area[later]) if metric == "ios" else inter / (area[j] + area[later] - inter)
                hit = later[m > thr]                                                  # NaN never matches
                absorbed[hit] = True
                n_abs += len(hit)
                row = c[j].copy()
                if mode == "nmm" and len(hit):
                    row[:2] = np.minimum(row[:2], c[hit, :2].min(0))
                    row[2:4] = np.maximum(row[2:4], c[hit, 2:4].max(0))
                    grown += int((row[:4] != c[j, :4]).any())
                kept.append(row)
            out.append(np.asarray(kept, np.float32).reshape(-1, 6))
            if info is not None:
                info.append(dict(candidates=n, absorbed=n_abs, kept=len(kept), grown=grown))
    return out


def pack_views(views, max_rows, fill=np.nan):
    """list of [n_v, 6] arrays -> (rows [V, max_rows, 6] with `fill` beyond each count, counts int32 [V])"""
    rows = np.full((len(views), max_rows, 6), fill, np.float32)
    counts = np.zeros(len(views), np.int32)
    for v, r in enumerate(views):
        r = _f32(r).reshape(-1, 6)
        rows[v, :len(r)], counts[v] = r, len(r)
    return rows, counts


class MergeCase(NamedTuple):
    rows: np.ndarray
    counts: np.ndarray
    view_start: np.ndarray
    max_rows: int


OPTIONS = [(metric, mode, agnostic, max_det) for metric in ("iou", "ios") for mode in ("nms", "nmm") for agnostic in (False, True)
           for max_det in (300, 7)]
THR = 0.5


def _cluster_rows(rng, n, n_clusters, canvas, nc=3, tie_every=0):
    """n rows drawn around n_clusters centres: whole objects, halves of them (what a tile border leaves) and shifted copies;
    distinct scores unless tie_every (then every tie_every-th row repeats its predecessor's score)"""
    centre = rng.uniform(100, canvas, (n_clusters, 2))
    size = rng.uniform(30, 160, (n_clusters, 2))
    cls = rng.integers(0, nc, n_clusters)
    k = rng.integers(0, n_clusters, n)
    c = centre[k] + rng.normal(0, 4, (n, 2))
    wh = size[k] * rng.uniform(0.9, 1.1, (n, 2))
    x1y1, x2y2 = c - wh / 2, c + wh / 2
    half = rng.uniform(0, 1, n)
    cut = (x1y1[:, 0] + x2y2[:, 0]) / 2
    x2y2[:, 0] = np.where(half < 0.25, cut, x2y2[:, 0])            # the left half
    x1y1[:, 0] = np.where(half > 0.8, cut, x1y1[:, 0])             # the right half
    score = rng.permutation(n).astype(np.float64) / (n + 1) * 0.7 + 0.25
    if tie_every:
        score[tie_every::tie_every] = score[tie_every - 1:-1:tie_every]
    label = np.where(rng.uniform(0, 1, n) < 0.85, cls[k], rng.integers(0, nc, n))
    return _f32(np.concatenate((x1y1, x2y2, score[:, None], label[:, None]), 1))


def random_case(name) -> MergeCase:
    """'three': three images - four views with counts 120, 0, 300, 57; two views without a row; one view with one row.
    'two': two images of three and two views.  'big': one image, 17 views x 300 rows = 5100 candidates (two 4096-key chunks)."""
    max_rows = 300
    layout = {"three": (41, [[120, 0, 300, 57], [0, 0], [1]]), "two": (42, [[300, 211, 64], [65, 300]]), "big": (43, [[300] * 17])}
    seed, images = layout[name]
    rng = np.random.default_rng(seed)
    views, start = [], [0]
    for counts in images:
        total = sum(counts)
        rows = _cluster_rows(rng, total, max(1, total // 12), 6000.0, tie_every=9 if total > 20 else 0)
        rows = rows[rng.permutation(total)]
        at = np.cumsum([0] + counts)
        views += [rows[a:b] for a, b in zip(at[:-1], at[1:])]
        start.append(len(views))
    rows, counts = pack_views(views, max_rows)
    return MergeCase(rows, counts, np.asarray(start, np.int32), max_rows)


RANDOM_CASES = ("three", "two", "big")


def random_facts(case: MergeCase):
    """per option: (total candidates, absorbed, kept, keepers whose hull grew), summed over the images"""
    facts = {}
    for metric, mode, agnostic, max_det in OPTIONS:
        info = []
        merge_ref(case.rows, case.counts, case.view_start, THR, metric, mode, agnostic, max_det, info=info)
        facts[(metric, mode, agnostic, max_det)] = tuple(sum(i[k] for i in info) for k in ("candidates", "absorbed", "kept", "grown"))
    return facts


def hand_cases():
    """name -> (views: list of [n, 6] row lists for ONE image, options dict, expected rows)"""
    A, Bc = [0, 0, 100, 100], [0, 0, 50, 50]
    out = {}
    # a contained box: IoU 0.25, IoS 1
    v = [[A + [0.9, 0], Bc + [0.8, 0]]]
    out["contained_iou"] = (v, dict(metric="iou", mode="nms"), [A + [0.9, 0], Bc + [0.8, 0]])
    out["contained_ios"] = (v, dict(metric="ios", mode="nms"), [A + [0.9, 0]])
    out["contained_ios_nmm"] = (v, dict(metric="ios", mode="nmm"), [A + [0.9, 0]])
    # A absorbs B (IoS 0.6); C overlaps hull(A, B) = [0, 0, 140, 100] but not A: kept
    Bh, C = [40, 0, 140, 100], [110, 0, 210, 100]
    v = [[A + [0.9, 1]], [Bh + [0.8, 1], C + [0.7, 1]]]
    out["hull_nmm"] = (v, dict(metric="ios", mode="nmm"), [[0, 0, 140, 100, 0.9, 1], C + [0.7, 1]])
    out["hull_nms"] = (v, dict(metric="ios", mode="nms"), [A + [0.9, 1], C + [0.7, 1]])
    # the same box under two classes
    v = [[A + [0.9, 0]], [A + [0.8, 1]]]
    out["class_aware"] = (v, dict(metric="iou", mode="nms"), [A + [0.9, 0], A + [0.8, 1]])
    out["class_agnostic"] = (v, dict(metric="iou", mode="nms", agnostic=True), [A + [0.9, 0]])
    # 904 + 1 * 4096 = 5000: the class-offset trick would lay the second box over the first
    v = [[[5000, 0, 5100, 100, 0.9, 0], [904, 0, 1004, 100, 0.8, 1]]]
    out["beyond_4096"] = (v, dict(metric="iou", mode="nms"), [[5000, 0, 5100, 100, 0.9, 0], [904, 0, 1004, 100, 0.8, 1]])
    # a zero-area box (and its copy) match nothing: inter 0, IoS 0 / 0, IoU of the copies 0 / 0
    Z = [10, 10, 10, 50]
    v = [[Z + [0.95, 0], A + [0.9, 0], Z + [0.5, 0]]]
    for metric in ("iou", "ios"):
        out[f"zero_area_{metric}"] = (v, dict(metric=metric, mode="nmm"), [Z + [0.95, 0], A + [0.9, 0], Z + [0.5, 0]])
    # equal scores: the candidate of the earlier view is the keeper, within a view the earlier rank
    D = [2, 0, 102, 100]
    v = [[[500, 500, 600, 600, 0.4, 0]], [D + [0.75, 0], A + [0.75, 0]], [[1, 0, 101, 100, 0.75, 0]]]
    out["ties"] = (v, dict(metric="iou", mode="nms"), [D + [0.75, 0], [500, 500, 600, 600, 0.4, 0]])
    v = [[[1, 0, 101, 100, 0.75, 0]], [D + [0.75, 0], A + [0.75, 0]]]
    out["ties_other_order"] = (v, dict(metric="iou", mode="nms"), [[1, 0, 101, 100, 0.75, 0]])
    # ten disjoint boxes, max_det 3
    v = [[[200 * k, 0, 200 * k + 100, 100, 0.9 - 0.05 * ((k * 3) % 10), 0] for k in range(10)]]
    best = sorted(v[0], key=lambda r: -r[4])[:3]
    out["max_det"] = (v, dict(metric="ios", mode="nmm", max_det=3), best)
    return out


def hand_case(name):
    views, opt, want = hand_cases()[name]
    rows, counts = pack_views(views, 12)
    return MergeCase(rows, counts, np.asarray([0, len(views)], np.int32), 12), opt, _f32(want).reshape(-1, 6)


# --------------------------------------------------------------------------------------------------------- images
def noise_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
