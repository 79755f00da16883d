"""Auto-anchor: fit anchor boxes to a dataset's labels on the device - YOLOv5's `check_anchors` / `kmean_anchors`
(utils/autoanchor.py), with the metric, the k-means steps and the genetic search in csrc/anchors.hip.

    wh = label_wh(boxes, shapes, 640)                     # what DeviceTrainPipeline is constructed with
    m = anchor_metrics(wh, anchor_info)                   # bpr, aat, fitness, n
    anchor_info, report = check_anchors(wh, anchor_info)  # refit when fewer than 98 % of the boxes can be assigned
    s8, s16, s32 = anchor_info_yaml(anchor_info)          # the three Hydra files

With the assigner's ratio threshold of 4 a box whose sides are more than 4 x away from every anchor is never assigned
and never learned; `bpr` (best possible recall) is the share of boxes that can be.  Anchors stay a constructor argument
of the assigner, the loss and the detectors: nothing here touches them.

The box sizes go to the device once; every kernel runs on the current torch stream; one `_host.fetch` at the end brings
back the result.  There is no host fallback: without a GPU these functions raise (`_lib.require_gpu`)."""
from __future__ import annotations

import warnings
from typing import NamedTuple, Sequence

import numpy as np

from ... import _lib
from ..types import FeatureShape
from .info import AnchorBoxInfo

MUTATION_PROB = 0.9        # YOLOv5 kmean_anchors: mp
MUTATION_SIGMA = 0.1       # ... s
MUTATION_CLIP = (0.3, 3.0)
MIN_ANCHOR_PX = 2.0


class AnchorMetrics(NamedTuple):
    bpr: float           # best possible recall: boxes with at least one anchor inside the ratio threshold / n
    aat: float           # anchors above threshold per box
    fitness: float       # mean over the boxes of (best ratio if above the threshold, else 0): what the evolution climbs
    n: int               # boxes measured


class AnchorReport(NamedTuple):
    before: AnchorMetrics
    after: AnchorMetrics
    replaced: bool


# ---- host helpers (no GPU) ------------------------------------------------------------------------------------------

def label_wh(boxes: Sequence[np.ndarray], shapes: Sequence, image_size: int) -> np.ndarray:
    """boxes: one [m, 4] xyxy pixel array per image, shapes: the (h, w) of each image -> float32 [N, 2] widths and heights
    at training resolution: scaled by image_size / max(h, w) (YOLOv5's `shapes / shapes.max(1)` normalisation)."""
    if len(boxes) != len(shapes):
        raise ValueError(f"label_wh: {len(boxes)} box arrays for {len(shapes)} image shapes")
    out = []
    for bb, (h, w) in zip(boxes, shapes):
        bb = np.asarray(bb, dtype=np.float64).reshape(-1, 4)
        out.append((bb[:, 2:4] - bb[:, 0:2]) * (float(image_size) / max(h, w)))
    return (np.concatenate(out) if out else np.zeros((0, 2))).astype(np.float32).reshape(-1, 2)


def dataset_label_wh(dataset_info, image_size: int) -> np.ndarray:
    """label_wh of a data.cache.DatasetInfo: image_metadata (width, height) and targets[*].bounding_box (x1, y1, x2, y2)."""
    boxes, shapes = [], []
    for s in dataset_info.samples:
        bb = [tuple(float(v) for v in tuple(t.bounding_box)[:4]) for t in (s.targets or ())]
        boxes.append(np.asarray(bb, dtype=np.float64).reshape(-1, 4))
        shapes.append((s.image_metadata.height, s.image_metadata.width))
    return label_wh(boxes, shapes, image_size)


def anchors_array(anchor_info) -> np.ndarray:
    """LayerwiseAnchorInfo (or any sequence of AnchorBoxInfo) or an [n, 2] array -> float32 [n, 2] (width, height), levels in order."""
    if isinstance(anchor_info, (tuple, list)) and len(anchor_info) and hasattr(anchor_info[0], "boxes_wh"):
        return np.asarray([[float(b.width), float(b.height)] for lv in anchor_info for b in lv.boxes_wh], dtype=np.float32)
    a = np.asarray(anchor_info, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != 2 or a.shape[0] < 1:
        raise ValueError(f"anchors must be a LayerwiseAnchorInfo or an [n, 2] array, got shape {a.shape}")
    return np.ascontiguousarray(a)


def split_levels(anchors: np.ndarray, strides: Sequence[int]):
    """[3 * levels, 2] anchors -> LayerwiseAnchorInfo for three levels (a tuple of AnchorBoxInfo otherwise): sorted by
    area, three each, smallest to the first stride.  Values are plain Python floats."""
    a = np.asarray(anchors, dtype=np.float32).reshape(-1, 2)
    if a.shape[0] != 3 * len(strides):
        raise ValueError(f"{a.shape[0]} anchors for {len(strides)} levels: need 3 per level")
    a = a[np.argsort(a.prod(1), kind="stable")]
    levels = [AnchorBoxInfo(stride=int(s), boxes_wh=[FeatureShape(width=float(w), height=float(h)) for w, h in a[3 * i:3 * i + 3]])
              for i, s in enumerate(strides)]
    if len(levels) == 3:
        from ...lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo
        return LayerwiseAnchorInfo(*levels)
    return tuple(levels)


def anchor_info_yaml(info) -> list:
    """One Hydra config text per level, in the layout of the reference's configs/anchor_boxes/voc_s{8,16,32}.yaml."""
    texts = []
    for lv in info:
        lines = ["_target_: kod.core.anchors.info.AnchorBoxInfo", f"stride: {int(lv.stride)}", "boxes_wh:"]
        for b in lv.boxes_wh:
            lines += ["  - _target_: kod.core.types.FeatureShape", f"    width: {_yaml_number(b.width)}",
                      f"    height: {_yaml_number(b.height)}"]
        texts.append("\n".join(lines) + "\n")
    return texts


def _yaml_number(v) -> str:
    f = float(v)
    return str(int(f)) if f == int(f) else repr(round(f, 2))


def mutation_table(rng: np.random.Generator, gen: int, population: int, n: int) -> np.ndarray:
    """float32 [gen, population, n, 2] mutation factors.  Draw order, per generation and then per candidate: a mask
    `rng.random((n, 2)) < 0.9`, one scalar `rng.random()`, `rng.standard_normal((n, 2))`; factor = clip(mask * scalar *
    normal * 0.1 + 1, 0.3, 3.0) in fp64, rounded to fp32; a candidate whose factors are all 1 is drawn again."""
    v = np.ones((gen, population, n, 2), dtype=np.float32)
    for g in range(gen):
        for p in range(population):
            while (v[g, p] == 1).all():
                mask = rng.random((n, 2)) < MUTATION_PROB
                u = rng.random()
                z = rng.standard_normal((n, 2))
                v[g, p] = (mask * u * z * MUTATION_SIGMA + 1.0).clip(*MUTATION_CLIP).astype(np.float32)
    return v


def filter_wh(wh: np.ndarray) -> np.ndarray:
    """kmean_anchors' filter: a box is dropped when BOTH sides are under 2 px (one side under 2 px: kept)."""
    wh = np.asarray(wh, dtype=np.float32).reshape(-1, 2)
    return np.ascontiguousarray(wh[(wh >= MIN_ANCHOR_PX).any(1)])


# ---- device ---------------------------------------------------------------------------------------------------------

def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _limits(lib, n=None, population=None, restarts=None):
    if n is not None and not 1 <= n <= lib.kodhip_anchor_max_anchors():
        raise ValueError(f"n = {n} anchors: the device kernels hold 1..{lib.kodhip_anchor_max_anchors()} (csrc/anchors.hip)")
    if population is not None and not 1 <= population <= lib.kodhip_anchor_max_population():
        raise ValueError(f"population = {population}: the device kernels hold 1..{lib.kodhip_anchor_max_population()}")
    if restarts is not None and not 1 <= restarts <= lib.kodhip_anchor_max_restarts():
        raise ValueError(f"restarts = {restarts}: the device kernels hold 1..{lib.kodhip_anchor_max_restarts()}")


def _workspace(lib, N, sets):
    import torch
    return torch.empty(lib.kodhip_anchor_workspace_bytes(N, sets), dtype=torch.uint8, device="cuda")


def _device_wh(wh):
    import torch
    wh = np.ascontiguousarray(np.asarray(wh, dtype=np.float32).reshape(-1, 2))
    if wh.shape[0] < 1:
        raise ValueError("no boxes")
    return torch.from_numpy(wh).cuda()


def _metric_launch(lib, d_wh, d_k, P, n, t, ws):
    """-> device (fitness_sum f64 [P], n_recalled i64 [P], n_pairs i64 [P]); launches only"""
    import torch
    fit = torch.empty(P, dtype=torch.float64, device="cuda")
    rec = torch.empty(P, dtype=torch.int64, device="cuda")
    pairs = torch.empty(P, dtype=torch.int64, device="cuda")
    _lib.check(lib.kodhip_anchor_metric(d_wh.data_ptr(), d_wh.shape[0], d_k.data_ptr(), P, n, t, ws.data_ptr(), fit.data_ptr(),
                                        rec.data_ptr(), pairs.data_ptr(), _stream()), "anchor_metric")
    return fit, rec, pairs


def _threshold(thr: float) -> float:
    return float(np.float32(1.0 / float(thr)))


def anchor_metrics(wh, anchor_info, thr: float = 4.0) -> AnchorMetrics:
    """YOLOv5's anchor metric of `anchor_info` (LayerwiseAnchorInfo or [n, 2] array) over box sizes wh [N, 2] (pixels at
    training resolution; every box given is measured).  A box counts when min(r, 1 / r) over both sides, r = wh / anchor, is
    strictly above float32(1 / thr) for some anchor."""
    import torch
    from ... import _host
    _lib.require_gpu()
    lib = _lib.lib()
    k = anchors_array(anchor_info)
    _limits(lib, n=k.shape[0])
    d_wh = _device_wh(wh)
    N = d_wh.shape[0]
    fit, rec, pairs = _metric_launch(lib, d_wh, torch.from_numpy(k).cuda(), 1, k.shape[0], _threshold(thr), _workspace(lib, N, 1))
    f, r, c = _host.fetch(fit, rec, pairs)
    return AnchorMetrics(bpr=int(r[0]) / N, aat=int(c[0]) / N, fitness=float(f[0]) / N, n=N)


def kmean_anchors(wh, n: int = 9, image_size: int = 640, thr: float = 4.0, gen: int = 1000, population: int = 1,
                  restarts: int = 30, kmeans_iters: int = 30, seed: int = 0) -> np.ndarray:
    """Fit n anchors to box sizes wh [N, 2] -> float32 [n, 2] sorted by area.  YOLOv5's `kmean_anchors`, step by step:

    1. boxes with both sides under 2 px are dropped; a warning counts the boxes with a side under 3 px;
    2. the sizes are whitened by their per-axis standard deviation;
    3. k-means: `restarts` initialisations of n distinct points each, `kmeans_iters` Lloyd steps, all restarts in one
       launch pair per step; the restart of lowest distortion (equal: lower index) is kept;
    4. un-whitened and sorted by area;
    5. when fewer than n distinct centroids survive: YOLOv5's `sort(random(2 n)).reshape(n, 2) * image_size`;
    6. genetic evolution, `gen` generations: mutation probability 0.9, sigma 0.1, factors clipped to [0.3, 3.0], a
       mutation that changes nothing drawn again, anchors clipped at 2 px; a generation's best candidate replaces the
       anchors when its fitness is strictly higher.

    One generator, `numpy.random.default_rng(seed)`, draws in this order: the k-means initialisations (`rng.choice(N, n,
    replace=False)`, restart by restart), the fallback of step 5 if taken, then `mutation_table`.  The table is uploaded
    once; only the final anchors, the final fitness and the trace come back.

    Deviations from YOLOv5 / scipy.cluster.vq.kmeans:
      * deterministic initialisation from `seed` (scipy draws from numpy's global stream), `restarts` of them where
        YOLOv5 asks scipy for 30 iterations of ONE;
      * a fixed number of Lloyd steps where scipy stops at a distortion-change threshold; the distortion compared between
        restarts is that of the last step (to the centroids before its update) and is a sum of squared distances;
      * the sums of the metric, the centroids and the distortion are accumulated in fp64 in a fixed order (per-box values
        are YOLOv5's fp32 arithmetic): results repeat bit for bit;
      * `population > 1` evaluates that many mutants per generation and keeps the best; `population = 1` is YOLOv5's
        schedule (with this module's random stream, not YOLOv5's)."""
    import torch
    from ... import _host
    _lib.require_gpu()
    lib = _lib.lib()
    _limits(lib, n=n, population=population, restarts=restarts)
    if gen < 0 or kmeans_iters < 1:
        raise ValueError("gen must be >= 0 and kmeans_iters >= 1")
    wh0 = np.asarray(wh, dtype=np.float32).reshape(-1, 2)
    small = int((wh0 < 3.0).any(1).sum())
    if small:
        warnings.warn(f"kmean_anchors: {small} of {len(wh0)} boxes have a side under 3 px")
    whf = filter_wh(wh0)
    N = whf.shape[0]
    if N < n:
        raise ValueError(f"kmean_anchors: {N} boxes of at least 2 px for {n} anchors")
    rng = np.random.default_rng(seed)
    t = _threshold(thr)

    std = whf.astype(np.float64).std(0).astype(np.float32)
    if not (std > 0).all():
        raise ValueError("kmean_anchors: all boxes share a width or a height")
    pts = np.ascontiguousarray(whf / std)
    init = np.stack([pts[rng.choice(N, n, replace=False)] for _ in range(restarts)])          # [R, n, 2]

    d_wh, d_pts = torch.from_numpy(whf).cuda(), torch.from_numpy(pts).cuda()
    d_cent = torch.from_numpy(np.ascontiguousarray(init)).cuda()
    ws = _workspace(lib, N, max(restarts, population))
    dist = torch.empty(restarts, dtype=torch.float64, device="cuda")
    counts = torch.empty((restarts, n), dtype=torch.int64, device="cuda")
    for _ in range(kmeans_iters):
        _lib.check(lib.kodhip_anchor_kmeans_step(d_pts.data_ptr(), N, d_cent.data_ptr(), restarts, n, ws.data_ptr(), dist.data_ptr(),
                                                 counts.data_ptr(), None, _stream()), "anchor_kmeans_step")
    h_cent, h_dist = _host.fetch(d_cent, dist)
    best = int(np.argmin(h_dist.numpy()))
    k = h_cent.numpy()[best].copy() * std
    k = k[np.argsort(k.prod(1), kind="stable")]
    if len(np.unique(k, axis=0)) < n:
        warnings.warn(f"kmean_anchors: k-means left fewer than {n} distinct anchors; starting the evolution from a uniform spread")
        k = (np.sort(rng.random(n * 2)).reshape(n, 2) * image_size).astype(np.float32)
    k = np.ascontiguousarray(k, dtype=np.float32)
    if gen == 0:
        return k

    table = mutation_table(rng, gen, population, n)
    d_k = torch.from_numpy(k).cuda()
    d_table = torch.from_numpy(table).cuda()
    fit, _, _ = _metric_launch(lib, d_wh, d_k, 1, n, t, ws)
    trace = torch.empty(gen * lib.kodhip_anchor_trace_bytes(), dtype=torch.uint8, device="cuda")
    _lib.check(lib.kodhip_anchor_evolve(d_wh.data_ptr(), N, d_k.data_ptr(), fit.data_ptr(), d_table.data_ptr(), gen, population, n, t,
                                        trace.data_ptr(), ws.data_ptr(), _stream()), "anchor_evolve")
    h_k, _, _ = _host.fetch(d_k, fit, trace)
    k = h_k.numpy().copy()
    return np.ascontiguousarray(k[np.argsort(k.prod(1), kind="stable")])


def check_anchors(wh, anchor_info, thr: float = 4.0, image_size: int = 640, bpr_ok: float = 0.98, **fit_kwargs):
    """YOLOv5's `check_anchors` rule -> (LayerwiseAnchorInfo, AnchorReport): the given anchors are kept when their best
    possible recall exceeds `bpr_ok`; otherwise new ones are fitted (`kmean_anchors(wh, n, image_size, thr, **fit_kwargs)`)
    and adopted only if their recall is higher.  New anchors are split by area, three per level, onto the given strides.
    (YOLOv5 also jitters the box sizes by 0.9 - 1.1 before measuring; here the boxes are measured as given.)"""
    levels = list(anchor_info)
    n = sum(len(lv.boxes_wh) for lv in levels)
    if any(len(lv.boxes_wh) != 3 for lv in levels) or "n" in fit_kwargs:
        raise ValueError("check_anchors: three anchors per level (n = 3 x the number of levels)")
    before = anchor_metrics(wh, anchor_info, thr)
    if before.bpr > bpr_ok:
        return anchor_info, AnchorReport(before=before, after=before, replaced=False)
    new = kmean_anchors(wh, n=n, image_size=image_size, thr=thr, **fit_kwargs)
    after = anchor_metrics(wh, new, thr)
    if after.bpr > before.bpr:
        return split_levels(new, [lv.stride for lv in levels]), AnchorReport(before=before, after=after, replaced=True)
    return anchor_info, AnchorReport(before=before, after=after, replaced=False)
