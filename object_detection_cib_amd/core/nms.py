"""non_max_suppression - drop-in for kod.core.nms.non_max_suppression (kod/core/nms.py:9-75).

Same signature and result (list of [n<=300, 6] tensors: x1, y1, x2, y2, conf, cls); the boolean-mask /
nonzero / argsort / torchvision.ops.nms chain of the reference is three HIP kernels per batch
(csrc/postproc.hip), so validation stays on the device.

The keyword-only arguments are the options of YOLOv5's detect.py (kodhip_nms_ex): `agnostic`, `multi_label`, `max_det` and
`letterbox`, which maps the kept boxes back into each image's own pixels.  With all of them at their defaults the call is
the validation one, unchanged.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .. import _host, _lib


_WORKSPACE = {}


class PackedDetections(list):
    """What non_max_suppression returns: the list of per-image [n, 6] tensors of the reference, which are views of ONE
    device buffer.  A consumer that runs on the device (DeviceConfusionMatrix) takes the buffer and the device-side counts
    as they are instead of re-packing the list: `packed` [B, max_det, 6] fp32 (rows beyond an image's count are
    uninitialised), `counts` [B] int32 on the device.  They describe the list as it was returned."""

    def __init__(self, items, packed: torch.Tensor, counts: torch.Tensor):
        super().__init__(items)
        self.packed, self.counts = packed, counts


def _workspace(dev, n: int) -> torch.Tensor:
    # the sort keys are the one large workspace (B * key_cap * 8 B = 134 MB at 64 x 25200 x 10): kept across calls,
    # returning it to the caching allocator every batch makes later allocations fall through to hipMalloc (tens of ms)
    # (grow-only per device: alternating full and partial validation batches reuse the largest buffer)
    keys = _WORKSPACE.get(dev)
    if keys is None or keys.numel() < n:
        keys = _WORKSPACE[dev] = torch.empty(n, dtype=torch.int64, device=dev)
    return keys


def _key_cap(need: int) -> int:
    key_cap = 64
    while key_cap < need:
        key_cap <<= 1
    return key_cap


def non_max_suppression(detections: torch.Tensor, conf_thres: float = 0.25, nms_thres: float = 0.45,
                        classes=None, *, agnostic: bool = False, multi_label: Optional[bool] = None, max_det: int = 300,
                        letterbox=None) -> Sequence[torch.Tensor]:
    """detections [B, rows, 5 + nc].  classes: keep these class ids only.  agnostic: boxes of different classes suppress
    each other.  multi_label: None = the reference's rule (nc > 1: every class over conf_thres is a candidate); False = one
    candidate per row, its best class (detect.py; the key workspace then holds `rows` keys per image, not `rows * nc`).
    max_det: 1..300 rows per image.  letterbox: float32 [B, 6] (left, top, scale_x, scale_y, width, height per image,
    KodLetterbox): the kept boxes become min(max((x - left) * scale_x, 0), width) and likewise for y."""
    _lib.require_gpu()
    if not 1 <= int(max_det) <= 300:
        raise ValueError(f"max_det {max_det}: expected 1..300 (the greedy pass keeps its survivors in LDS)")
    det = detections.contiguous().float()
    B, rows, P = det.shape
    nc = P - 5
    dev = det.device
    max_wh, max_nms = 4096.0, 30000                                # nms.py:22-26
    multi = nc > 1 if multi_label is None else bool(multi_label)
    extended = agnostic or multi_label is not None or int(max_det) != 300 or letterbox is not None
    keep = None
    if classes is not None:
        keep = torch.zeros(nc, dtype=torch.bool, device=dev)
        keep[torch.as_tensor(list(classes), dtype=torch.long, device=dev)] = True
        if not extended:
            # nms.py:52-54 drops candidates whose class is not listed, before the top-30000 cut: a zeroed class
            # probability never passes `cls * obj > conf_thres`, so masking the columns is the same filter
            det = det.clone()
            det[..., 5:] *= keep.to(det.dtype)
    max_det = int(max_det)
    key_cap = _key_cap(rows * nc if (multi or not extended) else rows)
    keys = _workspace(dev, B * key_cap)
    ncand = torch.empty(B, dtype=torch.int32, device=dev)
    out = torch.empty((B, max_det, 6), dtype=torch.float32, device=dev)
    nout = torch.empty(B, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    if not extended:
        _lib.check(_lib.lib().kodhip_nms(det.data_ptr(), keys.data_ptr(), key_cap, ncand.data_ptr(), out.data_ptr(),
                                         nout.data_ptr(), B, rows, nc, float(conf_thres), float(nms_thres), max_det,
                                         max_nms, max_wh, stream), "nms")
    else:
        lb = None
        if letterbox is not None:
            lb = letterbox if torch.is_tensor(letterbox) else torch.from_numpy(np.ascontiguousarray(letterbox, dtype=np.float32))
            lb = lb.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(lb.shape) != (B, 6):
                raise ValueError(f"letterbox shape {tuple(lb.shape)}: expected ({B}, 6)")
        mask = keep.to(torch.uint8) if keep is not None else None
        _lib.check(_lib.lib().kodhip_nms_ex(det.data_ptr(), keys.data_ptr(), key_cap, ncand.data_ptr(), out.data_ptr(),
                                            nout.data_ptr(), B, rows, nc, float(conf_thres), float(nms_thres), max_det,
                                            max_nms, 0.0 if agnostic else max_wh, 0 if multi else 1,
                                            mask.data_ptr() if mask is not None else None,
                                            lb.data_ptr() if lb is not None else None, stream), "nms_ex")
    counts = _host.fetch(nout)[0].tolist()                           # one polling hand-off per batch (sizes the outputs)
    return PackedDetections([out[b, :n] for b, n in enumerate(counts)], out, nout)


_MERGE_METRICS = {"iou": 0, "ios": 1}
_MERGE_MODES = {"nms": 0, "nmm": 1}


def merge_detections(rows: torch.Tensor, counts: torch.Tensor, view_start, *, thres: float = 0.5, metric: str = "ios",
                     mode: str = "nmm", agnostic: bool = False, max_det: int = 300) -> PackedDetections:
    """The cross-view merge of tiled inference (kodhip_merge_detections): rows [V, max_rows, 6] and counts [V] are what
    kodhip_nms_ex left for each view, in image pixels; the views of image i are view_start[i] .. view_start[i + 1]
    (`view_start`: a host sequence of n_images + 1 ints).  metric "iou" | "ios" (intersection over the smaller area), mode
    "nms" (an absorbed row is dropped) | "nmm" (the keeper's box grows to the hull of what it absorbs); classes are
    compared directly, `agnostic` lets every class absorb every other.  -> per image [n <= max_det, 6], best score first."""
    _lib.require_gpu()
    if metric not in _MERGE_METRICS:
        raise ValueError(f"metric {metric!r}: expected 'iou' or 'ios'")
    if mode not in _MERGE_MODES:
        raise ValueError(f"mode {mode!r}: expected 'nms' or 'nmm'")
    if not 1 <= int(max_det) <= 300:
        raise ValueError(f"max_det {max_det}: expected 1..300")
    if not 0.0 <= float(thres) <= 1.0:
        raise ValueError(f"thres {thres}: expected a value in [0, 1]")
    start = np.asarray(view_start, dtype=np.int64).reshape(-1)
    V, max_rows = int(rows.shape[0]), int(rows.shape[1])
    n_images = len(start) - 1
    if n_images < 1 or start[0] != 0 or start[-1] > V or (np.diff(start) < 0).any():
        raise ValueError(f"view_start {start.tolist()}: expected 0 = s[0] <= s[1] <= ... <= {V} for at least one image")
    if tuple(rows.shape[2:]) != (6,) or counts.numel() < V:
        raise ValueError(f"rows {tuple(rows.shape)} / counts {tuple(counts.shape)}: expected [V, max_rows, 6] and [V]")
    limit = _lib.lib().kodhip_merge_max_rows()
    need = int(np.diff(start).max()) * max_rows
    if need > limit:
        raise ValueError(f"an image brings {need} rows to the merge (views x max_rows), more than {limit}")
    dev = rows.device
    rows, counts = rows.contiguous(), counts.contiguous()
    assert rows.dtype == torch.float32 and counts.dtype == torch.int32
    max_det = int(max_det)
    key_cap = _key_cap(need)
    keys = _workspace(dev, n_images * key_cap)
    vs = torch.from_numpy(start.astype(np.int32)).to(dev)
    out = torch.empty((n_images, max_det, 6), dtype=torch.float32, device=dev)
    nout = torch.empty(n_images, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().kodhip_merge_detections(rows.data_ptr(), counts.data_ptr(), vs.data_ptr(), keys.data_ptr(), key_cap,
                                                  out.data_ptr(), nout.data_ptr(), n_images, max_rows, max_det,
                                                  _MERGE_METRICS[metric], float(thres), _MERGE_MODES[mode], 1 if agnostic else 0,
                                                  torch.cuda.current_stream().cuda_stream), "merge_detections")
    kept = _host.fetch(nout)[0].tolist()                             # the one hand-off of a tiled call (sizes the outputs)
    return PackedDetections([out[b, :n] for b, n in enumerate(kept)], out, nout)


def fuse_detections(rows: torch.Tensor, counts: torch.Tensor, view_start, weights=None, *, thres: float = 0.55,
                    agnostic: bool = False, max_det: int = 300) -> PackedDetections:
    """Weighted boxes fusion of an ensemble's detections (kodhip_fuse_detections): rows [V, max_rows, 6], counts [V] and
    `view_start` as in merge_detections, the views of an image being the ensemble's members.  weights: None (all ones) or
    one float per view, finite and > 0.  Rows are taken by score * weight, best first; each joins the cluster of its class
    (any class when `agnostic`) whose current fused box it overlaps most, with IoU > thres, or opens a cluster; a cluster's
    box is the score-weighted mean of its members, its score their mean score scaled by min(members, sum of the image's
    weights) / that sum.  -> per image [n <= max_det, 6], best fused score first."""
    _lib.require_gpu()
    if not 1 <= int(max_det) <= 300:
        raise ValueError(f"max_det {max_det}: expected 1..300")
    if not 0.0 <= float(thres) <= 1.0:
        raise ValueError(f"thres {thres}: expected a value in [0, 1]")
    start = np.asarray(view_start, dtype=np.int64).reshape(-1)
    V, max_rows = int(rows.shape[0]), int(rows.shape[1])
    n_images = len(start) - 1
    if n_images < 1 or start[0] != 0 or start[-1] > V or (np.diff(start) < 0).any():
        raise ValueError(f"view_start {start.tolist()}: expected 0 = s[0] <= s[1] <= ... <= {V} for at least one image")
    if rows.dim() != 3 or tuple(rows.shape[2:]) != (6,) or max_rows < 1 or counts.numel() < V:
        raise ValueError(f"rows {tuple(rows.shape)} / counts {tuple(counts.shape)}: expected [V, max_rows, 6] and [V]")
    if weights is None:
        w = np.ones(V, dtype=np.float32)
    else:
        w = np.asarray(weights.detach().cpu() if torch.is_tensor(weights) else weights, dtype=np.float32).reshape(-1)
        if len(w) != V or not (np.isfinite(w).all() and (w > 0).all()):
            raise ValueError(f"weights {w.tolist()}: expected {V} finite values > 0, one per view")
    limit = _lib.lib().kodhip_fuse_max_rows()
    need = int(np.diff(start).max()) * max_rows
    if need > limit:
        raise ValueError(f"an image brings {need} rows to the fusion (views x max_rows), more than {limit}")
    dev = rows.device
    rows, counts = rows.contiguous(), counts.contiguous()
    assert rows.dtype == torch.float32 and counts.dtype == torch.int32
    max_det = int(max_det)
    key_cap = _key_cap(need)
    keys = _workspace(dev, n_images * key_cap)
    vs = torch.from_numpy(start.astype(np.int32)).to(dev)
    vw = torch.from_numpy(w).to(dev)
    out = torch.empty((n_images, max_det, 6), dtype=torch.float32, device=dev)
    nout = torch.empty(n_images, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().kodhip_fuse_detections(rows.data_ptr(), counts.data_ptr(), vs.data_ptr(), vw.data_ptr(), keys.data_ptr(),
                                                 key_cap, out.data_ptr(), nout.data_ptr(), n_images, max_rows, max_det,
                                                 float(thres), 1 if agnostic else 0,
                                                 torch.cuda.current_stream().cuda_stream), "fuse_detections")
    kept = _host.fetch(nout)[0].tolist()                             # the one hand-off of the fusion (sizes the outputs)
    return PackedDetections([out[b, :n] for b, n in enumerate(kept)], out, nout)
