"""On-device detection confusion matrix - YOLOv5's `ConfusionMatrix.process_batch` (val.py / utils/metrics.py) made
deterministic, without leaving the GPU: which classes are taken for which, which objects are missed outright and which
detections sit on nothing.

    cm = DeviceConfusionMatrix(num_classes, class_names)        # conf_thres 0.25, iou_thres 0.45: YOLOv5's
    cm.add_batch(targets, detections)      # same arguments as DeviceMAPEvaluator.add_batch; never waits for the device
    m = cm.matrix()                        # int64 [nc+1, nc+1], row = predicted, column = true, index nc = background
    pc = cm.per_class()                    # precision / recall / f1 / missed / background_fp per class
    cm.reset()

Matching runs in csrc/confusion.hip (the rule is spelled out there and in include/kodhip.h); it is class-agnostic, which
is what fills the off-diagonal cells - the COCO matcher of csrc/map_match.hip only ever pairs equal classes.  The matrix
stays on the device and is added to by every launch; `matrix()` is the one host hand-off.
`add_batch` takes non_max_suppression's result as it lies on the device (core.nms.PackedDetections: one [B, 300, 6] buffer
and its device-side counts); any other list of [n, 6] tensors is packed here.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from ... import _lib
from ...core.label_assignment.yv5 import BatchedTargets
from ...core.nms import PackedDetections

_RING = 8          # pinned upload slots for the per-image detection counts (see PinnedCountUpload)


def reduce_counts(counts: torch.Tensor, process_group=None) -> torch.Tensor:
    """Sum an integer count tensor over the ranks of `process_group` (all_reduce SUM; counts are never averaged).  Takes a
    CPU or CUDA tensor and moves it to where the group's backend works (gloo: host, nccl: device).  -> the summed tensor,
    identical on every rank; `counts` itself unchanged.  process_group None: no collective, a copy."""
    out = counts.clone()
    if process_group is None:
        return out
    import torch.distributed as dist
    if dist.get_world_size(process_group) == 1:
        return out
    backend = dist.get_backend(process_group)
    if backend == "nccl" and not out.is_cuda:
        out = out.cuda()
    elif backend == "gloo" and out.is_cuda:
        out = out.cpu()
    dist.all_reduce(out, op=dist.ReduceOp.SUM, group=process_group)
    return out


def per_class_from(matrix: np.ndarray) -> dict:
    """matrix int64 [nc+1, nc+1] (row = predicted, column = true, last = background) -> arrays of length nc:
    precision = diag / row sum, recall = diag / column sum, f1 = their harmonic mean (NaN where a denominator is 0),
    missed = matrix[nc, :nc], background_fp = matrix[:nc, nc]."""
    m = np.asarray(matrix, dtype=np.int64)
    nc = m.shape[0] - 1
    diag = np.diag(m)[:nc].astype(np.float64)
    rows, cols = m[:nc].sum(1).astype(np.float64), m[:, :nc].sum(0).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = np.where(rows > 0, diag / rows, np.nan)
        recall = np.where(cols > 0, diag / cols, np.nan)
        f1 = np.where(precision + recall > 0, 2 * precision * recall / (precision + recall), np.nan)
    return {"precision": precision, "recall": recall, "f1": f1, "missed": m[nc, :nc].copy(), "background_fp": m[:nc, nc].copy()}


class PinnedCountUpload:
    """The per-image detection counts are host integers (tensor shapes).  torch.tensor(counts, device=dev) is a
    pageable copy: it blocks the host until the stream has drained.  Here: an asynchronous copy out of a pinned slot;
    a slot is reused _RING batches later, behind the event recorded after its copy (long complete by then)."""

    def __init__(self):
        self._ring, self._slot = [], 0

    def __call__(self, counts, dev) -> torch.Tensor:
        B = len(counts)
        if not self._ring or self._ring[0][0].numel() < B:
            self._ring = [[torch.empty(max(B, 64), dtype=torch.int32).pin_memory(), None] for _ in range(_RING)]
        slot = self._ring[self._slot]
        self._slot = (self._slot + 1) % _RING
        if slot[1] is not None:
            slot[1].synchronize()
        host = slot[0][:B]
        host.copy_(torch.tensor(counts, dtype=torch.int32))
        ndet = torch.empty(B, dtype=torch.int32, device=dev)
        ndet.copy_(host, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record()
        return ndet


class DeviceConfusionMatrix:
    def __init__(self, num_classes: int, class_names: Sequence[str] | None = None, conf_thres: float = 0.25,
                 iou_thres: float = 0.45):
        self.nc = num_classes
        self.names = list(class_names) if class_names else [str(i) for i in range(num_classes)]
        self.conf_thres, self.iou_thres = float(conf_thres), float(iou_thres)
        self._m = None                  # device int64 [(nc+1)^2], allocated with the first batch (its device)
        self._upload_counts = PinnedCountUpload()
        self._arange = {}

    def reset(self):
        if self._m is not None:
            self._m.zero_()

    def add_batch(self, targets, detections: Sequence[torch.Tensor]):
        """detections: list of [n, 6] tensors (non_max_suppression output, descending score; its PackedDetections is used in
        place, any other list is packed here with the counts taken from the tensors' shapes); targets: a
        Sequence[DetectionTarget] or a BatchedTargets.  Launches only: no value is read back."""
        _lib.require_gpu()
        B = len(detections)
        if B == 0:
            return
        dev = detections[0].device
        lib = _lib.lib()
        if isinstance(detections, PackedDetections):       # the NMS output as it lies on the device: nothing to pack or upload
            det, ndet = detections.packed, detections.counts
        else:
            counts = [int(d.shape[0]) for d in detections]
            det = torch.zeros((B, max(counts + [1]), 6), dtype=torch.float32, device=dev)
            for b, d in enumerate(detections):
                if d.shape[0]:
                    det[b, :d.shape[0]] = d
            ndet = self._upload_counts(counts, dev)
        if det.shape[1] > lib.kodhip_confusion_max_det():
            raise ValueError(f"an image carries {det.shape[1]} detections; the device confusion matrix holds at most "
                             f"{lib.kodhip_confusion_max_det()} per image (csrc/confusion.hip)")
        bt = targets if isinstance(targets, BatchedTargets) else BatchedTargets.from_targets(targets, dev)
        if bt.n:
            # offsets of each image's boxes (images are concatenated in order): start[i] = #{samples < i}.  One search per
            # image on the device; torch.bincount would read its largest value back to size its output.
            edges = self._arange.get((B, dev))
            if edges is None:
                edges = self._arange[(B, dev)] = torch.arange(B + 1, dtype=torch.int32, device=dev)
            start = torch.searchsorted(bt.samples.to(torch.int32), edges, out_int32=True)
        else:
            start = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        if self._m is None:
            self._m = torch.zeros((self.nc + 1) ** 2, dtype=torch.int64, device=dev)
        _lib.check(lib.kodhip_confusion_match(det.data_ptr(), ndet.data_ptr(), bt.boxes.data_ptr() if bt.n else None,
                                              bt.labels.data_ptr() if bt.n else None, start.data_ptr(), self._m.data_ptr(),
                                              B, det.shape[1], self.nc, self.conf_thres, self.iou_thres,
                                              torch.cuda.current_stream().cuda_stream), "confusion_match")

    def matrix(self, process_group=None) -> np.ndarray:
        """int64 [nc+1, nc+1]; with a process group the counts of its ranks are summed (all_reduce SUM)."""
        m = self._m if self._m is not None else torch.zeros((self.nc + 1) ** 2, dtype=torch.int64)
        return reduce_counts(m, process_group).cpu().numpy().reshape(self.nc + 1, self.nc + 1)

    def per_class(self, process_group=None) -> dict:
        return per_class_from(self.matrix(process_group))
