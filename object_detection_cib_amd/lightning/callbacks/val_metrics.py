"""YOLOv5's validation table on the device - val.py's `process_batch` plus utils/metrics.py's `ap_per_class`: precision,
recall, F1, mAP@.5 and mAP@.5:.95 per class and overall, and the confidence at which F1 peaks (what a user passes to
`Detector(conf_thres=...)`).

    vm = DeviceDetectionMetrics(num_classes, class_names)        # IoU thresholds np.linspace(0.5, 0.95, 10): YOLOv5's
    vm.add_batch(targets, detections)      # same arguments as DeviceMAPEvaluator.add_batch; never waits for the device
    res = vm.compute()                     # the one host hand-off: curves [nc, 1000], AP [nc, T], counts
    res["map50"], res["map"], res["best_conf"], res["per_class"]["precision"][c]
    vm.reset()

Matching and the curves run in csrc/val_metrics.hip (the rule, the record layout and the order contract are spelled out
there and in include/kodhip.h).  Every detection with a class in [0, nc) becomes one 8-byte record {score, class, mask over
the IoU thresholds} in a device-resident store; the store grows by doubling from the bound the host knows without asking the
device (the sum of B * max_det over the batches), so nothing is ever dropped and `add_batch` only launches.  `compute()`
sorts the records (class ascending, score descending, arrival ascending), evaluates the curves in fp64 on the device and
finishes with `summarize`, plain numpy over the classes that have ground truth.
`merge(other)` appends another evaluator's records behind this one's; `gather(process_group)` does that over the ranks of a
group in rank order, so every rank ends with identical state (the whole validation set's metrics).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from ... import _lib
from ...core.label_assignment.yv5 import BatchedTargets
from ...core.nms import PackedDetections
from .confusion import PinnedCountUpload

PX = np.linspace(0, 1, 1000)          # confidence grid of the precision / recall / F1 curves
X101 = np.linspace(0, 1, 101)         # recall grid of the AP integral (COCO's 101 points)
DEFAULT_IOUS = np.linspace(0.5, 0.95, 10)


def smooth(y: np.ndarray, f: float = 0.05) -> np.ndarray:
    """YOLOv5's box filter of fraction f: nf = round(len(y) * f * 2) // 2 + 1 taps (odd), the ends padded with the end
    values, `valid` convolution -> same length as y."""
    nf = round(len(y) * f * 2) // 2 + 1
    pad = np.ones(nf // 2)
    yp = np.concatenate((pad * y[0], y, pad * y[-1]), 0)
    return np.convolve(yp, np.ones(nf) / nf, mode="valid")


def summarize(p: np.ndarray, r: np.ndarray, ap: np.ndarray, nt: np.ndarray, n_p: Optional[np.ndarray] = None,
              px: np.ndarray = PX) -> dict:
    """The tail of ap_per_class over the classes with ground truth.  p, r [nc, len(px)], ap [nc, T], nt [nc].
    f1 = 2 p r / (p + r + 1e-16); i = first argmax of smooth(f1.mean(0), 0.1); per class P, R, F1 at px[i], AP at the first
    threshold and the mean over thresholds (0 for classes without ground truth); mp / mr / mf1 / map50 / map their means
    over the classes with ground truth; best_conf = px[i].  No ground truth at all: everything 0.0."""
    p, r, ap = np.asarray(p, np.float64), np.asarray(r, np.float64), np.asarray(ap, np.float64)
    nt = np.asarray(nt, np.int64)
    nc = len(nt)
    f1 = 2 * p * r / (p + r + 1e-16)
    seen = np.flatnonzero(nt > 0)
    per = {k: np.zeros(nc) for k in ("precision", "recall", "f1", "ap50", "ap")}
    out = {"classes": seen, "per_class": per, "nt": nt, "n_p": None if n_p is None else np.asarray(n_p, np.int64),
           "curves": {"px": px, "p": p, "r": r, "f1": f1, "ap": ap}}
    if len(seen) == 0:
        out.update(best_index=0, best_conf=0.0, mp=0.0, mr=0.0, mf1=0.0, map50=0.0, map=0.0)
        return out
    i = int(smooth(f1[seen].mean(0), 0.1).argmax())
    per["precision"][seen], per["recall"][seen], per["f1"][seen] = p[seen, i], r[seen, i], f1[seen, i]
    per["ap50"][seen], per["ap"][seen] = ap[seen, 0], ap[seen].mean(1)
    out.update(best_index=i, best_conf=float(px[i]), mp=float(p[seen, i].mean()), mr=float(r[seen, i].mean()),
               mf1=float(f1[seen, i].mean()), map50=float(ap[seen, 0].mean()), map=float(ap[seen].mean(1).mean()))
    return out


class DeviceDetectionMetrics:
    def __init__(self, num_classes: int, class_names: Sequence[str] | None = None, iou_thresholds=None, *,
                 initial_capacity: int = 1 << 16):
        self.nc = int(num_classes)
        self.names = list(class_names) if class_names else [str(i) for i in range(num_classes)]
        self.iou_thresholds = np.ascontiguousarray(DEFAULT_IOUS if iou_thresholds is None else iou_thresholds, dtype=np.float64)
        if self.iou_thresholds.ndim != 1 or not 1 <= len(self.iou_thresholds) <= 16:
            raise ValueError("iou_thresholds: 1 to 16 values")
        if not 1 <= self.nc <= 65536:
            raise ValueError("num_classes outside 1 .. 65536")
        self.initial_capacity = max(int(initial_capacity), 1)
        self._rec = None                # device int32 [capacity, 2]: the record store (allocated with the first batch)
        self._count = None              # device int32 [1]: records in the store
        self._nt = None                 # device int64 [nc]: ground truths per class
        self._bound = 0                 # host: sum of B * max_det over the batches, >= the device-side count
        self._offsets = None
        self._upload_counts = PinnedCountUpload()
        self._arange = {}
        self._grids = None

    # ---- state ------------------------------------------------------------------------------------------------------
    @property
    def capacity(self) -> int:
        return 0 if self._rec is None else int(self._rec.shape[0])

    def reset(self):
        if self._rec is not None:
            self._count.zero_()
            self._nt.zero_()
        self._bound = 0

    def _reserve(self, bound: int, dev):
        """capacity >= bound, by doubling; the old records move with one device-to-device copy.  No read-back: `bound`
        is what the host knows."""
        if bound > 1 << 30:
            raise ValueError(f"{bound} detection slots: the record store holds at most 2^30")
        if self._rec is None:
            self._count = torch.zeros(1, dtype=torch.int32, device=dev)
            self._nt = torch.zeros(self.nc, dtype=torch.int64, device=dev)
        cap = self.capacity or self.initial_capacity
        while cap < bound:
            cap *= 2
        cap = min(cap, 1 << 30)
        if cap != self.capacity:
            new = torch.empty((cap, 2), dtype=torch.int32, device=dev)
            if self._rec is not None:
                new[:self._rec.shape[0]].copy_(self._rec)
            self._rec = new

    # ---- per batch --------------------------------------------------------------------------------------------------
    def add_batch(self, targets, detections: Sequence[torch.Tensor]):
        """detections: list of [n, 6] tensors (non_max_suppression output, descending score; its PackedDetections is used in
        place, any other list is packed here); targets: a Sequence[DetectionTarget] or a BatchedTargets.  Launches only."""
        _lib.require_gpu()
        B = len(detections)
        if B == 0:
            return
        dev = detections[0].device
        lib = _lib.lib()
        if isinstance(detections, PackedDetections):
            det, ndet = detections.packed, detections.counts
        else:
            counts = [int(d.shape[0]) for d in detections]
            det = torch.zeros((B, max(counts + [1]), 6), dtype=torch.float32, device=dev)
            for b, d in enumerate(detections):
                if d.shape[0]:
                    det[b, :d.shape[0]] = d
            ndet = self._upload_counts(counts, dev)
        max_det = int(det.shape[1])
        if max_det > lib.kodhip_val_max_det():
            raise ValueError(f"an image carries {max_det} detections; the device metrics hold at most "
                             f"{lib.kodhip_val_max_det()} per image (csrc/val_metrics.hip)")
        bt = targets if isinstance(targets, BatchedTargets) else BatchedTargets.from_targets(targets, dev)
        if bt.n:
            edges = self._arange.get((B, dev))
            if edges is None:
                edges = self._arange[(B, dev)] = torch.arange(B + 1, dtype=torch.int32, device=dev)
            start = torch.searchsorted(bt.samples.to(torch.int32), edges, out_int32=True)
        else:
            start = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        self._reserve(self._bound + B * max_det, dev)
        self._bound += B * max_det
        if self._offsets is None or self._offsets.numel() < B:
            self._offsets = torch.empty(max(B, 64), dtype=torch.int32, device=dev)
        thr = self.iou_thresholds
        _lib.check(lib.kodhip_val_match(det.data_ptr(), ndet.data_ptr(), bt.boxes.data_ptr() if bt.n else None,
                                        bt.labels.data_ptr() if bt.n else None, start.data_ptr(),
                                        thr.ctypes.data_as(C.POINTER(C.c_double)), len(thr), self._rec.data_ptr(),
                                        self._count.data_ptr(), self.capacity, self._nt.data_ptr(), self._offsets.data_ptr(),
                                        B, max_det, self.nc, torch.cuda.current_stream().cuda_stream), "val_match")

    # ---- combining evaluators -----------------------------------------------------------------------------------------
    def _append(self, rec: torch.Tensor, count: torch.Tensor, bound: int, nt: torch.Tensor):
        """`rec` int32 [>= bound, 2] and `count` int32 [1] on the device: its first min(count, bound) records go behind this
        store's; nt int64 [nc] is added.  Launches only."""
        _lib.require_gpu()
        dev = rec.device
        self._reserve(max(self._bound + bound, 1), dev)
        if bound:
            _lib.check(_lib.lib().kodhip_val_append(self._rec.data_ptr(), self._count.data_ptr(), self.capacity, rec.data_ptr(),
                                                    count.data_ptr(), bound, torch.cuda.current_stream().cuda_stream),
                       "val_append")
            self._bound += bound
        self._nt += nt.to(dev)

    def add_records(self, scores, classes, masks, nt):
        """Append records given as arrays (scores fp32 >= 0, classes in [0, nc), masks: bit t set = correct at threshold t)
        and add nt [nc] ground truths per class: how a caller with its own matcher, or a test, feeds the curves."""
        scores = np.ascontiguousarray(scores, dtype=np.float32)
        n = len(scores)
        rec = np.zeros((max(n, 1), 2), np.uint32)
        rec[:n, 0] = scores.view(np.uint32)
        rec[:n, 1] = (np.asarray(classes, dtype=np.int64) & 0xFFFF) | ((np.asarray(masks, dtype=np.int64) & 0xFFFF) << 16)
        dev = self._rec.device if self._rec is not None else torch.device("cuda")
        self._append(torch.from_numpy(rec.view(np.int32)).to(dev), torch.tensor([n], dtype=torch.int32).to(dev), n,
                     torch.from_numpy(np.asarray(nt, dtype=np.int64)))

    def merge(self, other: "DeviceDetectionMetrics"):
        """Append `other`'s records behind this evaluator's and add its ground-truth counts: the state of one evaluator fed
        this one's batches, then the other's.  `other` is left as it is."""
        if other.nc != self.nc or not np.array_equal(other.iou_thresholds, self.iou_thresholds):
            raise ValueError("merge: evaluators with different classes or IoU thresholds")
        if other._rec is not None:
            self._append(other._rec, other._count, other._bound, other._nt)
        return self

    def gather(self, process_group=None):
        """Replace this evaluator's state by the records of every rank of `process_group`, appended in rank order (identical
        state on every rank).  Tensors travel where the group's backend works (gloo: host, nccl: device)."""
        import torch.distributed as dist
        if process_group is None or dist.get_world_size(process_group) == 1:
            return self
        world = dist.get_world_size(process_group)
        on_host = dist.get_backend(process_group) == "gloo"
        dev = self._rec.device if self._rec is not None else torch.device("cuda")
        via = (lambda t: t.cpu()) if on_host else (lambda t: t.to(dev))
        bounds = [torch.zeros(1, dtype=torch.int64, device="cpu" if on_host else dev) for _ in range(world)]
        dist.all_gather(bounds, via(torch.tensor([self._bound], dtype=torch.int64)), group=process_group)
        bounds = [int(b) for b in bounds]
        width = max(max(bounds), 1)
        mine = torch.zeros((width, 2), dtype=torch.int32, device=dev)
        head = torch.zeros(1 + self.nc, dtype=torch.int64, device=dev)          # [count, nt...]
        if self._rec is not None:
            mine[:self._bound].copy_(self._rec[:self._bound])
            head[0], head[1:] = self._count[0], self._nt
        recs = [torch.empty_like(via(mine)) for _ in range(world)]
        heads = [torch.empty_like(via(head)) for _ in range(world)]
        dist.all_gather(recs, via(mine), group=process_group)
        dist.all_gather(heads, via(head), group=process_group)
        self.reset()
        for rec, h, bound in zip(recs, heads, bounds):
            h = h.to(dev)
            self._append(rec.to(dev), h[:1].to(torch.int32), bound, h[1:])
        return self

    # ---- once per epoch ---------------------------------------------------------------------------------------------
    def curves(self) -> dict:
        """-> {"p" [nc, 1000], "r" [nc, 1000], "ap" [nc, T], "nt" [nc], "n_p" [nc]} as numpy arrays: the launches of
        kodhip_val_curves and the single read-back."""
        nc, T = self.nc, len(self.iou_thresholds)
        if self._rec is None:
            return {"p": np.zeros((nc, len(PX))), "r": np.zeros((nc, len(PX))), "ap": np.zeros((nc, T)),
                    "nt": np.zeros(nc, np.int64), "n_p": np.zeros(nc, np.int64)}
        _lib.require_gpu()
        lib = _lib.lib()
        dev = self._rec.device
        if self._grids is None or self._grids[0].device != dev:
            self._grids = (torch.from_numpy(PX).to(dev), torch.from_numpy(X101).to(dev))
        px, xr = self._grids
        # capacity handed to the kernels: the bound (every record lies below it), not the allocation
        cap = max(self._bound, 1)
        ws_bytes = lib.kodhip_val_curves_workspace_bytes(cap, nc, T)
        if ws_bytes < 0:
            raise RuntimeError("val_curves: bad workspace arguments")
        ws = torch.empty(ws_bytes // 8 + 2, dtype=torch.int64, device=dev)
        ws_ptr = (ws.data_ptr() + 15) & ~15
        npx = len(PX)
        sizes = (nc * npx, nc * npx, nc * T, nc, nc)                   # p, r, ap, nt, n_p: one buffer of 8-byte words
        out = torch.zeros(sum(sizes), dtype=torch.float64, device=dev)
        o = np.concatenate(([0], np.cumsum(sizes)))
        ptr = lambda k: out.data_ptr() + 8 * int(o[k])                 # noqa: E731
        out[o[3]:o[4]].view(torch.int64).copy_(self._nt)
        _lib.check(lib.kodhip_val_curves(self._rec.data_ptr(), self._count.data_ptr(), cap, self._nt.data_ptr(), px.data_ptr(), npx,
                                         xr.data_ptr(), len(X101), nc, T, ws_ptr, ptr(0), ptr(1), ptr(2), ptr(4),
                                         torch.cuda.current_stream().cuda_stream), "val_curves")
        host = out.cpu().numpy()
        ints = host.view(np.int64)
        return {"p": host[o[0]:o[1]].reshape(nc, npx).copy(), "r": host[o[1]:o[2]].reshape(nc, npx).copy(),
                "ap": host[o[2]:o[3]].reshape(nc, T).copy(), "nt": ints[o[3]:o[4]].copy(), "n_p": ints[o[4]:o[5]].copy()}

    def compute(self, process_group=None) -> dict:
        """The table: see `summarize`.  With a process group the records of its ranks are gathered first."""
        if process_group is not None:
            self.gather(process_group)
        c = self.curves()
        return summarize(c["p"], c["r"], c["ap"], c["nt"], c["n_p"])

    def records(self):
        """(scores fp32 [n], classes [n], masks [n]) in arrival order - a host copy, for inspection and tests."""
        if self._rec is None:
            return np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)
        n = int(self._count.item())
        rec = self._rec[:n].cpu().numpy().view(np.uint32)
        return rec[:, 0].copy().view(np.float32), (rec[:, 1] & 0xFFFF).astype(np.int64), (rec[:, 1] >> 16).astype(np.int64)

    def ground_truths(self) -> np.ndarray:
        return np.zeros(self.nc, np.int64) if self._nt is None else self._nt.cpu().numpy()
