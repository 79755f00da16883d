"""Multi-scale training (YOLOv5 train.py --multi-scale): every batch is resized to a random multiple of 32 between 0.5 and
1.5 of the training size before it goes through the network.

* `multiscale_sizes` / `MultiScaleSchedule`: which canvas a step runs at - host, pure Python.
* `resize_batch`: one kodhip_multiscale_batch launch (csrc/multiscale.hip): the batch, already on the device at the base
  size, resized into the network's input layout, and its boxes scaled with it.
* `MultiScaleTrainStep`: one captured GraphedTrainStep per canvas behind one staging input and one target block; a call
  draws the size, resizes with one launch and replays that size's graph.  No host synchronisation.
"""
from __future__ import annotations

import math
import random
from collections import OrderedDict
from typing import Optional, Sequence, Tuple

import torch

from .. import _lib
from .graphed import _KEEP, GraphedTrainStep, TargetBlock


def _canvas(H: int, W: int, sz: int, gs: int) -> Tuple[int, int]:
    sf = sz / max(H, W)
    if sf == 1:
        return H, W
    return math.ceil(H * sf / gs) * gs, math.ceil(W * sf / gs) * gs


def _plan_sz(H: int, W: int, scale_range, gs: int):
    """the `sz` values YOLOv5's draw can produce, ascending"""
    S = max(H, W)
    lo, hi = scale_range
    a, b = int(S * lo), int(S * hi) + gs
    if not (0 < lo <= hi) or gs < 1 or a >= b:
        raise ValueError(f"multi-scale: bad scale_range {scale_range!r} / grid size {gs}")
    return list(range(a // gs * gs, (b - 1) // gs * gs + 1, gs))


def multiscale_sizes(H: int, W: int, scale_range=(0.5, 1.5), gs: int = 32):
    """The distinct (h, w) canvases of the plan of a base size H x W, smallest first."""
    out = []
    for sz in _plan_sz(H, W, scale_range, gs):
        c = _canvas(H, W, sz, gs)
        if c not in out:
            out.append(c)
    return out


class MultiScaleSchedule:
    """YOLOv5's draw, with Python floats, on a generator of its own (random.Random(seed), never the global one):

        S = max(H, W);  sz = rng.randrange(int(S * lo), int(S * hi) + gs) // gs * gs;  sf = sz / S
        (h, w) = (H, W) if sf == 1 else ceil(x * sf / gs) * gs per axis

    A new size is drawn every `interval` steps.  `sizes` (an explicit list of sz values) replaces the randrange by
    rng.choice over that list.  The end sizes of a range that is no multiple of gs come at a lower weight (base 416:
    192 and 640 at half weight), as in YOLOv5.

    The k-th draw is a function of (seed, k) only, so every data-parallel rank that builds the schedule with the same
    arguments draws the same size at the same step.  That is required, not a convenience: SyncBN exchanges per-rank
    statistics of equal local shapes and refuses uneven ones, and the ranks' captured steps must be the same graphs.
    state_dict() / load_state_dict() carry (seed, number of draws, steps); a resume replays the draws."""

    def __init__(self, H: int, W: int, seed: int = 0, scale_range=(0.5, 1.5), gs: int = 32, interval: int = 1,
                 sizes: Optional[Sequence[int]] = None):
        self.H, self.W, self.gs = int(H), int(W), int(gs)
        self.scale_range = (float(scale_range[0]), float(scale_range[1]))
        self.interval = int(interval)
        if self.interval < 1:
            raise ValueError(f"multi-scale: interval {interval}: expected >= 1")
        self.sizes = None if sizes is None else [int(s) for s in sizes]
        plan = self.sizes if self.sizes is not None else _plan_sz(self.H, self.W, self.scale_range, self.gs)
        if not plan or min(plan) < self.gs:
            raise ValueError(f"multi-scale: size {min(plan) if plan else None} is below the grid size {self.gs} "
                             f"(base {self.H} x {self.W}, scale_range {self.scale_range}, sizes {self.sizes})")
        self.seed = int(seed)
        self._rng = random.Random(self.seed)
        self.draws, self.steps = 0, 0
        self.sz, self.size = None, None

    def canvases(self):
        """the distinct (h, w) this schedule can produce"""
        if self.sizes is None:
            return multiscale_sizes(self.H, self.W, self.scale_range, self.gs)
        out = []
        for sz in sorted(set(self.sizes)):
            c = _canvas(self.H, self.W, sz, self.gs)
            if c not in out:
                out.append(c)
        return out

    def _draw(self):
        S = max(self.H, self.W)
        if self.sizes is not None:
            sz = self._rng.choice(self.sizes)
        else:
            lo, hi = self.scale_range
            sz = self._rng.randrange(int(S * lo), int(S * hi) + self.gs) // self.gs * self.gs
        self.draws += 1
        self.sz, self.size = sz, _canvas(self.H, self.W, sz, self.gs)

    def next(self) -> Tuple[int, int]:
        """the canvas (h, w) of the next step"""
        if self.steps % self.interval == 0:
            self._draw()
        self.steps += 1
        return self.size

    def state_dict(self) -> dict:
        return {"seed": self.seed, "draws": self.draws, "steps": self.steps}

    def load_state_dict(self, state: dict):
        self.seed = int(state["seed"])
        self._rng = random.Random(self.seed)
        self.draws, self.steps, self.sz, self.size = 0, 0, None, None
        for _ in range(int(state["draws"])):
            self._draw()
        self.steps = int(state.get("steps", self.draws * self.interval))


def resize_batch(lib, src: torch.Tensor, out_pairs: torch.Tensor, h: int, w: int, out_f32: Optional[torch.Tensor] = None,
                 boxes_in: Optional[torch.Tensor] = None, boxes_out: Optional[torch.Tensor] = None, n: int = 0):
    """One kodhip_multiscale_batch launch on the current stream.  src: fp32 [B, 3, H, W] or bf16 pairs [B, H, W/2, 8]."""
    pairs = src.dtype == torch.bfloat16
    if pairs:
        B, H, W = src.shape[0], src.shape[1], src.shape[2] * 2
        assert src.dim() == 4 and src.shape[3] == 8 and src.is_contiguous(), src.shape
    else:
        B, _, H, W = src.shape
        assert src.dtype == torch.float32 and src.shape[1] == 3 and src.is_contiguous(), (src.shape, src.dtype)
    assert tuple(out_pairs.shape) == (B, h, w // 2, 8) and out_pairs.dtype == torch.bfloat16 and out_pairs.is_contiguous()
    assert out_f32 is None or (tuple(out_f32.shape) == (B, 3, h, w) and out_f32.dtype == torch.float32 and out_f32.is_contiguous())
    if n:
        assert boxes_in.dtype == torch.float64 and boxes_out.dtype == torch.float64 and boxes_in.is_contiguous() and boxes_out.is_contiguous()
        assert boxes_in.numel() >= 4 * n and boxes_out.numel() >= 4 * n
    _lib.check(lib.kodhip_multiscale_batch(None if pairs else src.data_ptr(), src.data_ptr() if pairs else None, out_pairs.data_ptr(),
                                           None if out_f32 is None else out_f32.data_ptr(), B, H, W, h, w,
                                           boxes_in.data_ptr() if n else None, boxes_out.data_ptr() if n else None, int(n),
                                           torch.cuda.current_stream().cuda_stream), "multiscale_batch")


class MultiScaleTrainStep:
    """GraphedTrainStep over changing input sizes: one captured single-shape step per canvas of a MultiScaleSchedule.

    It owns one base-size staging input (fp32 NCHW, or bf16 pixel pairs with input_pairs=True: `input_buffer()` hands it out so
    that a pipeline can composite straight into it), one target block in base coordinates that GraphedTrainStep's pinned-ring
    upload fills, and per canvas a GraphedTrainStep(input_pairs=True) that reads that same block.  A call draws the size,
    takes (or captures) that size's step, issues ONE kodhip_multiscale_batch launch - it writes the size's engine input
    buffer and scales the boxes of the block in place - and replays.  A size met for the first time is captured with
    preserve_state=True on the resized batch and then replayed on it like any other: no batch is lost and the trajectory does
    not move.  A step at the base size resizes with l1 = 0, i.e. copies: it is GraphedTrainStep's step bit for bit.

    max_graphs: None keeps every size; otherwise the least recently used step is released (graph dropped, shape unpinned)
    and a size that returns is captured again.  Every captured size holds a full engine buffer set: when the plan does not
    fit in device memory, narrow `scale_range`, list fewer `sizes`, bound `max_graphs`, and raise `interval` so that captures
    come less often.

    Data parallel: build every rank's step with the same seed (see MultiScaleSchedule)."""

    def __init__(self, net, loss, batch_size: int, height: int, width: int, max_targets: int = 4096,
                 loss_scale: Optional[float] = None, input_pairs: bool = False,
                 gradient_clip_val: Optional[float] = None, gradient_clip_algorithm: str = "norm",
                 skip_nonfinite: bool = False, track_grad_norm: bool = False, *, scale_range=(0.5, 1.5),
                 sizes: Optional[Sequence[int]] = None, interval: int = 1, seed: int = 0, max_graphs: Optional[int] = None,
                 optimizer: str = "sgd", accumulate_grad_batches: int = 1):
        """optimizer: "sgd" | "adam", passed to every GraphedTrainStep it builds (with "adam" a call takes `adam=` like
        GraphedTrainStep.__call__).
        accumulate_grad_batches = N, passed on likewise: the steps of all sizes share the engine's window, a size is drawn per
        micro-batch as train.py does (`interval` counts micro-batches), and a size met for the first time inside a window is
        captured without disturbing it.  `stepped` and flush() as on GraphedTrainStep."""
        from .accumulate import check_accumulate_grad_batches
        self.accumulate = check_accumulate_grad_batches(accumulate_grad_batches)
        self.stepped = False
        self._last = None                 # the step of the last call (flush() closes the window through it)
        if gradient_clip_algorithm not in ("norm", "value"):
            raise ValueError(f"gradient_clip_algorithm {gradient_clip_algorithm!r}: expected 'norm' or 'value'")
        if optimizer not in ("sgd", "adam"):
            raise ValueError(f"optimizer {optimizer!r}: expected 'sgd' or 'adam'")
        if optimizer == "adam" and skip_nonfinite:
            raise ValueError("skip_nonfinite with optimizer='adam' is not supported (the step count lives on the host)")
        self.optimizer = optimizer
        if max_graphs is not None and int(max_graphs) < 1:
            raise ValueError(f"max_graphs {max_graphs}: expected >= 1 or None")
        self.net, self.loss = net, loss
        self.eng = net.engine()
        dev = self.eng.device
        self.B, self.H, self.W = batch_size, height, width
        self.cap = int(max_targets)
        self.loss_scale = loss_scale
        self.input_pairs = bool(input_pairs)
        self.gradient_clip_val = None if gradient_clip_val is None else float(gradient_clip_val)
        self.gradient_clip_algorithm = gradient_clip_algorithm
        self.skip_nonfinite, self.track_grad_norm = bool(skip_nonfinite), bool(track_grad_norm)
        top = max(b.stride for b in self.eng.g.bufs)
        self.schedule = MultiScaleSchedule(height, width, seed, scale_range, top, interval, sizes)
        self.max_graphs = None if max_graphs is None else int(max_graphs)
        if self.input_pairs:
            self.x = torch.zeros((batch_size, height, width // 2, 8), dtype=torch.bfloat16, device=dev)
        else:
            self.x = torch.zeros((batch_size, 3, height, width), dtype=torch.float32, device=dev)
        self._tb = TargetBlock(self.cap, dev, self.eng.lib)
        self.steps: "OrderedDict[Tuple[int, int], GraphedTrainStep]" = OrderedDict()      # least recently used first
        self.size: Optional[Tuple[int, int]] = None
        self.captures = 0                 # how many captures so far (first meetings and returns after an eviction)

    def input_buffer(self) -> torch.Tensor:
        """The base-size staging input.  A data pipeline that runs on the step's stream may write the next batch straight into
        it and pass the same tensor to __call__: no copy between pipeline and step."""
        return self.x

    @property
    def grad_norm(self) -> torch.Tensor:
        """[total, bias, decay, norm] gradient norms of the last step, before clipping (device, static)"""
        return self.eng.clip[0:4]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """steps skipped for a NaN / Inf gradient norm so far (device scalar, static)"""
        return self.eng.clip[6]

    def state_dict(self) -> dict:
        return self.schedule.state_dict()

    def load_state_dict(self, state: dict):
        self.schedule.load_state_dict(state)

    def _evict(self, keep: int):
        while len(self.steps) > keep:
            _, old = self.steps.popitem(last=False)
            torch.cuda.current_stream().synchronize()          # its last replay has finished
            old.release()

    def _new_step(self, h: int, w: int) -> GraphedTrainStep:
        return GraphedTrainStep(self.net, self.loss, self.B, h, w, self.cap, self.loss_scale, True,
                                self.gradient_clip_val, self.gradient_clip_algorithm, self.skip_nonfinite,
                                self.track_grad_norm, target_block=self._tb, optimizer=self.optimizer,
                                accumulate_grad_batches=self.accumulate)

    def __call__(self, images: torch.Tensor, targets, lr: Optional[Sequence[float]] = None,
                 momentum: Optional[Sequence[float]] = None, weight_decay: Optional[Sequence[float]] = None,
                 grad_scale: float = 1.0, gradient_clip_val=_KEEP, gradient_clip_algorithm: Optional[str] = None,
                 adam: Optional[dict] = None):
        """One step on a new base-size batch at the size the schedule draws.  Returns (total, (box, obj, cls)) - static
        tensors of that size's step, overwritten by its next replay (clone to keep)."""
        eng = self.eng
        if gradient_clip_val is not _KEEP:
            self.gradient_clip_val = None if gradient_clip_val is None else float(gradient_clip_val)
        if gradient_clip_algorithm is not None:
            self.gradient_clip_algorithm = gradient_clip_algorithm
        # the guards of GraphedTrainStep.__call__, for every held step: a size that comes back later must not replay stale launches
        if self.steps:
            fz, bn = eng.freeze_flags(), eng.bn_mode_flags()
            cfg = (self.gradient_clip_algorithm if self.gradient_clip_val is not None else None, self.skip_nonfinite,
                   self.track_grad_norm)
            for st in self.steps.values():
                st._guard(fz, bn, cfg)
        assert tuple(images.shape) == tuple(self.x.shape) and (images.dtype == self.x.dtype or not self.input_pairs), \
            (images.shape, images.dtype, self.x.shape)
        h, w = self.size = self.schedule.next()
        if images.data_ptr() != self.x.data_ptr():
            self.x.copy_(images, non_blocking=True)
        n = self._tb.load(targets)
        step = self.steps.get((h, w))
        fresh = step is None
        if fresh:
            if self.max_graphs is not None:
                self._evict(self.max_graphs - 1)
            step = self._new_step(h, w)
        else:
            self.steps.move_to_end((h, w))
        try:
            buf = eng.image_buffer(self.B, h, w)
            resize_batch(eng.lib, self.x, buf, h, w, boxes_in=self._tb.boxes, boxes_out=self._tb.boxes, n=n)
            if fresh:
                if lr is not None and self.optimizer == "sgd":
                    eng.set_hyper(lr, momentum, weight_decay, grad_scale)
                step.capture(buf, None, preserve_state=True,
                             adam=None if adam is None else dict(adam, grad_scale=grad_scale))
                self.steps[(h, w)] = step
                self.captures += 1
        except torch.cuda.OutOfMemoryError as e:
            if fresh:
                step.release()
            raise RuntimeError(
                f"out of device memory while building the multi-scale step of size {h} x {w} ({len(self.steps)} sizes are held; every "
                f"size keeps a full buffer set): narrow scale_range, list fewer sizes, bound max_graphs, or raise interval"
            ) from e
        step._prepare(lr, momentum, weight_decay, grad_scale, self.gradient_clip_val, self.gradient_clip_algorithm, adam)
        if eng.peer is not None:
            eng.peer.check()                  # a failed SyncBN exchange of an earlier replay: raise, do not train on NaN
        out = step._replay()
        self.stepped, self._last = step.stepped, step
        return out

    def flush(self, *args, **kw) -> bool:
        """GraphedTrainStep.flush: close a partial window; nothing when none is open."""
        self.stepped = False
        if self._last is None or self._last.graph is None:        # (no call yet, or the step was evicted with its window closed)
            window = self.eng.accumulation if self.accumulate > 1 else None
            if window is None or not window.flush_needed:
                return False
            self._last = next(reversed(self.steps.values()))
        self.stepped = self._last.flush(*args, **kw)
        return self.stepped
