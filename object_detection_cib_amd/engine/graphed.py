"""GraphedTrainStep - one training step (forward, assigner + loss, backward, gradient all-reduce, fused SGD) captured
once as a hipGraph and replayed on new data.

The reference leaves launch scheduling to PyTorch / Lightning (one aten kernel at a time from Python).  Here the
step is ~520 launches of 5-100 us; issued from Python it is host-bound, so the capture is what makes a training LOOP
run at device speed (bench.py measures exactly this replay).  What makes the step capturable:

* inputs live in static device buffers that new batches are copied into: the image batch, and the boxes / labels /
  image indices of all targets padded to a fixed capacity with zero-size boxes, which the assigner never matches
  (kod/core/label_assignment/yv5.py:262-296: the anchor-ratio test rejects w = h = 0);
* optimizer hyper-parameters are read from device memory (Engine.set_hyper), so warm-up / LR schedules keep working;
  so is the gradient-clipping value (Engine.set_clip): the norm reduction and the clipped SGD run inside the graph;
* no host synchronisation anywhere in the step (assigner counts stay on the device).

accumulate_grad_batches = N > 1 (engine/accumulate.py): the captured step ends with one kodhip_grad_accumulate launch instead of
the update - a device flag, uploaded outside the graph, says whether it opens a window - and the update runs eagerly behind the
replay that closes a window.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional, Sequence

import torch

from .. import _lib
from ..core.label_assignment.yv5 import BatchedTargets
from ..core.types import FeatureShape


_KEEP = object()          # __call__(gradient_clip_val=...) left out: keep the current value


class TargetBlock:
    """The targets of one batch padded to a fixed capacity: boxes f64 [cap, 4] | labels i64 [cap] | sample ids i32 [cap] as
    views of ONE device block, and the ring of pinned host mirrors it is filled from.  Padding rows are zero-size boxes,
    which the assigner never matches.  GraphedTrainStep owns one; the captured steps of a MultiScaleTrainStep share one."""

    def __init__(self, max_targets: int, device, lib):
        # a batch's targets arrive as one host -> device copy of the pinned mirror block (three copies + three fills cost
        # 0.17 ms per step)
        self.cap, self.lib = int(max_targets), lib
        cap = self.cap
        tbytes = (cap * 44 + 15) // 16 * 16            # (kodhip_pull_from_host moves 16-byte pieces)
        self.block = torch.zeros(tbytes, dtype=torch.uint8, device=device)
        self.boxes = self.block[:cap * 32].view(torch.float64).view(cap, 4)
        self.labels = self.block[cap * 32:cap * 40].view(torch.int64)
        self.samples = self.block[cap * 40:cap * 44].view(torch.int32)
        self.targets = BatchedTargets(self.boxes, self.labels, self.samples, self.cap)
        self._host = []
        for _ in range(4):
            blk = torch.zeros(tbytes, dtype=torch.uint8).pin_memory()
            self._host.append((blk, blk[:cap * 32].view(torch.float64).view(cap, 4), blk[cap * 32:cap * 40].view(torch.int64),
                               blk[cap * 40:cap * 44].view(torch.int32)))
        self._events, self._slot, self._used = [None] * 4, 0, [0] * 4

    def load(self, targets) -> int:
        """Fill the device block from a batch's targets; -> the number of boxes (a host value in every form)."""
        if isinstance(targets, BatchedTargets):
            n = targets.n
            if n > self.cap:
                raise ValueError(f"{n} target boxes in the batch exceed the graph's capacity {self.cap}")
            self.boxes.zero_(); self.labels.zero_(); self.samples.zero_()      # padding = zero-size boxes: never assigned
            if n:
                self.boxes[:n].copy_(targets.boxes)
                self.labels[:n].copy_(targets.labels)
                self.samples[:n].copy_(targets.samples)
            return n
        # host-side targets (tuple of DetectionTarget on the CPU, or the flat arrays of data.device_pipeline.PackedTargets):
        # pack them into one pinned block and upload it without stalling the host behind the previous step (a pageable
        # copy would)
        packed = hasattr(targets, "samples") and hasattr(targets, "counts")
        lens = None if packed else [int(t.boxes.shape[0]) for t in targets]
        n = int(len(targets.labels)) if packed else sum(lens)
        if n > self.cap:
            raise ValueError(f"{n} target boxes in the batch exceed the graph's capacity {self.cap}")
        k = self._slot
        self._slot = (self._slot + 1) % len(self._host)
        if self._events[k] is not None:
            self._events[k].synchronize()
        blk, hb, hl, hs = self._host[k]
        m_old = self._used[k]                  # padding = zero-size boxes: only what the slot's previous batch filled needs clearing
        if m_old > n:
            hb[n:m_old].zero_(); hl[n:m_old].zero_(); hs[n:m_old].zero_()
        self._used[k] = n
        if packed:
            if n:
                hb.numpy()[:n] = targets.boxes
                hl.numpy()[:n] = targets.labels
                hs.numpy()[:n] = targets.samples
            targets = ()
        o = 0
        for i, t in enumerate(targets):
            m = lens[i]
            if m:
                hb[o:o + m] = t.boxes.reshape(-1, 4).to(torch.float64)
                hl[o:o + m] = t.labels.reshape(-1).to(torch.int64)
                hs[o:o + m] = i
                o += m
        _lib.check(self.lib.kodhip_pull_from_host(self.block.data_ptr(), blk.data_ptr(), blk.numel(),
                                                  torch.cuda.current_stream().cuda_stream), "pull_from_host")
        ev = torch.cuda.Event()
        ev.record()
        self._events[k] = ev
        return n


class GraphedTrainStep:
    def __init__(self, net, loss, batch_size: int, height: int, width: int, max_targets: int = 4096,
                 loss_scale: Optional[float] = None, input_pairs: bool = False,
                 gradient_clip_val: Optional[float] = None, gradient_clip_algorithm: str = "norm",
                 skip_nonfinite: bool = False, track_grad_norm: bool = False, target_block: Optional["TargetBlock"] = None,
                 optimizer: str = "sgd", accumulate_grad_batches: int = 1):
        """input_pairs: batches arrive as bf16 pixel pairs [B, H, W/2, 8] (DeviceTrainPipeline.make_batch(out_pairs=True)) and
        are copied straight into the network's input buffer - no fp32 NCHW batch, no layout-change pass in the step.
        gradient_clip_val / gradient_clip_algorithm ("norm" | "value"): Lightning's Trainer arguments; the clipping runs
        between the gradient all-reduce and the update inside the captured step (the value may change per call, the
        algorithm and on / off may not).  skip_nonfinite: a step whose gradient norm is NaN / Inf leaves parameters and
        momentum untouched and is counted in `skipped_steps`.  track_grad_norm: run the norm reduction without clipping.
        `grad_norm` (total, bias, decay, norm-group norms before clipping) and `skipped_steps` are static device tensors:
        reading them is the caller's synchronisation, the step has none.  target_block: a TargetBlock to read the targets from
        instead of one of its own (MultiScaleTrainStep: one block for the steps of all its sizes).
        optimizer: "sgd" (default) | "adam" - which fused update the captured step ends with (Engine.sgd_step_device /
        adam_step_device, the latter for Adam and AdamW); baked in at capture() and guarded like the clip configuration.
        With "adam", __call__ takes `adam=FusedAdam.hyper()` in place of (lr, momentum, weight_decay): the bias corrections
        are host values formed from the step count, so EVERY call must bring the hyper of its step.  skip_nonfinite is
        refused with "adam" (a skipped device step would not hold the host's count back), so is capture(preserve_state=False)
        (its warm-up steps would move the moments without the count).
        accumulate_grad_batches = N (Lightning's Trainer argument; engine/accumulate.py): with N > 1 the captured step ends with
        ONE kodhip_grad_accumulate launch in place of the update, `loss_scale` defaults to B / N, and the call that closes a
        window of N micro-batches launches norm / clip / update eagerly behind its replay, on the same stream, reading the
        accumulator.  `stepped` says whether the last call updated; flush() closes a partial window (an epoch's end).  The
        window lives in the engine, N is baked in at capture().  N = 1 is the step without any of this."""
        from .accumulate import check_accumulate_grad_batches
        self.accumulate, self._accumulate = check_accumulate_grad_batches(accumulate_grad_batches), None
        self.stepped = False              # the last call (or flush()) ran the optimizer update
        if gradient_clip_algorithm not in ("norm", "value"):
            raise ValueError(f"gradient_clip_algorithm {gradient_clip_algorithm!r}: expected 'norm' or 'value'")
        if optimizer not in ("sgd", "adam"):
            raise ValueError(f"optimizer {optimizer!r}: expected 'sgd' or 'adam'")
        if optimizer == "adam" and skip_nonfinite:
            raise ValueError("skip_nonfinite with optimizer='adam' is not supported: the bias corrections come from the host's "
                             "step count, which a step skipped on the device would not hold back")
        self.optimizer, self._optimizer = optimizer, None      # (_optimizer: what capture() baked in)
        self.gradient_clip_val = None if gradient_clip_val is None else float(gradient_clip_val)
        self.gradient_clip_algorithm = gradient_clip_algorithm
        self.skip_nonfinite, self.track_grad_norm = bool(skip_nonfinite), bool(track_grad_norm)
        self._clip_cfg = None             # what capture() baked in
        self.net, self.loss = net, loss
        self.input_pairs = bool(input_pairs)
        self.eng = net.engine()
        dev = self.eng.device
        self.B, self.H, self.W = batch_size, height, width
        self.cap = int(max_targets)
        # exp.py:104-138: total = B * sum; under accumulation Lightning's loss / N, formed as one double: B / N
        self.scale = float(batch_size / self.accumulate if loss_scale is None else loss_scale)
        self.x = torch.zeros((batch_size, 3, height, width), dtype=torch.float32, device=dev)
        # boxes f64 [cap, 4] | labels i64 [cap] | sample ids i32 [cap] as views of ONE device block (TargetBlock)
        self._tb = target_block if target_block is not None else TargetBlock(max_targets, dev, self.eng.lib)
        assert self._tb.cap == self.cap
        self._tblock, self.boxes, self.labels, self.samples = self._tb.block, self._tb.boxes, self._tb.labels, self._tb.samples
        self.targets = self._tb.targets
        self.shape = FeatureShape(width=width, height=height)
        self.params = list(net.parameters())
        self.graph = None
        self._freeze_flags, self._keep_mask = None, None
        self._bn_flags = None
        self.total = None
        self.parts = None
        self._last_adam = None            # the hyper the last call brought (flush() without one)
        self._pins = 0                    # pins capture() took on this shape, given back by release()

    def input_buffer(self) -> torch.Tensor:
        """input_pairs=True: the network's own input buffer (bf16 pixel pairs [B, H, W/2, 8]).  A data pipeline that runs on
        the step's stream may write the next batch straight into it (DeviceTrainPipeline.compose_host_batch(pairs_out=...))
        and pass the same tensor to __call__: no copy between pipeline and step."""
        assert self.input_pairs
        return self.eng.image_buffer(self.B, self.H, self.W)

    @property
    def grad_norm(self) -> torch.Tensor:
        """[total, bias, decay, norm] gradient norms of the last step, before clipping (device, static)"""
        return self.eng.clip[0:4]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """steps skipped for a NaN / Inf gradient norm so far (device scalar, static)"""
        return self.eng.clip[6]

    def _clip_config(self):
        return (self.gradient_clip_algorithm if self.gradient_clip_val is not None else None, self.skip_nonfinite,
                self.track_grad_norm)

    # -- the step itself (what gets captured)
    def _step(self):
        for p in self.params:
            p.grad = None
        if self.accumulate > 1:
            # the weight packs are made inside the step (Engine.forward, when the key moved).  The plain step moves the key
            # itself with its update; this one must hold the pack launch too, for the replay behind an eager update
            self.eng.mark_params_changed()
        total, lr = self.net.train_step(self.x, self.loss, self.shape, self.targets, self.scale, image_ready=self.input_pairs)
        self.eng.wait_grads()
        if self.accumulate > 1:           # the update runs behind the replay that closes the window (_close)
            self.eng.accumulate_grads_device()
        else:
            self._update(False)
        return total, (lr.localization.detach(), lr.objectness.detach(), lr.classification.detach())

    def _update(self, accumulated: bool):
        """norm / clip / update launches on the current stream: inside the captured step, or behind a closing replay"""
        self.eng.configure_clip(*self._clip_config())
        if accumulated:
            self.eng.step_accumulated_device(self.optimizer)
        elif self.optimizer == "adam":
            self.eng.adam_step_device()
        else:
            self.eng.sgd_step_device()

    def _load(self, images: torch.Tensor, targets):
        if self.input_pairs:
            buf = self.eng.image_buffer(self.B, self.H, self.W)
            assert tuple(images.shape) == tuple(buf.shape) and images.dtype == buf.dtype, (images.shape, images.dtype, buf.shape)
            if images.data_ptr() != buf.data_ptr():        # (a pipeline may composite straight into the input buffer: input_buffer())
                buf.copy_(images, non_blocking=True)
        else:
            assert tuple(images.shape) == tuple(self.x.shape), (images.shape, self.x.shape)
            self.x.copy_(images, non_blocking=True)
        if targets is not None:            # (None: a MultiScaleTrainStep has filled the shared block already)
            self._tb.load(targets)

    def capture(self, images: torch.Tensor, targets, warmup: int = 2, preserve_state: bool = True, adam: Optional[dict] = None):
        """Runs `warmup` eager steps on this batch (allocations, lazy initialisation), then captures the step.
        preserve_state: parameters, momentum (with optimizer="adam": both moments) and BatchNorm buffers are restored
        afterwards, so that capturing does not move the training trajectory.
        adam (optimizer="adam"): the hyper the warm-up steps run with; left out, they run with the block the engine holds, or,
        when it holds none yet, with a neutral one (lr 0)."""
        eng = self.eng
        if self.optimizer == "adam":
            if not preserve_state:
                raise ValueError("capture(preserve_state=False) with optimizer='adam': the warm-up steps would move the moments "
                                 "without the host's step count")
            if adam is not None:
                eng.set_adam_hyper(**adam)
            elif eng.v_arena is None:
                eng.set_adam_hyper([0.0] * 3, [(0.9, 0.999)] * 3, [1e-8] * 3, [0.0] * 3, step=1)
        eng.pin_shape(self.B, self.H, self.W)      # the graph bakes this shape's buffer addresses in (Engine.allocate)
        self._pins += 1
        self._load(images, targets)
        self._clip_cfg = self._clip_config()
        self._optimizer = self.optimizer
        self._accumulate = self.accumulate
        window = eng.configure_accumulation(self.accumulate)
        eng.set_clip(self.gradient_clip_val)
        state = (eng.p_arena, eng.m_arena, eng.rm_arena, eng.rv_arena, eng.nbt_arena, eng.clip)     # (clip: the skipped-steps count)
        adam_steps = eng.adam_steps
        if self.optimizer == "adam":
            state = state + (eng.v_arena,)
        if window is not None:            # the warm-up steps accumulate: an open window (a size first met inside one) survives
            state = state + (eng.acc_arena, eng.acc_ctl)
            pos = window.pos
            if eng._acc_first is None:
                eng.set_accumulate_first(window.first)
        keep = [t.clone() for t in state] if preserve_state else None
        side = torch.cuda.Stream(device=eng.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(warmup, 2)):
                self._step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        # the freeze set the graph's backward program and masked SGD were captured for (the mask stays alive with it)
        self._freeze_flags, self._keep_mask = eng.freeze_flags(), eng.keep_mask
        # and the BatchNorm modes it was captured with (eval units: constants from running statistics, no statistics stage)
        self._bn_flags = eng.bn_mode_flags()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.total, self.parts = self._step()
        if keep is not None:
            for t, k in zip(state, keep):
                t.copy_(k)
            eng.mark_params_changed()
        eng.adam_steps = adam_steps               # (the warm-up steps are not steps of the trajectory)
        if window is not None:
            if keep is not None:
                window.pos = pos
            else:
                window.reset()
        return self

    def __call__(self, images: torch.Tensor, targets, lr: Optional[Sequence[float]] = None,
                 momentum: Optional[Sequence[float]] = None, weight_decay: Optional[Sequence[float]] = None,
                 grad_scale: float = 1.0, gradient_clip_val=_KEEP, gradient_clip_algorithm: Optional[str] = None,
                 adam: Optional[dict] = None):
        """One replayed step on a new batch.  Returns (total, (box, obj, cls)) - static tensors that the next call
        overwrites (clone to keep).  gradient_clip_val: a new max_norm / clamp value from this step on.
        optimizer="adam": `adam=FusedAdam.hyper()` (Engine.set_adam_hyper's keywords: lr, betas, eps, weight_decay per group,
        step, maximize, decoupled) takes the place of lr / momentum / weight_decay and is required at every call; grad_scale
        applies as for SGD."""
        self._prepare(lr, momentum, weight_decay, grad_scale, gradient_clip_val, gradient_clip_algorithm, adam)
        if self.eng.peer is not None:
            self.eng.peer.check()             # a failed SyncBN exchange of an earlier replay: raise, do not train on NaN
        self._load(images, targets)
        return self._replay()

    def flush(self, lr: Optional[Sequence[float]] = None, momentum: Optional[Sequence[float]] = None,
              weight_decay: Optional[Sequence[float]] = None, grad_scale: float = 1.0, gradient_clip_val=_KEEP,
              adam: Optional[dict] = None) -> bool:
        """Close a partial window (the last batch of an epoch came before N micro-batches were in): the update on what has
        been accumulated, with the hyper-parameters given here or, left out, the ones the last call brought.  Does nothing -
        no launch, no upload - when no window is open.  Returns `stepped`."""
        self.stepped = False
        window = self.eng.accumulation if self.accumulate > 1 else None
        if window is None or not window.flush_needed:
            return False
        if adam is None and self.optimizer == "adam":
            adam, grad_scale = self._last_adam          # (the block the last call uploaded, its grad_scale included)
        self._prepare(lr, momentum, weight_decay, grad_scale, gradient_clip_val, None, adam)
        self._close(window)
        return True

    def _close(self, window):
        """the per-window work behind the replay (or flush) that closes it"""
        self._update(True)                    # (param_version, note_sgd_step / note_adam_step: the update launchers' own)
        window.reset()
        self.stepped = True

    def release(self):
        """Drop the captured graph and give back the pins capture() took on the shape (Engine.unpin_shape): the buffer set
        becomes an ordinary one that the engine may drop.  The caller makes sure that no replay is still running; a later
        capture() captures again."""
        self.graph, self.total, self.parts = None, None, None
        while self._pins:
            self.eng.unpin_shape(self.B, self.H, self.W)
            self._pins -= 1

    def _guard(self, freeze_flags, bn_flags, clip_cfg):
        """what the graph was captured with against what holds now (MultiScaleTrainStep checks every held step per call)"""
        window = self.eng.accumulation
        now = self.accumulate if (self.accumulate == 1 or window is None or self.accumulate != self._accumulate) else window.n
        if now != self._accumulate:
            # the graph ends with the accumulate launch (N > 1) or the update (N = 1), and its loss scale is B / N; the
            # window the engine holds must be the one it was captured for
            raise RuntimeError(f"accumulate_grad_batches changed to {now} after capture() with {self._accumulate}: the captured "
                               "step holds the old launches and loss scale; build a new GraphedTrainStep and capture() again")
        if self.optimizer != self._optimizer:
            # the graph ends with the update launch of the optimizer it was captured with
            raise RuntimeError(f"optimizer changed to {self.optimizer!r} after capture() with {self._optimizer!r}: the captured "
                               "step holds the old update launch; build a new GraphedTrainStep and capture() again")
        if freeze_flags != self._freeze_flags:
            # the graph replays the backward program of the freeze set it was captured with
            raise RuntimeError("requires_grad changed after capture(): the captured step would train the old freeze set; "
                               "build a new GraphedTrainStep and capture() again")
        if bn_flags != self._bn_flags:
            # the graph replays the forward / backward program of the BatchNorm modes it was captured with
            raise RuntimeError("a BatchNorm module changed mode (train / eval) after capture(): the captured step would "
                               "normalise with the old modes; build a new GraphedTrainStep and capture() again")
        if clip_cfg != self._clip_cfg:
            # the graph replays the launches of the clipping mode it was captured with; only the value is device data
            raise RuntimeError("the gradient clipping algorithm (or clipping on / off, skip_nonfinite, track_grad_norm) changed "
                               "after capture(): the captured step holds the old launches; build a new GraphedTrainStep and "
                               "capture() again (gradient_clip_val itself may change per step)")

    def _prepare(self, lr, momentum, weight_decay, grad_scale, gradient_clip_val, gradient_clip_algorithm, adam=None):
        """everything of a call before the batch is loaded: the guards, the clip value and the hyper-parameters"""
        if self.graph is None:
            raise RuntimeError("call capture() first")
        if gradient_clip_val is not _KEEP:
            self.gradient_clip_val = None if gradient_clip_val is None else float(gradient_clip_val)
        if gradient_clip_algorithm is not None:
            self.gradient_clip_algorithm = gradient_clip_algorithm
        self._guard(self.eng.freeze_flags(), self.eng.bn_mode_flags(), self._clip_config())
        self.eng.set_clip(self.gradient_clip_val)
        if self.optimizer == "adam":
            if adam is None or lr is not None:
                raise ValueError("optimizer='adam': pass adam=FusedAdam.hyper() at every call (the bias corrections of the step "
                                 "are host values), not lr / momentum / weight_decay")
            self._last_adam = (dict(adam), grad_scale)
            self.eng.set_adam_hyper(**adam, grad_scale=grad_scale)
            self.eng.check_adam_freeze()
        elif adam is not None:
            raise ValueError("adam=... needs GraphedTrainStep(optimizer='adam')")
        elif lr is not None:
            self.eng.set_hyper(lr, momentum, weight_decay, grad_scale)

    def _replay(self):
        if self.accumulate > 1:
            eng = self.eng
            window = eng.accumulation
            eng.set_accumulate_first(window.first)
            self.graph.replay()
            # the replay moved running statistics and no parameter: the eval constants (keyed on both halves of
            # freshness_key) are rebuilt, the weight packs (parameter half) are not
            eng.stats_version += 1
            self.stepped = False
            if window.advance():
                self._close(window)
            return self.total, self.parts
        self.graph.replay()
        self.eng.param_version += 1           # the replayed update changed the parameters
        if self.optimizer == "adam":
            self.eng.note_adam_step()
        else:
            self.eng.note_sgd_step()
        self.stepped = True
        return self.total, self.parts


class _GraphedEval:
    """What the captured eval forwards share: the static fp32 input batch, the eager refresh of weight packs and eval-mode
    BatchNorm constants before a replay when parameters / running statistics moved (both live in buffers with fixed
    addresses, so the same graph serves every validation epoch), the `eval_fused` guard and the capture itself.  A
    subclass says which engine shapes its launches touch (`_shapes`) and what is captured (`_forward`)."""

    def __init__(self, net, anchor_info, batch_size: int, height: int, width: int):
        self.net, self.anchor_info = net, anchor_info
        self.eng = net.engine()
        self.x = torch.zeros((batch_size, 3, height, width), dtype=torch.float32, device=self.eng.device)
        self.shape = FeatureShape(width=width, height=height)
        self.graph, self.det = None, None
        self._eval_fused = None           # EngineOptions.eval_fused the graph was captured with
        self._held = []                   # the shapes capture() pinned, until release()

    def release(self):
        """Drop the captured graph and give back its pins (Engine.unpin_shape): the buffer sets become ordinary ones that
        the engine may drop.  The caller makes sure that no replay is still running (GraphCache synchronises the stream);
        a later call captures again."""
        self.graph, self.det = None, None
        for shp in self._held:
            self.eng.unpin_shape(*shp)
        self._held = []

    def _shapes(self):
        """the (B, H, W) buffer sets the graph bakes addresses of"""
        return [(self.x.shape[0], self.x.shape[2], self.x.shape[3])]

    def _forward(self):
        raise NotImplementedError

    def _refresh(self):
        eng = self.eng
        key = eng.freshness_key()
        if eng._packed_key != key[0]:
            eng.pack_weights(key)
        eng._eval_affine_ptrs(key)

    @torch.no_grad()
    def capture(self, images: torch.Tensor):
        eng = self.eng
        if not self._held:                # (a second capture() of the same object keeps its pins)
            for shp in self._shapes():
                eng.pin_shape(*shp)
                self._held.append(shp)
        self.x.copy_(images)
        side = torch.cuda.Stream(device=eng.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._forward()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._refresh()
        self._eval_fused = bool(eng.opt.eval_fused)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.det = self._forward()
        return self

    @torch.no_grad()
    def __call__(self, images: torch.Tensor) -> torch.Tensor:
        """Decoded detections [B, rows, 5 + nc] of a new batch (a static tensor the next call overwrites)."""
        if self.graph is None:
            self.capture(images)
        assert tuple(images.shape) == tuple(self.x.shape), (images.shape, self.x.shape)
        if bool(self.eng.opt.eval_fused) != self._eval_fused:
            # the graph replays the launches of the form it was captured with (one fused launch per unit, or conv + apply)
            raise RuntimeError("EngineOptions.eval_fused changed after capture(): the captured forward holds the old launches; "
                               f"build a new {type(self).__name__} and capture() again")
        self._refresh()
        self.x.copy_(images, non_blocking=True)
        # a replay needs its shapes' buffer sets to be what the graph captured - they are pinned, nothing to swap
        self.graph.replay()
        return self.det


class GraphedEvalForward(_GraphedEval):
    """Eval-mode forward + prediction decode captured once per input shape and replayed (validation loop).

    Issued one launch at a time from Python the eval forward is host-bound like the training step (~230 launches,
    ~15 ms of ctypes / Python per batch against ~7 ms of GPU time); replaying a hipGraph leaves the host only the copy
    of the batch into the static input buffer.  Weight packs and the eval-mode BatchNorm constants are refreshed
    eagerly before a replay when parameters / running statistics moved (both live in buffers with fixed addresses), so
    the same graph serves every validation epoch."""

    def __init__(self, net, anchor_info, batch_size: int, height: int, width: int):
        from ..lightning.experiments.yv5_baseline.layers import get_detections
        super().__init__(net, anchor_info, batch_size, height, width)
        self._decode = get_detections

    def _forward(self):
        from ..nn.networks.yolov5 import Yolov5NetworkResult
        from ..nn.heads.types import DetectionHeadResult
        raws = self.eng.forward(self.x, training=False)
        res = Yolov5NetworkResult(*[DetectionHeadResult(t[..., 0:4], t[..., 4:5], t[..., 5:]) for t in raws])
        return self._decode(self.shape, res, self.anchor_info)


class GraphedAugmentedForward(_GraphedEval):
    """The test-time-augmented eval forward (layers.get_detections_augmented: three views, three forwards, one merged
    decoded tensor) captured as ONE hipGraph and replayed.  All launches of the three views sit on one stream in one
    linear chain - view, forward, decode, next view: the eval forward uses no side stream, so the graph has no parallel
    branch - and the buffer sets of all the views' shapes are pinned, as the graph bakes their addresses in."""

    def __init__(self, net, anchor_info, batch_size: int, height: int, width: int):
        from ..lightning.experiments.yv5_baseline.layers import get_detections_augmented
        from .tta import tta_plan
        super().__init__(net, anchor_info, batch_size, height, width)
        self._augmented, self.plan = get_detections_augmented, tta_plan(height, width)

    def _shapes(self):
        return [(self.x.shape[0], hp, wp) for hp, wp in self.plan.shapes()]

    def _forward(self):
        return self._augmented(self.x, self.net, self.anchor_info)


class GraphCache(OrderedDict):
    """input shape (B, 3, H, W) -> captured eval forward, least recently used first, at most `max_graphs` of them.

    A front end that sees changing input shapes (rectangular inference: one canvas per batch) would otherwise keep a graph,
    a static input batch, a static output and up to three pinned engine buffer sets per shape for its lifetime.  `forward`
    returns the shape's graph, building it when it is new; beyond `max_graphs` the least recently used one goes first: the
    current stream is synchronised (its last replay and whatever read its output have finished), the graph is dropped and
    its shapes are unpinned (`_GraphedEval.release`; pins are counted, so a shape that a training step or another graph
    also holds stays pinned).  The trade-off: a shape that comes back after its eviction pays a buffer-set allocation and
    a capture again, so `max_graphs` should cover the shapes of one pass over the data where memory allows."""

    def __init__(self, max_graphs: int = 8):
        super().__init__()
        self.max_graphs = 1
        self.resize(max_graphs)

    def resize(self, max_graphs: int):
        """a new bound; graphs beyond it go now, least recently used first"""
        if int(max_graphs) < 1:
            raise ValueError(f"max_graphs {max_graphs}: expected >= 1")
        self.max_graphs = int(max_graphs)
        self._evict(self.max_graphs)

    def _evict(self, keep: int):
        while len(self) > keep:
            _, old = self.popitem(last=False)
            torch.cuda.current_stream().synchronize()
            old.release()

    def forward(self, key, build):
        """the graph of input shape `key`, now the most recently used; `build()` makes a missing one"""
        g = self.get(key)
        if g is not None:
            self.move_to_end(key)
            return g
        self._evict(self.max_graphs - 1)
        g = self[key] = build()
        return g
