"""Parameter side of the engine: flat fp32 arenas (masters, gradients x 2, momentum), BatchNorm statistic arenas, the
bf16 MFMA operand packs, the fused SGD and Adam / AdamW steps and the gradient accumulator (accumulate_grad_batches).

Replaces what torch.optim.SGD's foreach kernels and autograd's .grad bookkeeping do for the reference
(kod/nn/optim/smart.py:36-58, kod/lightning/experiments/yv5_baseline/exp.py:156-185): torch Parameters are views of ONE
arena in forward execution order, so gradients complete back-to-front, data-parallel buckets are contiguous slices and
the optimizer is one launch.  Mixed into engine.executor.Engine.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

import torch

from .. import _lib
from .freshness import freshness_key, track_data_edits
from .graph import Graph, head_param


def _pad(n: int, a: int = 64) -> int:
    return (n + a - 1) // a * a


ADAM_HYPER_FLOATS = 32           # the device block of csrc/adam.hip; checked against kodhip_adam_hyper_floats() at allocation


def adam_hyper_values(lr, betas, eps, weight_decay, step: int, grad_scale: float = 1.0, maximize: bool = False,
                      decoupled: bool = False):
    """The Adam hyper block (layout: include/kodhip.h, kodhip_adam_step) as Python doubles; the upload rounds them to fp32.
    lr / eps / weight_decay: 3 values, betas: 3 pairs, for (bias_params, decay_params, norm_params); step: the 1-based
    count of the step that will read the block.  Every constant is formed as torch's single-tensor, non-capturable Adam
    forms it (torch/optim/adam.py): in doubles, from the host's step count."""
    if step < 1:
        raise ValueError(f"adam step {step}: the count of the step about to run, 1-based")
    v = [0.0] * ADAM_HYPER_FLOATS
    for k in range(3):
        l, (b1, b2), e, wd = float(lr[k]), (float(betas[k][0]), float(betas[k][1])), float(eps[k]), float(weight_decay[k])
        bias_correction1 = 1 - b1 ** step
        bias_correction2 = 1 - b2 ** step
        step_size = l / bias_correction1
        v[k], v[3 + k], v[6 + k] = -step_size, b2, 1 - b1
        v[12 + k], v[15 + k], v[18 + k], v[21 + k], v[24 + k] = 1 - b2, bias_correction2 ** 0.5, e, wd, 1 - l * wd
    v[9] = float(grad_scale)
    v[10] = (1.0 if maximize else 0.0) + (2.0 if decoupled else 0.0)
    return tuple(v)


def arena_layout(g: Graph, numel: Dict[str, int]):
    """The flat parameter arena (pure host logic): parameters in forward execution order, each set padded to 64 elements.
    Returns (name -> (offset, numel), optimizer group per 64-element chunk, arena size, offset where each exec unit's
    parameters begin - conv units, then heads)."""
    off = 0
    layout = {}                   # name -> (offset, numel)
    gid = []

    def place(names, group):
        nonlocal off
        start = off
        for n in names:
            layout[n] = (off, numel[n])
            off += numel[n]
        end = _pad(off)
        gid.extend([group] * ((end - start) // 64))
        off = end

    exec_units = [op.unit for op in g.ops if op.kind == "conv"]
    for u in exec_units:
        place([u.name + ".0.weight"], 1)
        place([u.name + ".1.weight"], 2)
        place([u.name + ".1.bias"], 0)
    for h in g.heads:
        place([head_param(h, k, "weight") for k in ("box", "obj", "cls")], 1)
        place([head_param(h, k, "bias") for k in ("box", "obj", "cls")], 0)
    unit_starts = ([layout[u.name + '.0.weight'][0] for u in exec_units]
                   + [layout[head_param(h, 'box', 'weight')][0] for h in g.heads])
    return layout, gid, off, unit_starts


class UnitLayout:
    """Per conv unit, per engine: the unit, its arena / pack offsets (elements), the packs' K paddings, the stride-2 data-
    gradient form.  Written once in _build_arenas; what depends on the input shape is in engine/buffers.py UnitBuffers."""
    __slots__ = ("u", "w_off", "g_off", "b_off", "rs_off", "f_off", "d_off", "Kp", "Kp_f", "Kdp", "s2_fold")


class HeadLayout:
    """Per head, per engine: the head unit, its arena and pack offsets and K paddings (shape side: buffers.HeadBuffers)."""
    __slots__ = ("h", "w_off", "b_off", "f_off", "d_off", "Kp", "Kdp")


class _StagingRing:
    """Pinned staging ring of small host -> device uploads issued outside any captured graph (optimizer hyper-parameters,
    the clip value): the H2D copy is asynchronous, so a slot is not rewritten for the next 15 uploads."""

    def __init__(self, numel: int, slots: int = 16):
        self.host = [torch.zeros(numel, dtype=torch.float32).pin_memory() for _ in range(slots)]
        self.events = [None] * slots
        self.slot = 0

    def upload(self, dst: torch.Tensor, values):
        """dst <- a slot whose first len(values) elements are `values`, on the current stream"""
        k = self.slot
        self.slot = (k + 1) % len(self.host)
        if self.events[k] is not None:          # the DMA that last read this pinned slot must have run
            self.events[k].synchronize()
        host = self.host[k]
        host[:len(values)].copy_(torch.tensor(values, dtype=torch.float32))
        dst.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[k] = ev


class ArenaMixin:
    # ------------------------------------------------------------------ arenas
    def _build_arenas(self, device):
        g = self.g
        self.ulayout: Dict[str, UnitLayout] = {}
        layout, gid, off, self.unit_starts = arena_layout(g, {n: p.numel() for n, p in self.params.items()})
        exec_units = [op.unit for op in g.ops if op.kind == "conv"]
        self.n_arena = off
        self.layout = layout
        self.p_arena = torch.zeros(off, dtype=torch.float32, device=device)
        self.g_arena = [torch.zeros(off, dtype=torch.float32, device=device) for _ in range(2)]
        self.g_cur = 0
        self.m_arena = torch.zeros(off, dtype=torch.float32, device=device)
        self.gid = torch.tensor(gid, dtype=torch.uint8, device=device)
        with torch.no_grad():
            for n, (o, k) in layout.items():
                p = self.params[n]
                self.p_arena[o:o + k].copy_(p.detach().reshape(-1).to(device))
                p.data = self.p_arena[o:o + k].view(p.shape)
                p.grad = None
                track_data_edits(p)
        # BN running statistics arena
        roff = 0
        self.rs_layout = {}
        for u in exec_units:
            self.rs_layout[u.name] = roff
            roff += _pad(u.cout, 16)
        self.rm_arena = torch.zeros(roff, dtype=torch.float32, device=device)
        self.rv_arena = torch.ones(roff, dtype=torch.float32, device=device)
        self.nbt_arena = torch.zeros(len(exec_units), dtype=torch.int64, device=device)
        with torch.no_grad():
            for i, u in enumerate(exec_units):
                o = self.rs_layout[u.name]
                for key, arena in (("running_mean", self.rm_arena), ("running_var", self.rv_arena)):
                    b = self.buffers[f"{u.name}.1.{key}"]
                    arena[o:o + u.cout].copy_(b.to(device))
                    b.data = arena[o:o + u.cout]
                b = self.buffers[f"{u.name}.1.num_batches_tracked"]
                self.nbt_arena[i] = b.to(device)
                b.data = self.nbt_arena[i]
        # what freshness_key() reads: the arenas and every tensor bound into them, held once (engine/freshness.py)
        self._fresh_params = [self.p_arena] + [self.params[n] for n in layout]
        self._fresh_stats = [self.rm_arena, self.rv_arena] + [self.buffers[f"{u.name}.1.{key}"] for u in exec_units
                                                              for key in ("running_mean", "running_var")]
        # weight packs
        descs = []
        foff = doff = 0
        blk = 0
        A, nc = g.num_anchors, g.num_classes

        def add_desc(w_name, f_off, d_off, N, Cin, KH, KW, Kp, Kdp, Ntot, n_off, stem):
            nonlocal blk
            descs.append([layout[w_name][0], f_off, d_off, N, Cin, KH, KW, Kp, Kdp, Ntot, n_off, stem, blk])
            blk += (N * Cin * KH * KW + 255) // 256

        for u in exec_units:
            st = UnitLayout()
            st.u = u
            K = u.k * u.k * u.cin if not u.stem else 144
            st.Kp = _pad(K, 32)                       # K of the weight-gradient slabs (stem: 6x3 taps x 8 = 144 -> 160)
            # forward operand rows: the stem packs each kernel row as one 32-value K step (4 pixel pairs, the 4th
            # zero) so that it runs on the LDS-DMA path like every other layer
            # packed MFMA operands: K axis tap-major, every tap padded to a multiple of 32 channels (csrc/misc_ops.hip)
            st.Kp_f = 6 * 32 if u.stem else u.k * u.k * _pad(u.cin, 32)
            st.Kdp = u.k * u.k * _pad(u.cout, 32)
            st.f_off, st.d_off = foff, (-1 if u.stem else doff)
            foff += u.cout * st.Kp_f
            s2 = (not u.stem) and u.k == 3 and u.s == 2 and u.p == 1
            st.s2_fold = bool(s2 and self.lib.kodhip_conv_dgrad_s2_folded(u.cin, u.cout))
            if s2:       # parity-class packs (1 + 2 + 2 + 4 taps) or the folded pack (4 classes x 4 taps), csrc/conv_igemm.hip
                doff += u.cin * (16 if st.s2_fold else 9) * _pad(u.cout, 32)
            elif not u.stem:
                doff += u.cin * st.Kdp
            st.w_off = layout[u.name + ".0.weight"][0]
            st.g_off = layout[u.name + ".1.weight"][0]
            st.b_off = layout[u.name + ".1.bias"][0]
            st.rs_off = self.rs_layout[u.name]
            if u.stem:
                add_desc(u.name + ".0.weight", st.f_off, -1, u.cout, 3, 6, 6, st.Kp_f, 0, 0, 0, 1)
            else:
                add_desc(u.name + ".0.weight", st.f_off, st.d_off, u.cout, u.cin, u.k, u.k, st.Kp_f, st.Kdp,
                         u.cout, 0, (3 if st.s2_fold else 2) if s2 else 0)
            self.ulayout[u.name] = st
        self.hlayout: Dict[str, HeadLayout] = {}
        self.head_npad = _pad(A * (5 + nc), 8)
        for h in g.heads:
            Kp = _pad(h.cin, 32)
            Kdp = _pad(self.head_npad, 32)
            hs = HeadLayout()
            hs.h, hs.f_off, hs.d_off, hs.Kp, hs.Kdp = h, foff, doff, Kp, Kdp
            hs.w_off = layout[head_param(h, "box", "weight")][0]
            hs.b_off = layout[head_param(h, "box", "bias")][0]
            n_off = 0
            for k, n in (("box", 4 * A), ("obj", A), ("cls", nc * A)):
                add_desc(head_param(h, k, "weight"), foff + n_off * Kp, doff, n, h.cin, 1, 1, Kp, Kdp,
                         self.head_npad, n_off, 0)
                n_off += n
            foff += self.head_npad * Kp
            doff += h.cin * Kdp
            self.hlayout[h.name] = hs
        self.fpack = torch.zeros(foff, dtype=torch.bfloat16, device=device)
        self.dpack = torch.zeros(max(doff, 8), dtype=torch.bfloat16, device=device)
        self.pack_descs = torch.tensor(descs, dtype=torch.int64, device=device)
        assert self.lib.kodhip_pack_desc_bytes() == 13 * 8
        self.pack_blocks = blk
        self.exec_units = exec_units
        self.device = device
        self._plan_static()               # engine/buffers.py: the plans that depend on the graph and the options alone
        self.hyper = torch.zeros(12, dtype=torch.float32, device=device)      # lr[3] | momentum[3] | wd[3] | grad scale | flags | dampening
        self.sgd_nesterov = True          # FusedSGD(nesterov=...): smart_sgd.yaml's default, kod/configs/nn/optimizers/smart_sgd.yaml
        self.sgd_dampening, self.sgd_maximize = 0.0, False      # torch.optim.SGD(dampening=, maximize=) through FusedSGD
        self.sgd_steps = 0                # optimizer steps taken (torch's first step copies the gradient into the momentum buffer)
        self.freeze = None                # engine/freeze.py FreezePlan of the last training forward (None: never read)
        self.keep_mask = None             # u8 per arena element: 0 = frozen (masked SGD), only for a non-default plan
        self.stepped = None               # names with a momentum buffer when not all of them (see note_sgd_step)
        self._freeze_params = None        # parameters in arena order (freeze_flags)
        self._freeze_flags = None
        self._keep_masks = {}             # freeze key -> keep mask
        self._f32_frozen = {}             # freeze key -> F32Plan over the writes backward still issues
        self._stepped_key = None
        self._hyper_args = None
        self._hyper_ring = _StagingRing(12)
        self._hyper_vals = None
        # gradient norm / clipping (csrc/misc_ops.hip, clip block layout in include/kodhip.h): off by default - the step then
        # issues exactly the launches it always did
        self.clip = torch.zeros(self.lib.kodhip_clip_block_bytes() // 4, dtype=torch.float32, device=device)
        self.norm_ws = torch.zeros(self.lib.kodhip_grad_norm_workspace_bytes() // 8, dtype=torch.float64, device=device)
        self.clip_algorithm: Optional[str] = None      # None | "norm" | "value"
        self.clip_skip_nonfinite = False
        self.track_grad_norm = False
        self.norm_nontemporal = False                  # plain loads: the SGD kernel re-reads the arena right after (LOG.md)
        self._count_masks = {}                         # freeze key (None: default plan) -> u8 per element: counts in the norm
        self._unit_hyper = torch.zeros(12, dtype=torch.float32, device=device)
        self._unit_hyper[9] = 1.0                      # grad_scale 1: the norm of .grad as published (clip_grad_norm_)
        self._clip_ring = _StagingRing(4)
        self.clip[8] = float("inf")                    # input slot: max_norm / clamp value (set_clip); inf clips nothing
        self._clip_val = float("inf")
        # Adam / AdamW (csrc/adam.hip): m_arena serves as exp_avg; exp_avg_sq and the hyper block exist once Adam is configured
        # (configure_adam), never for SGD
        self.v_arena = None
        self.adam_hyper = None
        self._adam_ring, self._adam_vals = None, None
        self.adam_steps = 0               # Adam steps taken, as the optimizer counts them (set_adam_hyper)
        self.adam_frozen = None           # frozenset of the names frozen at the first Adam step (they own no state)
        # gradient accumulation (engine/accumulate.py, csrc/accumulate.hip): nothing exists until configure_accumulation(n > 1)
        self.acc_arena = None             # fp32, the gradient arena's layout: the open window's sum
        self.acc_ctl = None               # 4 fp32 on the device; [0] != 0: the next accumulate launch copies (a window's first)
        self._acc_ring, self._acc_first = None, None
        self.accumulation = None          # AccumulationWindow shared by every captured step of this engine
        self._update_from_acc = False     # current_grad_arena() is the accumulator (step_accumulated_device)

    def _grad_view(self, name, arena=None):
        o, k = self.layout[name]
        a = self.g_arena[self.g_cur] if arena is None else arena
        return a[o:o + k].view(self.params[name].shape)

    def pack_weights(self, key=None):
        """key: the caller's reading of freshness_key(), if it has one"""
        _lib.check(self.lib.kodhip_pack_weights(self.p_arena.data_ptr(), self.fpack.data_ptr(),
                                                self.dpack.data_ptr(), self.pack_descs.data_ptr(),
                                                self.pack_descs.shape[0], self.pack_blocks, self._stream()),
                   "pack_weights")
        self._packed_key = (key or self.freshness_key())[0]

    def freshness_key(self):
        """(parameter half, statistics half): moves whenever a parameter / a running statistic may have changed, whoever
        changed it (engine/freshness.py).  The weight packs are keyed on the first half, the eval constants on both."""
        return freshness_key(self.param_version, self.stats_version, self._fresh_params, self._fresh_stats)

    def _publish_grads(self):
        """Expose the arena slices as .grad (accumulating into an existing .grad like autograd would).  Under a freeze plan
        (engine/freeze.py) a frozen tensor keeps .grad = None, as torch leaves it."""
        cur = self.g_arena[self.g_cur]
        other = self.g_arena[self.g_cur ^ 1]
        fz = self.freeze_active()
        names = self.layout if fz is None else fz.trainable
        if not names:                            # (a sub-network with every parameter frozen: only input gradients)
            for n in self.layout:
                self.params[n].grad = None
            self.g_cur ^= 1
            return
        first = next(iter(names))
        existing = self.params[first].grad
        if existing is not None and existing.data_ptr() == self._grad_view(first, other).data_ptr():
            self.wait_grads()
            other.add_(cur)                      # gradient accumulation across backward() calls
            return
        for n in names:
            p = self.params[n]
            if p.grad is not None and p.grad.data_ptr() != self._grad_view(n, cur).data_ptr():
                raise RuntimeError("mixed external .grad tensors are not supported; call zero_grad(set_to_none=True)")
            p.grad = self._grad_view(n, cur)
        if fz is not None:
            for n in fz.frozen:
                self.params[n].grad = None
        self.g_cur ^= 1

    # ------------------------------------------------------------------ freezing (engine/freeze.py)
    def freeze_flags(self):
        """requires_grad of every parameter, in arena order"""
        if self._freeze_params is None:
            self._freeze_params = [self.params[n] for n in self.layout]
        return tuple(p.requires_grad for p in self._freeze_params)

    def sync_freeze(self):
        """Read requires_grad and rebuild the freeze plan when it moved.  Called at every training forward; the common case
        is one tuple of flags compared with the last one."""
        flags = self.freeze_flags()
        if flags == self._freeze_flags:
            return self.freeze
        from .freeze import build_freeze_plan
        plan = build_freeze_plan(self.g, dict(zip(self.layout, flags)))
        if self.freeze is None or self.freeze.key != plan.key:
            self._on_freeze_change(plan)           # (raises on a rank mismatch before the plan is adopted)
        self._freeze_flags, self.freeze = flags, plan
        return plan

    def freeze_active(self):
        """The freeze plan when it differs from the default (everything trainable), else None: the default runs the
        program that has no freeze logic in it."""
        fz = self.freeze
        return None if (fz is None or fz.is_default) else fz

    def _require_same_on_all_ranks(self, key, what):
        """Every rank must run the same program (the same collectives): `key` is compared across the group and a
        mismatch raises on every rank before any collective of the step.  `what`: the error text ("{keys}": what the
        ranks hold)."""
        if not (self.collectives and self.world_size > 1):
            return
        import torch.distributed as dist
        keys = [None] * self.world_size
        dist.all_gather_object(keys, key, group=self.process_group)
        if any(k != key for k in keys):
            raise RuntimeError(what.format(keys=keys))

    def _on_freeze_change(self, plan):
        # the freeze set is compared across the group whenever it changes - so every rank changes it at the same step, as
        # a training script does
        self._require_same_on_all_ranks(plan.key, "the ranks disagree on which parameters are frozen (requires_grad): "
                                        "every rank must freeze the same set")
        if plan.is_default:
            self.keep_mask = None
            return
        # one mask per freeze set, kept for the engine's lifetime: a captured step bakes the mask's address in
        keep = self._keep_masks.get(plan.key)
        if keep is None:
            keep = torch.ones(self.n_arena, dtype=torch.uint8, device=self.device)
            for n in plan.frozen:
                o, k = self.layout[n]
                keep[o:o + k] = 0
            self._keep_masks[plan.key] = keep
        self.keep_mask = keep

    # ------------------------------------------------------------------ BatchNorm modes (engine/bn_mode.py)
    def bn_mode_flags(self):
        """`training` of every conv unit's BatchNorm module, in program order (None: no modules registered)"""
        mods = self.bn_modules
        return None if mods is None else tuple(m.training for m in mods)

    def sync_bn_mode(self):
        """Read the BatchNorm modules' modes and rebuild the mode plan when they moved.  Called at every training forward;
        the common case is one tuple of flags compared with the last one."""
        flags = self.bn_mode_flags()
        if self.bn_mode is not None and flags == self._bn_mode_flags:
            return self.bn_mode
        from .bn_mode import build_bn_mode_plan
        names = [u.name for u in self.exec_units]
        plan = build_bn_mode_plan(self.g, dict(zip(names, flags)) if flags is not None else {})
        if self.bn_mode is None or self.bn_mode.key != plan.key:
            self._on_bn_mode_change(plan)          # (raises on a rank mismatch before the plan is adopted)
        self._bn_mode_flags, self.bn_mode = flags, plan
        return plan

    def bn_mode_active(self):
        """The mode plan when some unit is in eval mode, else None: the default runs the program without eval units."""
        mp = self.bn_mode
        return None if (mp is None or mp.is_default) else mp

    def _on_bn_mode_change(self, plan):
        # (eval units leave the SyncBN exchanges): compared across the group whenever the eval set changes, so a mismatch
        # raises on every rank before any exchange
        self._require_same_on_all_ranks(plan.key, "the ranks disagree on which BatchNorm modules are in eval mode: every "
                                        "rank must put the same modules in eval mode")
        if not plan.is_default and plan.key not in self._nbt_inc:
            self._nbt_inc[plan.key] = torch.tensor(plan.train_mask(), dtype=torch.int64, device=self.device)

    def current_grad_arena(self):
        """Arena holding the gradients published by the last backward() - the gradient operand of every update launch (norm,
        SGD forms, Adam).  While a closed accumulation window is being consumed (step_accumulated_device) that operand is the
        accumulator."""
        if self._update_from_acc:
            return self.acc_arena
        return self.g_arena[self.g_cur ^ 1]

    # ------------------------------------------------------------------ gradient accumulation
    def configure_accumulation(self, n: int):
        """accumulate_grad_batches = n for the captured steps of this engine.  n > 1 allocates, once: the accumulator (the
        parameter arena's size), the 4-float control block with its staging ring, and the window.  n == 1 allocates nothing."""
        from .accumulate import AccumulationWindow, check_accumulate_grad_batches
        n = check_accumulate_grad_batches(n)
        if n == 1:
            return None
        if self.acc_arena is None:
            self.acc_arena = torch.zeros(self.n_arena, dtype=torch.float32, device=self.device)
            self.acc_ctl = torch.zeros(4, dtype=torch.float32, device=self.device)
            self._acc_ring = _StagingRing(4)
        if self.accumulation is None:
            self.accumulation = AccumulationWindow(n)
        elif self.accumulation.n != n:
            if self.accumulation.flush_needed:
                raise RuntimeError(f"accumulate_grad_batches changed from {self.accumulation.n} to {n} inside an open window: "
                                   "flush() first")
            self.accumulation = AccumulationWindow(n)
        return self.accumulation

    def set_accumulate_first(self, first: bool):
        """Upload the control block's flag when it changed - outside any captured graph, like set_hyper."""
        first = bool(first)
        if first != self._acc_first:
            self._acc_ring.upload(self.acc_ctl, (1.0 if first else 0.0, 0.0, 0.0, 0.0))
            self._acc_first = first

    def accumulate_grads_device(self):
        """acc_arena <- (copy of | acc_arena +) the gradients of the last backward(), as acc_ctl says: ONE launch - the
        graph-capturable form, after wait_grads() (data parallel: what is accumulated is the all-reduced gradient)."""
        self.wait_grads()
        _lib.check(self.lib.kodhip_grad_accumulate(self.acc_arena.data_ptr(), self.current_grad_arena().data_ptr(), self.n_arena,
                                                   2, self.acc_ctl.data_ptr(), self._stream()), "grad_accumulate")

    def step_accumulated_device(self, optimizer: str = "sgd"):
        """sgd_step_device() / adam_step_device() on the accumulator: the update that closes a window."""
        if self.acc_arena is None:
            raise RuntimeError("step_accumulated_device() before configure_accumulation(n > 1)")
        self._update_from_acc = True
        try:
            self.adam_step_device() if optimizer == "adam" else self.sgd_step_device()
        finally:
            self._update_from_acc = False

    # ------------------------------------------------------------------ optimizer
    def set_hyper(self, lr, momentum, weight_decay, grad_scale: float = 1.0):
        """Upload the optimizer hyper-parameters (3-tuples for bias_params, decay_params, norm_params) to the device
        buffer the fused SGD kernel reads - outside any captured graph, so schedules keep working under replay."""
        self._hyper_args = (tuple(lr), tuple(momentum), tuple(weight_decay), grad_scale)
        first = self.sgd_dampening != 0.0 and self.sgd_steps == 0
        flags = (1.0 if self.sgd_nesterov else 0.0) + (2.0 if self.sgd_maximize else 0.0) + (4.0 if first else 0.0)
        vals = (*lr, *momentum, *weight_decay, grad_scale, flags, float(self.sgd_dampening))
        if vals != self._hyper_vals:                       # only touch the device copy when the schedule moved
            self._hyper_ring.upload(self.hyper, vals)
            self._hyper_vals = vals

    def sgd_step(self, lr, momentum, weight_decay, grad_scale: float = 1.0):
        """lr / momentum / weight_decay: 3-tuples for (bias_params, decay_params, norm_params)."""
        self.wait_grads()
        self.set_hyper(lr, momentum, weight_decay, grad_scale)
        self.sgd_step_device()

    # ------------------------------------------------------------------ gradient norm / clipping
    CLIP_MODES = {"norm": 0, "value": 1}

    def configure_clip(self, algorithm: Optional[str] = None, skip_nonfinite: bool = False, track_grad_norm: bool = False):
        """Which launches sgd_step_device() issues: algorithm None = no clipping.  The clip VALUE lives in device memory
        (set_clip); this choice is baked into a captured step."""
        if algorithm is not None and algorithm not in self.CLIP_MODES:
            raise ValueError(f"gradient_clip_algorithm {algorithm!r}: expected 'norm' or 'value'")
        self.clip_algorithm, self.clip_skip_nonfinite = algorithm, bool(skip_nonfinite)
        self.track_grad_norm = bool(track_grad_norm)

    def set_clip(self, value: Optional[float]):
        """Upload max_norm (algorithm "norm") or the clamp value ("value") into the clip block's input slot - outside any
        captured graph, like set_hyper.  None = +inf: nothing is clipped (skip_nonfinite without a clip value)."""
        v = float("inf") if value is None else float(value)
        if v != self._clip_val:
            self._clip_ring.upload(self.clip[8:12], (v,))
            self._clip_val = v

    def _count_mask(self):
        """u8 per arena element: 1 where the element belongs to a trainable tensor.  The 64-element padding behind a
        parameter set carries the set's group id and the head tensors share granules, so the norm masks per element
        instead of trusting every writer of both gradient arenas to leave the padding zero.  One mask per freeze set, kept
        for the engine's lifetime (a captured step bakes its address in)."""
        fz = self.freeze_active()
        key = None if fz is None else fz.key
        m = self._count_masks.get(key)
        if m is None:
            host = np.zeros(self.n_arena, dtype=np.uint8)
            for n in (self.layout if fz is None else fz.trainable):
                o, k = self.layout[n]
                host[o:o + k] = 1
            m = torch.from_numpy(host).to(self.device)
            self._count_masks[key] = m
        return m

    def grad_norm_device(self, hyper=None):
        """Launch the norm reduction over the current gradient arena (two launches); the results land in self.clip."""
        h = self.hyper if hyper is None else hyper
        _lib.check(self.lib.kodhip_grad_norm(self.current_grad_arena().data_ptr(), self.gid.data_ptr(),
                                             self._count_mask().data_ptr(), self.n_arena, h.data_ptr(), self.clip.data_ptr(),
                                             self.norm_ws.data_ptr(), int(self.clip_skip_nonfinite and hyper is None),
                                             int(self.norm_nontemporal), self._stream()), "grad_norm")

    def clip_grads_inplace(self, algorithm: str, value: float):
        """torch.nn.utils.clip_grad_norm_ / clip_grad_value_ over the published .grad views (eager path): the norm of the
        gradients as they stand (no grad_scale), then g *= coef (or the clamp) in place.  Returns the total norm as a device
        scalar for "norm", None for "value"."""
        mode = self.CLIP_MODES[algorithm]
        self.wait_grads()
        self.set_clip(value)
        if mode == 0:
            self.grad_norm_device(self._unit_hyper)
        _lib.check(self.lib.kodhip_grad_clip_inplace(self.current_grad_arena().data_ptr(), self.gid.data_ptr(),
                                                     self._count_mask().data_ptr(), self.n_arena, self.clip.data_ptr(),
                                                     mode, self._stream()), "grad_clip_inplace")
        return self.clip[0].clone() if mode == 0 else None

    def sgd_step_device(self):
        """SGD with whatever is in self.hyper (device, 12 floats) - the graph-capturable form.  With clipping configured
        (configure_clip): norm reduction (after wait_grads(), so every rank reduces the same all-reduced gradients and forms
        the same coefficient without a collective of its own), then the SGD form that consumes it."""
        algo, skip = self.clip_algorithm, self.clip_skip_nonfinite
        if algo is not None or skip or self.track_grad_norm:
            if algo != "value" or skip or self.track_grad_norm:
                self.grad_norm_device()
            if algo is not None or skip:
                fz = self.freeze_active()
                _lib.check(self.lib.kodhip_sgd_nesterov_clipped(
                    self.p_arena.data_ptr(), self.current_grad_arena().data_ptr(), self.m_arena.data_ptr(),
                    self.gid.data_ptr(), None if fz is None else self.keep_mask.data_ptr(), self.n_arena,
                    self.hyper.data_ptr(), self.clip.data_ptr(), self.CLIP_MODES[algo or "norm"], int(skip),
                    self._stream()), "sgd_clipped")
                self.param_version += 1
                self.note_sgd_step()
                return
        if self.freeze_active() is None:
            _lib.check(self.lib.kodhip_sgd_nesterov(self.p_arena.data_ptr(), self.current_grad_arena().data_ptr(),
                                                    self.m_arena.data_ptr(), self.gid.data_ptr(), self.n_arena,
                                                    self.hyper.data_ptr(), self._stream()), "sgd")
        else:       # frozen tensors: no weight decay, no momentum, no update (torch.optim.SGD skips p.grad is None)
            _lib.check(self.lib.kodhip_sgd_nesterov_masked(self.p_arena.data_ptr(), self.current_grad_arena().data_ptr(),
                                                           self.m_arena.data_ptr(), self.gid.data_ptr(),
                                                           self.keep_mask.data_ptr(), self.n_arena,
                                                           self.hyper.data_ptr(), self._stream()), "sgd_masked")
        self.param_version += 1
        self.note_sgd_step()

    # ------------------------------------------------------------------ Adam / AdamW
    def configure_adam(self):
        """Allocate what Adam needs beside the SGD arenas, once: exp_avg_sq (the parameter arena's size) and the hyper block
        with its staging ring.  exp_avg is m_arena."""
        if self.v_arena is None:
            n = self.lib.kodhip_adam_hyper_floats()
            if n != ADAM_HYPER_FLOATS:
                raise RuntimeError(f"libkodhip's Adam hyper block has {n} floats, the host lays out {ADAM_HYPER_FLOATS}")
            self.v_arena = torch.zeros(self.n_arena, dtype=torch.float32, device=self.device)
            self.adam_hyper = torch.zeros(n, dtype=torch.float32, device=self.device)
            self._adam_ring = _StagingRing(n)

    def set_adam_hyper(self, lr, betas, eps, weight_decay, step: int, grad_scale: float = 1.0, maximize: bool = False,
                       decoupled: bool = False):
        """Upload the Adam hyper block (adam_hyper_values) - outside any captured graph, like set_hyper.  step: the 1-based
        count of the step about to run; the bias corrections are host values, so a replayed graph needs a new block before
        every replay."""
        self.configure_adam()
        vals = adam_hyper_values(lr, betas, eps, weight_decay, step, grad_scale, maximize, decoupled)
        self.adam_steps = int(step) - 1
        if vals != self._adam_vals:
            self._adam_ring.upload(self.adam_hyper, vals)
            self._adam_vals = vals

    def adam_step(self, lr, betas, eps, weight_decay, step: int, grad_scale: float = 1.0, maximize: bool = False,
                  decoupled: bool = False):
        """The eager route: wait for the gradients, upload the block, launch."""
        self.wait_grads()
        self.set_adam_hyper(lr, betas, eps, weight_decay, step, grad_scale, maximize, decoupled)
        self.adam_step_device()

    def _frozen_now(self):
        fz = self.freeze_active()
        return frozenset() if fz is None else frozenset(fz.frozen)

    def check_adam_freeze(self):
        """One host step count serves every tensor, so the freeze set is fixed by the first Adam step: a tensor that joins or
        leaves later would need a count of its own (torch keeps one per tensor)."""
        if self.adam_steps > 0 and self.adam_frozen is not None and self._frozen_now() != self.adam_frozen:
            raise RuntimeError("the freeze set (requires_grad) changed after the first Adam step: the fused Adam keeps one step "
                               "count for all tensors, so the set of frozen parameters must stay what it was at the first step "
                               "(frozen from the start is supported); build a new optimizer to change it")

    def adam_step_device(self):
        """Adam / AdamW with whatever is in self.adam_hyper (device) - the graph-capturable form, with the same launches in
        front as sgd_step_device(): the norm reduction when clipping by norm or tracking the norm, then ONE kodhip_adam_step
        that consumes the clip block.  skip_nonfinite is refused: a step skipped on the device would not hold the host's step
        count back."""
        if self.clip_skip_nonfinite:
            raise ValueError("skip_nonfinite with Adam is not supported: the bias corrections come from the host's step count, "
                             "which a step skipped on the device would not hold back")
        if self.v_arena is None:
            raise RuntimeError("adam_step_device() before set_adam_hyper()")
        self.check_adam_freeze()
        algo = self.clip_algorithm
        if algo == "norm" or self.track_grad_norm:
            self.grad_norm_device(self.adam_hyper)
        fz = self.freeze_active()
        _lib.check(self.lib.kodhip_adam_step(
            self.p_arena.data_ptr(), self.current_grad_arena().data_ptr(), self.m_arena.data_ptr(), self.v_arena.data_ptr(),
            self.gid.data_ptr(), None if fz is None else self.keep_mask.data_ptr(), self.n_arena, self.adam_hyper.data_ptr(),
            None if algo is None else self.clip.data_ptr(), -1 if algo is None else self.CLIP_MODES[algo], self._stream()),
            "adam_step")
        self.param_version += 1
        self.note_adam_step()

    def note_adam_step(self):
        """one Adam step has run (eagerly, or inside a replayed graph)"""
        if self.adam_steps == 0:
            self.adam_frozen = self._frozen_now()
        self.adam_steps += 1

    def note_sgd_step(self):
        """one optimizer step has run (eagerly, or inside a replayed graph): with dampening the first step's flag must leave
        the device block before the next one"""
        self.sgd_steps += 1
        # which tensors own a momentum buffer (torch's optimizer state has one only for tensors stepped at least once):
        # None = all of them
        fz = self.freeze_active()
        if fz is None:
            self.stepped, self._stepped_key = None, None
        elif fz.key != self._stepped_key:
            self._stepped_key = fz.key
            if self.sgd_steps == 1 or self.stepped is not None:
                self.stepped = (self.stepped or set()) | set(fz.trainable)
        if self.sgd_dampening != 0.0 and self.sgd_steps == 1 and self._hyper_args is not None:
            self.set_hyper(*self._hyper_args)

    def mark_params_changed(self):
        self.param_version += 1

    def invalidate_eval_constants(self):
        """Call after anything the version counters cannot see changed parameters or running statistics - i.e. a
        replay of a user-captured hipGraph that contains a training forward or an optimizer step (GraphedTrainStep
        does it itself)."""
        self.param_version += 1
        self.stats_version += 1
