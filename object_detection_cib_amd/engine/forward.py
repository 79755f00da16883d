"""Forward launch program: walks the static op list (engine/graph.py) and enqueues libkodhip kernels on the caller's
stream (+ side streams for the CSP short_conv branches and the P3 / P4 heads).

Replaces what aten does for the reference's `net(images)` (kod/nn/networks/yolov5.py:90-108): conv -> train-mode
BatchNorm -> SiLU units, torch.cat / nn.Upsample as channel-slice writes, the three fused heads.  ForwardMixin is mixed
into Engine; the state of one pass lives in a _ForwardPass, never on the engine (engine/backward.py _BackwardPass is its pair).
"""
from __future__ import annotations

import torch

from .. import _lib
from .graph import ConvUnit, Op, View

chk = _lib.check

BN_EPS, BN_MOMENTUM = 1e-3, 0.03        # kod/nn/networks/yolov5.py:24


class _ForwardPass:
    """One forward() call over the engine's current buffer set: what the launches share (streams, base pointers, the mode
    of the call and its BatchNorm mode plan) and the pass's mutable state (the pending side branch, the head-source
    events, the pool counter, the caller's hook)."""

    def __init__(self, eng, training: bool, after_first_layer):
        self.eng, self.lib, self.bs = eng, eng.lib, eng.cur
        self.B, self.H, self.W = self.bs.shape
        self.training, self.after_first_layer = training, after_first_layer
        self.s = eng._stream()           # the stream the unit stages launch on (side_branch switches it)
        self.fp, self.pa = eng.fpack.data_ptr(), eng.p_arena.data_ptr()
        self.rm, self.rv = eng.rm_arena.data_ptr(), eng.rv_arena.data_ptr()
        self.eval_aff = None if training else eng._eval_affine_ptrs(eng._fresh)
        self.sync = sync = training and eng.sync_bn and eng.collectives
        if sync:
            eng._check_equal_local_batch(self.bs.shape)
        # BatchNorm mode plan (engine/bn_mode.py), None when every unit is in train mode: then this is the program
        # without eval units.  With one: the eval units' constants come from one launch before the first conv, and they
        # have no statistics stage (no running-statistic update, no SyncBN exchange)
        mp = eng.sync_bn_mode() if training else None
        self.mp = None if (mp is None or mp.is_default) else mp
        # eval forward only, read per call (the option may be toggled on a live engine).  A training forward never fuses,
        # eval UNITS of a training network included: their backward needs the saved pre-BN tensor
        self.fused = (not training) and eng.opt.eval_fused
        # A CSP layer's short_conv (conv -> statistics -> apply) depends only on the layer input and is needed only by
        # last_conv: it runs on a side stream next to main_conv and the blocks, where it fills the chip while the main
        # branch sits in a single-block statistics kernel or a latency-bound deep layer.  (Not under SyncBN - the two
        # statistic exchanges travel as one grouped collective on the main stream - and not while timing families.)
        self.main = torch.cuda.current_stream()
        if sync and eng.peer is not None:
            eng.peer.step_begin(self.s)        # the step's sequence number: tags every statistic this rank publishes
        # (with the peer exchange there is no communicator whose call order the side streams could disturb)
        self.branch = training and (not sync or eng.peer is not None) and eng.branch_overlap and eng.profile is None
        self.joined_buf = None           # concat buffer whose short_conv half is being written on the side stream
        # the P3 / P4 head convolutions are leaves (only the loss reads them): they run on their own side stream as soon
        # as their input exists, beside the bottom-up path, instead of after it.  head_src: buffer -> "ready" event
        heads_aside = training and eng.branch_overlap and eng.profile is None          # (also under SyncBN: no collective involved)
        self.head_src = {op.src.buf.name: None for op in eng.g.ops[:-1] if op.kind == "head"} if heads_aside else {}
        self.heads_on_aux, self.pool_i, self.outs = False, 0, []

    # ------------------------------------------------------------------ the stages of a conv unit
    def conv_stage(self, u: ConvUnit):
        eng, st = self.eng, self.bs.units[u.name]
        e0 = eng._t0()
        chk(self.lib.kodhip_conv_fwd_raw(eng._ptr(u.src), self.fp + 2 * st.lay.f_off, st.raw.data_ptr(),
                                         st.stats.data_ptr(), *st.geo_fwd(), st.raw_ld, 0, self.s), u.name)
        eng._t1(e0, "conv_fwd", st.conv_bytes(), name=u.name)

    def fused_stage(self, u: ConvUnit):
        """eval forward with EngineOptions.eval_fused: conv + BatchNorm (running statistics) + activation (+ residual)
        as ONE launch from u.src to u.dst - no pre-BN tensor (st.raw), no statistics, no apply pass"""
        eng, st = self.eng, self.bs.units[u.name]
        res = u.residual
        e0 = eng._t0()
        chk(self.lib.kodhip_conv_fwd_fused(eng._ptr(u.src), self.fp + 2 * st.lay.f_off, *self.eval_aff[u.name],
                                           eng._ptr(res) if res else None, res.buf.C if res else 0, res.coff if res else 0,
                                           eng._ptr(u.dst), *st.geo_fwd(), u.dst.buf.C, u.dst.coff, eng.act_kind,
                                           eng.act_slope, self.s), u.name)
        eng._t1(e0, "conv_fwd_fused", st.conv_bytes() + (2 * st.M * u.cout if res else 0), name=u.name)

    def finalize_args(self, u: ConvUnit, ranks: int):
        """the finalize kernels' common arguments: (element count over `ranks`, gamma, beta, running mean / variance,
        momentum, eps, scale | shift | mean | rstd of st.aff, channels, update the running statistics)"""
        eng, st, C_ = self.eng, self.bs.units[u.name], u.cout
        lay, pa, aff = st.lay, self.pa, st.aff.data_ptr()
        return (float(st.M) * ranks, pa + 4 * lay.g_off, pa + 4 * lay.b_off, self.rm + 4 * lay.rs_off, self.rv + 4 * lay.rs_off,
                eng.bn_momentum, eng.bn_eps, aff, aff + 4 * C_, aff + 8 * C_, aff + 12 * C_, C_, 1)

    def stats_stage(self, group):
        """Batch statistics -> BatchNorm constants.  Under SyncBN the [sum, sum of squares] vectors of the group's
        units (a CSP layer's main + short convs) are exchanged as ONE grouped collective."""
        eng, lib, units, s = self.eng, self.lib, self.bs.units, self.s
        if self.mp is not None:
            group = self.mp.stat_group(group)
            if not group:
                return
        e0 = eng._t0()
        if not self.sync:
            for u in group:
                st = units[u.name]
                chk(lib.kodhip_bn_finalize_partials(st.stats.data_ptr(), st.T, *self.finalize_args(u, 1), s), u.name)
        elif eng.peer is not None:
            # SyncBN over peer buffers: the same single launch per unit, the ranks' sums meet inside the kernel
            for u in group:
                st = units[u.name]
                chk(lib.kodhip_bn_finalize_partials_peer(st.stats.data_ptr(), st.T, *self.finalize_args(u, eng.world_size),
                                                         eng.peer.view_ptr(), eng.peer_slots[(u.name, "f")], s), u.name)
        else:
            for u in group:
                st = units[u.name]
                chk(lib.kodhip_bn_reduce_partials(st.stats.data_ptr(), st.sums.data_ptr(), u.cout, st.T, s), u.name)
            eng._allreduce_group([units[u.name].sums for u in group])
            for u in group:
                chk(lib.kodhip_bn_finalize(units[u.name].sums.data_ptr(), *self.finalize_args(u, eng.world_size), s), u.name)
        eng._t1(e0, "bn_finalize", sum(8.0 * u.cout * units[u.name].T for u in group), name="+".join(u.name for u in group))

    def apply_stage(self, u: ConvUnit):
        eng, st, C_ = self.eng, self.bs.units[u.name], u.cout
        aff = st.aff.data_ptr()
        sc_p, sh_p = (aff, aff + 4 * C_) if self.training else self.eval_aff[u.name]
        res = u.residual
        e0 = eng._t0()
        chk(self.lib.kodhip_bn_act_apply(st.raw.data_ptr(), st.raw_ld, sc_p, sh_p,
                                         eng._ptr(res) if res else None, res.buf.C if res else 0, res.coff if res else 0,
                                         eng._ptr(u.dst), u.dst.buf.C, u.dst.coff, st.M, C_, eng.act_kind, eng.act_slope,
                                         self.s), u.name)
        eng._t1(e0, "bn_silu_apply", (6.0 if res else 4.0) * st.M * C_, name=u.name)

    # ------------------------------------------------------------------ the program
    def run(self):
        ops = self.eng.g.ops
        if self.mp is not None:         # the eval units' BatchNorm constants of a training forward: one launch before the first conv
            eng, mp = self.eng, self.mp
            table, n_ev = eng._bn_eval_table(mp)
            e0 = eng._t0()
            chk(self.lib.kodhip_bn_eval_constants(table.data_ptr(), n_ev, eng.bn_eps, self.s), "bn_eval_constants")
            eng._t1(e0, "bn_eval_constants", 8.0 * sum(u.cout for u in eng.exec_units if mp.is_eval(u.name)), name="eval_units")
        i = 0
        while i < len(ops):
            op = ops[i]
            i += 1
            if op.kind == "conv":
                u = op.unit
                # a CSP main_conv's sibling (its short_conv: same input) is the next op of the program
                sib = ops[i].unit if (u.sibling is not None and i < len(ops) and ops[i].unit is u.sibling) else None
                i += self.conv(u, sib, first=(i == 1))
            else:
                getattr(self, op.kind)(op)           # pool | up | head
        if self.after_first_layer is not None:
            self.after_first_layer()
        if self.joined_buf is not None:
            self.main.wait_stream(self.eng.br_stream)
        if self.heads_on_aux:
            self.main.wait_stream(self.eng.head_stream)
        return self.outs

    def conv(self, u: ConvUnit, sib, first: bool) -> int:
        """One conv op of the program; `sib`: the unit's sibling when it is the next op.  Returns how many further ops it
        took along (the sibling, in the side-branch and the grouped-exchange schedules)."""
        if self.joined_buf is not None and u.src.buf.name == self.joined_buf:
            self.main.wait_stream(self.eng.br_stream)
            self.joined_buf = None
        if self.branch and sib is not None and self.joined_buf is None:
            self.side_branch(u, sib)
            return 1
        if u.dst.buf.name in self.head_src and not (self.branch and u.sibling is not None):
            self.head_source(u)
            return 0
        if self.after_first_layer is not None and not first:
            self.after_first_layer()
            self.after_first_layer = None
        if self.fused:
            self.fused_stage(u)
            return 0
        # SyncBN over RCCL: a unit and its sibling (same input, next in the program) share one statistic exchange
        group = [u, sib] if (self.sync and self.eng.peer is None and sib is not None) else [u]
        self.unit_group(group)
        return len(group) - 1

    def side_branch(self, u: ConvUnit, short: ConvUnit):
        """a CSP layer's main_conv on the main stream and its short_conv on the side stream"""
        eng = self.eng
        if eng.br_stream is None:
            eng.br_stream = torch.cuda.Stream(device=eng.device)
        # the fork's dependency is taken here, the side branch is CAPTURED after the main branch's kernels: the
        # graph executor keeps a node's first captured successor on its queue (see backward())
        fork = torch.cuda.Event()
        fork.record(self.main)
        self.unit_group([u])
        eng.br_stream.wait_event(fork)
        self.s = eng.br_stream.cuda_stream
        self.unit_group([short])
        self.s = self.main.cuda_stream
        self.joined_buf = short.dst.buf.name

    def head_source(self, u: ConvUnit):
        """a unit whose output a side-stream head reads: the head waits for the event recorded behind it"""
        self.unit_group([u])
        ev = torch.cuda.Event()
        ev.record(self.main)
        self.head_src[u.dst.buf.name] = ev

    def unit_group(self, group):
        """conv -> statistics (one exchange for the whole group) -> apply of one unit or a sibling pair, on self.s"""
        for u in group:
            self.conv_stage(u)
        if self.training:
            self.stats_stage(group)
        for u in group:
            self.apply_stage(u)

    def pool(self, op: Op):
        eng = self.eng
        h, w = self.H // op.src.stride, self.W // op.src.stride
        chk(self.lib.kodhip_maxpool_fwd(eng._ptr(op.src), op.src.buf.C, op.src.coff, eng._ptr(op.dst),
                                        op.dst.buf.C, op.dst.coff, self.bs.pool_idx[self.pool_i].data_ptr(),
                                        self.B, h, w, op.src.C, op.k, self.s), "maxpool")
        self.pool_i += 1

    def up(self, op: Op):
        eng = self.eng
        h, w = self.H // op.src.stride, self.W // op.src.stride
        chk(self.lib.kodhip_upsample2x_fwd(eng._ptr(op.src), op.src.buf.C, op.src.coff, eng._ptr(op.dst),
                                           op.dst.buf.C, op.dst.coff, self.B, h, w, op.src.C, self.s), "upsample")

    def head(self, op: Op):
        eng, hu, hs = self.eng, op.unit, self.bs.heads[op.unit.name]
        A, nc = eng.g.num_anchors, eng.g.num_classes
        out = torch.empty((self.B, A, hs.H, hs.W, 5 + nc), dtype=torch.float32, device=eng.device)
        hstream = self.s
        ev = self.head_src.get(hu.src.buf.name)
        if ev is not None:
            if eng.head_stream is None:
                eng.head_stream = torch.cuda.Stream(device=eng.device)
            eng.head_stream.wait_event(ev)
            hstream, self.heads_on_aux = eng.head_stream.cuda_stream, True
        chk(self.lib.kodhip_conv_fwd_head(eng._ptr(hu.src), self.fp + 2 * hs.lay.f_off, self.pa + 4 * hs.lay.b_off,
                                          out.data_ptr(), self.B, hs.H, hs.W, hu.src.buf.C, hu.src.coff,
                                          hu.cin, A, nc, hs.lay.Kp, hstream), hu.name)
        self.outs.append(out)


class ForwardMixin:
    # ------------------------------------------------------------------ helpers
    def _ptr(self, v: View, grad=False):
        return (self.cur.gact if grad else self.cur.act)[v.buf.name].data_ptr()

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    # -- per-family kernel timing (bench.py's roofline table): HIP events around every launch of an eager step, recorded
    #    on the stream the launch goes to.  self.profile = [] switches it on; entries (family, e0, e1, algorithmic bytes).
    def _t0(self, stream=None):
        if self.profile is None:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream) if stream is not None else e.record()
        return e

    def _t1(self, e0, family: str, nbytes: float, stream=None, name: str = ""):
        if e0 is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(stream) if stream is not None else e1.record()
        self.profile.append((family, e0, e1, nbytes, name))          # name: the unit(s) the launch belongs to (tools/layer_table.py)

    def _stamp(self, name: str, stream=None):
        """(debug) device time stamp `name` on `stream` (a torch stream; default: the current one)"""
        if not self.stamps_on:
            return
        if self.stamp_buf is None:
            assert torch.device(self.device).type == "cuda"
            self.stamp_buf = torch.zeros(1024, dtype=torch.int64, device=self.device)
        assert self.stamp_buf.is_cuda and len(self.stamp_names) < 1000
        if name not in self.stamp_names:
            self.stamp_names.append(name)
        i = self.stamp_names.index(name)
        sid = stream.cuda_stream if stream is not None else self._stream()
        _lib.check(self.lib.kodhip_debug_stamp(self.stamp_buf.data_ptr() + 8 * i, sid), "stamp")

    def _allreduce_group(self, tensors, outs=None):
        """In-place (or, with `outs`, out-of-place) sum all-reduce of several small tensors as ONE collective launch
        (ncclGroupStart / End) on the native communicator; one call each on a torch.distributed group."""
        if not self.collectives:
            return
        if self.comm is not None:
            if len(tensors) == 1:
                self.comm.all_reduce(tensors[0]) if outs is None else self.comm.all_reduce_to(tensors[0], outs[0])
                return
            with self.comm.group():
                for k, t in enumerate(tensors):
                    self.comm.all_reduce(t) if outs is None else self.comm.all_reduce_to(t, outs[k])
        else:
            for k, t in enumerate(tensors):
                if outs is not None:
                    outs[k].copy_(t)
                    t = outs[k]
                torch.distributed.all_reduce(t, group=self.process_group)

    def image_buffer(self, B: int, H: int, W: int) -> torch.Tensor:
        """The network's input buffer for this shape: bf16 pixel pairs [B, H, W/2, 8] (channels r, g, b, 0 of two
        neighbouring pixels).  Fill it and call forward(..., image_ready=True)."""
        assert not self.g.inputs
        self.allocate(B, H, W)
        return self.cur.act["image"]

    # ------------------------------------------------------------------ forward
    def forward(self, x, training: bool = True, after_first_layer=None, image_ready: bool = False):
        """Whole network / backbone: x = [B,3,H,W] fp32 NCHW on this device.  Sub-network graphs (Graph.inputs): x = a
        sequence of NCHW tensors, one per input view (copied into the channels-last bf16 buffers; torch does the layout
        change, the arithmetic stays in libkodhip).  Returns the head tensors [B,A,h,w,5+nc] fp32 (ll, ml, hl) followed
        by the Graph.outputs views as NCHW fp32 tensors.
        after_first_layer: called once after the first layer's kernels are launched (a hook for side-stream work that only
        depends on the step's inputs: it is then captured behind the forward chain's head, see Yolov5Network.train_step).
        image_ready: the caller has already put the batch into the engine's own input buffer (`image_buffer()`: bf16 pixel
        pairs [B, H, W/2, 8], what kodhip_nchw_to_nhwc4 produces and kodhip_compose_batch can write directly) - x then only
        carries the shape, and the layout-change pass is skipped (the training loop of bench.py / DeviceTrainPipeline)."""
        if self.g.inputs:
            xs = list(x)
            assert len(xs) == len(self.g.inputs)
            v0 = self.g.inputs[0]
            B, H, W = xs[0].shape[0], xs[0].shape[2] * v0.stride, xs[0].shape[3] * v0.stride
            self.allocate(B, H, W)
            for v, t in zip(self.g.inputs, xs):
                assert tuple(t.shape) == (B, v.C, H // v.stride, W // v.stride) and t.device == self.device, (t.shape, v.C, v.stride)
                self.cur.act[v.buf.name][..., v.coff:v.coff + v.C].copy_(t.permute(0, 2, 3, 1))
        else:
            B, Cimg, H, W = x.shape
            assert Cimg == 3 and x.dtype == torch.float32 and x.is_contiguous() and x.device == self.device
            self.allocate(B, H, W)
        self._fresh = self.freshness_key()      # read once per forward; the eval constants below use the same reading
        if self._packed_key != self._fresh[0]:
            # (round 6: the re-pack on a side stream beside the input's layout change measured 1.3 % SLOWER in the replayed
            # step - a second root node moves the forward chain's head to another hardware queue; LOG round 6)
            self.pack_weights(self._fresh)
        if not self.g.inputs and not image_ready:
            chk(self.lib.kodhip_nchw_to_nhwc4(x.data_ptr(), self.cur.act["image"].data_ptr(), B, 3, H, W, self._stream()),
                "nchw_to_nhwc4")
        self._stamp("fwd_begin")
        fwd = _ForwardPass(self, training, after_first_layer)
        outs = fwd.run()
        self._stamp("fwd_end")
        mp = fwd.mp
        if training and mp is None:
            self.nbt_arena += 1
            self.stats_version += 1              # running statistics moved
        elif training:
            self.nbt_arena += self._nbt_inc[mp.key]         # train-mode units only
            if mp.any_train:
                self.stats_version += 1
        self.training_ready = training          # an eval forward overwrites the saved pre-BN tensors
        for v in self.g.outputs:                # sub-network graphs: their output views, NCHW fp32
            outs.append(self.cur.act[v.buf.name][..., v.coff:v.coff + v.C].permute(0, 3, 1, 2).float())
        return outs

    def _bn_eval_table(self, mp):
        """(device descriptor table, unit count) of the forward's kodhip_bn_eval_constants launch for the current buffer
        set.  One table per eval set and buffer set, kept for the engine's lifetime: a captured step bakes its address in."""
        from .bn_mode import eval_constant_units
        units = eval_constant_units(mp, self.freeze_active())
        sts = self.cur.units
        ptrs = tuple((sts[n].aff.data_ptr(), sts[n].coef.data_ptr() if c else 0) for n, c in units)
        key = (mp.key, ptrs)
        t = self._bn_eval_tables.get(key)
        if t is None:
            assert self.lib.kodhip_bn_eval_desc_bytes() == 8 * 8
            pa, rm, rv = self.p_arena.data_ptr(), self.rm_arena.data_ptr(), self.rv_arena.data_ptr()
            rows = []
            for (n, _), (aff, coef) in zip(units, ptrs):
                lay = self.ulayout[n]
                rows.append([pa + 4 * lay.g_off, pa + 4 * lay.b_off, rm + 4 * lay.rs_off, rv + 4 * lay.rs_off, aff, coef,
                             lay.u.cout, 0])
            t = torch.tensor(rows, dtype=torch.int64).to(self.device)
            self._bn_eval_tables[key] = t
        return t, len(units)

    def _eval_affine_ptrs(self, key=None):
        """Eval-mode BatchNorm constants of every unit (scale = gamma * rsqrt(running_var + eps), shift = beta -
        running_mean * scale) in ONE flat buffer, recomputed with five whole-network tensor ops only when parameters or
        running statistics changed - not per layer per forward (a validation epoch forwards many batches with frozen
        weights).  Kept apart from the training constants (st.aff), so an eval forward never disturbs a pending backward.
        Returns {unit name: (scale ptr, shift ptr)}."""
        # keyed on the version counters of the arenas and of every tensor bound into them too (engine/freshness.py): in-place
        # edits that bypass the engine - EMA swap, reset_running_stats, nn.init, a non-fused optimizer (a user-captured graph
        # replay bumps nothing - see invalidate_eval_constants).  key: the caller's reading of freshness_key(), if it has one
        if key is None:
            key = self.freshness_key()
        if self._eval_aff is None:
            gi, bi, ri, off = [], [], [], 0
            self._eval_off = {}
            for u in self.exec_units:
                st = self.ulayout[u.name]
                ar = torch.arange(u.cout)
                gi.append(st.g_off + ar); bi.append(st.b_off + ar); ri.append(st.rs_off + ar)
                self._eval_off[u.name] = off
                off += u.cout
            dev = self.device
            self._eval_idx = tuple(torch.cat(t).to(dev) for t in (gi, bi, ri))
            self._eval_n = off
            self._eval_aff = torch.empty(2 * off, dtype=torch.float32, device=dev)
            self._eval_key = None
        if self._eval_key != key:
            gi, bi, ri = self._eval_idx
            n = self._eval_n
            sc = self.p_arena[gi] * torch.rsqrt(self.rv_arena[ri] + self.bn_eps)
            self._eval_aff[:n] = sc
            self._eval_aff[n:] = self.p_arena[bi] - self.rm_arena[ri] * sc
            self._eval_key = key
        base, n = self._eval_aff.data_ptr(), self._eval_n
        return {name: (base + 4 * o, base + 4 * (n + o)) for name, o in self._eval_off.items()}
