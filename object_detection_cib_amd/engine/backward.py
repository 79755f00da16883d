"""Backward launch program: the forward op list in reverse - BatchNorm/SiLU backward, data gradients on the main
stream, weight gradients (+ gradient buckets) on a side stream, captured so that the critical chain stays on one
queue of the replayed hipGraph.

Replaces autograd's traversal for the reference's `total.backward()` (kod/lightning/experiments/yv5_baseline/
exp.py:104-138) and torch DDP's reducer hooks (kod/configs/trainer/ddp.yaml:4-9).  BackwardMixin is mixed into Engine;
the state of one pass lives in a _BackwardPass, never on the engine.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import torch

from .. import _lib
from .graph import HeadUnit, View, head_param
from .ddp import plan_buckets, launch_bucket
from .freeze import trainable_span, group_launches, UnitLaunch
from .bn_mode import coef_launches

chk = _lib.check


class _BackwardPass:
    """One backward() call over the engine's current buffer set: what the launches share (streams, base pointers, the
    active plans) and the pass's mutable state (first-writer bookkeeping, deferred weight gradients, due gradient buckets)."""

    def __init__(self, eng, head_grads: List[torch.Tensor]):
        self.eng, self.lib, self.head_grads = eng, eng.lib, head_grads
        self.bs = bs = eng.cur
        self.B, self.H, self.W = bs.shape
        self.s = eng._stream()
        self.ga = eng.g_arena[eng.g_cur]
        self.gp = self.ga.data_ptr()
        self.dp = eng.dpack.data_ptr()
        self.pa = eng.p_arena.data_ptr()
        self.wgp = bs.wg_part.data_ptr()
        self.touched = set()            # grad buffers already holding a (partial) sum
        # freeze plan (engine/freeze.py), None when everything is trainable: then this is the program without any freeze
        # logic.  With one: nothing for units in the no-grad region, no data gradient that no trainable tensor needs,
        # no weight gradient of a frozen weight
        self.fz = fz = eng.freeze_active()
        if fz is not None:
            fz.require_trainable()
        # Weight gradients run on a side stream: dW of a layer is off the critical path (bn-bwd -> dgrad -> next
        # layer), so it fills the tails of the small kernels on the main stream and, under SyncBN, the latency of
        # the per-layer statistic all-reduce.  All wgrads share one stream (and the split-K scratch) => ordered.
        self.main = torch.cuda.current_stream()
        self.wg = None
        if eng.wgrad_overlap:
            if eng.wg_stream is None:
                eng.wg_stream = torch.cuda.Stream(device=eng.device)
            self.wg = eng.wg_stream
        # How a weight gradient joins the side stream matters in the captured graph: this stack's graph executor keeps a
        # node's FIRST captured successor on the node's queue and hands the later ones to other queues (~11 us per
        # hand-over).  So a weight gradient takes its dependency where dY is ready (an event right after
        # bn_silu_bwd_apply / head_bwd_prep - it then runs beside the same unit's data gradient, both reading dY) but
        # is launched, i.e. captured, only after the main stream's next kernel (the data gradient): the critical chain
        # apply -> dgrad -> next unit's coefficients -> ... stays on one queue and only the off-path weight gradients
        # pay the hand-over.
        self.deferred = []              # [(event, name, nbytes, args)]
        self.fork_ev = None             # the pending fork event (fork_point -> timed_wgrad)
        # a short_conv whose weight gradient waits for its main_conv's dual launch: no gradient bucket may be enqueued meanwhile
        self.hold = False
        # gradient buffers last written on a side stream (the P3 / P4 heads' data gradients): buffer -> event the main
        # stream must wait for before it reads or accumulates into the buffer
        self.grad_events = {}
        self.op_index = {id(o): i for i, o in enumerate(eng.g.ops)}
        self.f32plan = eng._f32plan if (fz is None or eng._f32plan is None) else eng._frozen_f32plan(fz)
        self.buckets = {}
        self.due = []                   # gradient buckets whose last unit has been processed: launched at the next flush point
        self.unit_i = len(eng.unit_starts)
        self.pool_i = len(bs.pool_idx)
        self.head_i = len(eng.g.heads)
        self.sync = eng.sync_bn and eng.collectives
        self.rccl_sync = self.sync and eng.peer is None

    # ------------------------------------------------------------------ streams: weight gradients, gradient buckets
    def join_main(self):
        """the weight-gradient stream (where the gradient buckets ride) waits for what the main stream has queued"""
        if self.wg is not None and self.buckets:
            ev = torch.cuda.Event()
            ev.record(self.main)
            self.wg.wait_event(ev)

    def fork_point(self, stream=None):
        """call right after the kernel that completes dY (on `stream`, default the main stream)"""
        if self.wg is not None:
            self.fork_ev = torch.cuda.Event()
            self.fork_ev.record(stream or self.main)

    def launch_wgrad(self, name, nbytes, args, stream_obj):
        """args = kodhip_conv_wgrad's (x, dy, slab scratch, grad, geometry ..., n_valid, stem, scale), or ("stem",
        kodhip_stem_bwd_fused's arguments) or ("dual", kodhip_conv_wgrad_dual's arguments)"""
        eng, lib = self.eng, self.lib
        e0 = eng._t0(stream_obj)
        sid = stream_obj.cuda_stream if stream_obj is not None else self.s
        eng._stamp("wg:" + name, stream_obj)
        if args[0] == "stem":
            chk(lib.kodhip_stem_bwd_fused(*args[1:], sid), name + ".bwd_fused")
        elif args[0] == "dual":
            chk(lib.kodhip_conv_wgrad_dual(*args[1:], sid), name + ".wgrad2")
        else:
            chk(lib.kodhip_conv_wgrad(*args, sid), name + ".wgrad")
        eng._t1(e0, "wgrad", nbytes, stream_obj, name=name)

    def flush_wgrads(self):
        """call after the main stream's next kernel has been launched"""
        for ev, name, nbytes, args in self.deferred:
            self.wg.wait_event(ev)
            self.launch_wgrad(name, nbytes, args, self.wg)
        self.deferred.clear()
        if self.due and not self.hold:
            self.launch_due()

    def timed_wgrad(self, name, nbytes, *args):
        if self.wg is None:
            self.launch_wgrad(name, nbytes, args, None)
            return
        ev, self.fork_ev = self.fork_ev, None
        if ev is None:
            ev = torch.cuda.Event()
            ev.record(self.main)
        self.deferred.append((ev, name, nbytes, args))

    def launch_due(self):
        eng = self.eng
        for idx in self.due:
            lo, hi = self.buckets[idx]
            cs = eng._comm_stream()
            # overlapped buckets use their own communicator: SyncBN sums (main stream) and buckets (side stream)
            # never interleave on one communicator from two streams
            bc = eng.comm_buckets if (cs is not None and eng.comm_buckets is not None) else eng.comm
            # on the weight-gradient stream the bucket's last weight gradient has already waited for an event
            # recorded behind every BatchNorm / bias gradient of the bucket (fork_point): no new edge from the main chain
            # (under a freeze plan the bucket's last unit may launch no weight gradient: wait for the main stream)
            eng._pending.append(launch_bucket(self.ga, lo, hi, eng.process_group, cs, bc, also_after=self.wg,
                                              wait_caller=not (cs is not None and cs is self.wg) or self.fz is not None))
        self.due.clear()

    def bucket_tick(self):
        """one conv / head unit's gradients are complete: buckets finish from the arena's end toward its start.  The
        bucket is launched at a flush point of the weight-gradient stream, never ahead of one: a fused short_conv's
        weight gradient is still deferred here (it is captured behind its main_conv's data gradient, so that the main
        chain's next kernel stays the first captured successor - see flush_wgrads), and flushing it early for the
        bucket's sake moves the main chain to another queue in the replayed graph (measured: -11 % step rate)."""
        self.unit_i -= 1
        if self.unit_i in self.buckets:
            self.due.append(self.unit_i)
            if not self.deferred and not self.hold:
                self.launch_due()

    # ------------------------------------------------------------------ gradient buffers
    def sync_grad(self, name):
        ev = self.grad_events.pop(name, None)
        if ev is not None:
            self.main.wait_event(ev)

    def acc_flag(self, v: View) -> int:
        """0 = first writer (overwrite), 1 = accumulate; zero-fills on a partial first touch."""
        eng, name = self.eng, v.buf.name
        self.sync_grad(name)
        if name in self.touched:
            return 1
        self.touched.add(name)
        if v.C != v.buf.C:
            self.bs.gact[name].zero_()
            if name in self.bs.gact32:
                self.bs.gact32[name].zero_()
            return 1
        return 0

    def f32(self, kind, ident, v: View):
        """(bits 8.. of the `accumulate` argument, fp32 shadow pointer) of one gradient-buffer write (engine/plan.py)"""
        if self.f32plan is None:
            return 0, None
        mode = self.f32plan.modes.get((kind, self.op_index[id(ident)] if kind in ("up", "pool") else ident), 0)
        sh = self.bs.gact32.get(v.buf.name)
        return mode << 8, (sh.data_ptr() if (sh is not None and mode in (1, 2, 3)) else None)

    # ------------------------------------------------------------------ BatchNorm-backward coefficients
    def coef_job(self, u, ranks: int = 1):
        """one unit's coefficient job: (partials, slots, M, gamma, mean, rstd, dgamma, dbeta, coef, C, raw_moment)"""
        st, C_ = self.bs.units[u.name], u.cout
        lay, aff, pa, gp = st.lay, st.aff.data_ptr(), self.pa, self.gp
        # raw_moment: the partials came from the last dgrad into this tensor
        return (st.bpart.data_ptr(), st.T2, float(st.M) * ranks, pa + 4 * lay.g_off, aff + 8 * C_, aff + 12 * C_,
                gp + 4 * lay.g_off, gp + 4 * lay.b_off, st.coef.data_ptr(), C_, 1 if st.fused_red else 0)

    def bn_bwd_stats(self, group):
        """BatchNorm-backward sums -> coefficients.  Under SyncBN the [sum dz, sum dz*xhat] vectors of the group's
        units (a CSP layer's short + main convs) are exchanged as ONE grouped collective.  The launches come from the
        forward's BatchNorm mode plan (engine/bn_mode.py coef_launches; the default plan: one train launch of the group):
        eval units take the eval-mode coefficient kernel and no exchange; an eval unit whose gamma and beta are both
        frozen launches nothing (its coefficients came with the forward's eval constants); the train units of the group
        run the batch-statistics program."""
        eng, lib, s = self.eng, self.lib, self.s
        for u in group:
            self.sync_grad(u.dst.buf.name)          # (a head's data gradient on the side stream may be its last writer)
        by_name = {u.name: u for u in group}
        for kind, names, flags in coef_launches(eng.bn_mode, self.fz, [u.name for u in group], self.sync):
            units = [by_name[n] for n in names]
            for u in units:
                st, C_ = self.bs.units[u.name], u.cout
                if not st.fused_red:
                    aff, dA = st.aff.data_ptr(), u.dst
                    e0 = eng._t0()
                    chk(lib.kodhip_bn_act_bwd_reduce(eng._ptr(dA, True), dA.buf.C, dA.coff, st.raw.data_ptr(), st.raw_ld,
                                                     aff, aff + 4 * C_, aff + 8 * C_, aff + 12 * C_,
                                                     st.bpart.data_ptr(), st.M, C_, eng.act_kind, eng.act_slope, s), u.name)
                    eng._t1(e0, "bn_bwd_reduce", 4.0 * st.M * C_, name=u.name)
            e0 = eng._t0()
            if kind == "train":
                self.coef_train(units)
            elif kind == "mode2":
                ranks = eng.world_size if self.sync else 1
                chk(lib.kodhip_bn_bwd_coeffs_eval_partials2(*self.coef_job(units[0], ranks), flags[0],
                                                            *self.coef_job(units[1], ranks), flags[1], s), "+".join(names))
            else:
                job = self.coef_job(units[0])
                chk(lib.kodhip_bn_bwd_coeffs_eval_partials(job[0], job[1], *job[3:], s), names[0])
            eng._t1(e0, "bn_bwd_coeffs", sum(8.0 * u.cout * self.bs.units[u.name].T2 for u in units), name="+".join(names))

    def coef_train(self, group):
        """the train-mode coefficient launch(es) of a group: peer exchange, RCCL exchange, paired launch or single launch"""
        eng, lib, s = self.eng, self.lib, self.s
        if self.sync and eng.peer is not None:
            for u in group:
                chk(lib.kodhip_bn_bwd_coeffs_partials_peer(*self.coef_job(u, eng.world_size), eng.peer.view_ptr(),
                                                           eng.peer_slots[(u.name, "b")], s), u.name)
        elif self.sync:
            for u in group:
                st = self.bs.units[u.name]
                chk(lib.kodhip_bn_reduce_partials(st.bpart.data_ptr(), st.bsums.data_ptr(), u.cout, st.T2, s), u.name)
            # out of place: the local sums stay for dgamma / dbeta
            eng._allreduce_group([self.bs.units[u.name].bsums for u in group], [self.bs.units[u.name].bsums_g for u in group])
            for u in group:
                st = self.bs.units[u.name]
                chk(lib.kodhip_bn_bwd_coeffs(st.bsums.data_ptr(), st.bsums_g.data_ptr(),
                                             *self.coef_job(u, eng.world_size)[2:], s), u.name)
        elif len(group) == 2:           # short_conv + main_conv: one launch for both coefficient sets
            chk(lib.kodhip_bn_bwd_coeffs_partials2(*self.coef_job(group[0]), *self.coef_job(group[1]), s),
                group[0].name + "+" + group[1].name)
        else:
            for u in group:
                chk(lib.kodhip_bn_bwd_coeffs_partials(*self.coef_job(u), s), u.name)

    # ------------------------------------------------------------------ the program
    def run(self, out_grads):
        eng, lib, s = self.eng, self.lib, self.s
        B, H, W = self.B, self.H, self.W
        fz, main, touched = self.fz, self.main, self.touched
        # sub-network graphs: the callers' output gradients are the first writers of those buffers
        if eng.g.outputs:
            og = list(out_grads) if out_grads is not None else [None] * len(eng.g.outputs)
            for v, t in zip(eng.g.outputs, og):
                name = v.buf.name
                if name not in touched:
                    touched.add(name)
                    if v.C != v.buf.C or t is None:
                        self.bs.gact[name].zero_()
                if t is not None:
                    self.bs.gact[name][..., v.coff:v.coff + v.C].copy_(t.permute(0, 2, 3, 1))
        eng._pending = []
        if eng.collectives:
            first = 0 if fz is None else trainable_span(eng.unit_starts, fz, eng.layout)
            self.buckets = {trig: (lo, hi) for trig, lo, hi in plan_buckets(eng.unit_starts, eng.n_arena,
                                                                             max(eng.bucket_bytes // 4, 1), first)}
        # (with every collective on the main stream - KODHIP_COMM_OVERLAP=0, RCCL SyncBN - the head chains stay there too)
        self.heads_side = (self.wg is not None and eng.branch_overlap and eng.profile is None and
                           (not eng.collectives or (eng._comm_stream() is not None and not self.rccl_sync)))
        eng._stamp("bwd_begin")
        self.bwd_start = torch.cuda.Event()
        if self.heads_side:
            self.bwd_start.record(main)
        rops = list(reversed(eng.g.ops))
        ri = 0
        while ri < len(rops):
            op = rops[ri]
            ri += 1
            if op.kind == "head":
                self.head(op.unit)
                # gradient buckets complete from the arena's end toward its start
                self.bucket_tick()
            elif fz is not None and op.kind in ("up", "pool") and not fz.op_in_grad[len(rops) - ri]:
                if op.kind == "pool":          # nothing upstream of this pass-through needs its gradient
                    self.pool_i -= 1
            elif op.kind == "up":
                h, w = H // op.src.stride, W // op.src.stride
                chk(lib.kodhip_upsample2x_bwd(eng._ptr(op.dst, True), op.dst.buf.C, op.dst.coff,
                                              eng._ptr(op.src, True), op.src.buf.C, op.src.coff,
                                              self.acc_flag(op.src), B, h, w, op.src.C, self.f32("up", op, op.src)[1], s), "upsample_bwd")
            elif op.kind == "pool":
                self.pool_i -= 1
                h, w = H // op.src.stride, W // op.src.stride
                # src and dst are slices of the same (already initialised) concat gradient buffer
                chk(lib.kodhip_maxpool_bwd(eng._ptr(op.dst, True), op.dst.buf.C, op.dst.coff,
                                           self.bs.pool_idx[self.pool_i].data_ptr(), eng._ptr(op.src, True),
                                           op.src.buf.C, op.src.coff, B, h, w, op.src.C, op.k, self.f32("pool", op, op.src)[1], s), "maxpool_bwd")
            else:
                group = [op.unit]
                # SyncBN: short_conv (reached first in reverse order) and its main_conv share one exchange - main's
                # output gradient is complete by now (everything between them in the forward program ran backward)
                if ri < len(rops) and rops[ri].kind == "conv" and rops[ri].unit.sibling is op.unit and \
                        (self.rccl_sync or rops[ri].unit.name in eng._dual):
                    group.append(rops[ri].unit)
                    ri += 1
                # what each unit of the group launches (engine/freeze.py group_launches; None: outside the grad region)
                launches = group_launches(group, fz, eng._dual, len(group) == 2 and self.bs.units[group[1].name].wg_dual > 0)
                runs = [u for u, ln in zip(group, launches) if ln is not None]
                if runs:
                    self.bn_bwd_stats(runs)
                for u, ln in zip(group, launches):
                    if ln is not None:
                        self.unit(u, ln)
                    self.bucket_tick()
        self.flush_wgrads()
        eng._stamp("main_end")
        if self.wg is not None:
            eng._stamp("wg_end", self.wg)
        for name in list(self.grad_events):
            self.sync_grad(name)
        if self.wg is not None:
            main.wait_stream(self.wg)
        eng._stamp("bwd_end")

    def head(self, hu: HeadUnit):
        """gradient re-layout -> data gradient -> weight gradient of one head"""
        eng, lib, gp = self.eng, self.lib, self.gp
        B, main, s, fz = self.B, self.main, self.s, self.fz
        A, nc = eng.g.num_anchors, eng.g.num_classes
        self.head_i -= 1
        hf = fz.heads[hu.name] if fz is not None else None
        if hf is not None and not hf.needs_out_grad:
            return
        hs = self.bs.heads[hu.name]
        geo = hs.geo_bwd(eng.head_npad)
        gten = self.head_grads[self.head_i].contiguous()
        assert gten.shape == (B, A, hs.H, hs.W, 5 + nc) and gten.dtype == torch.float32
        names = [head_param(hu, k, "bias") for k in ("box", "obj", "cls")]
        offs = [eng.layout[n][0] for n in names]
        src = hu.src
        # The three head chains (gradient re-layout -> data gradient) are independent until the neck: the P5
        # chain, which the first backward layers wait for, stays on the main stream; the P4 and P3 chains
        # run beside it on a side stream and the main stream joins each where that level's gradient buffer
        # is next touched (acc_flag / the producing unit's apply).
        side = (self.heads_side and self.head_i < len(eng.g.heads) - 1 and src.C == src.buf.C and src.buf.name not in self.touched)
        hstream, hs_ = main, s
        if side:
            if eng.head_stream is None:
                eng.head_stream = torch.cuda.Stream(device=eng.device)
            hstream, hs_ = eng.head_stream, eng.head_stream.cuda_stream
            hstream.wait_event(self.bwd_start)
        chk(lib.kodhip_head_bwd_prep(gten.data_ptr(), hs.dy.data_ptr(), hs.ws.data_ptr(),
                                     gp + 4 * offs[0], gp + 4 * offs[1], gp + 4 * offs[2],
                                     B, hs.H * hs.W, A, nc, eng.head_npad, hs_), hu.name)
        self.fork_point(hstream)
        if hf is None or hf.needs_in_grad:
            acc = self.acc_flag(src)
            fm, fptr = self.f32("head", hu.name, src)
            e0 = eng._t0()
            chk(lib.kodhip_conv_dgrad(hs.dy.data_ptr(), self.dp + 2 * hs.lay.d_off, eng._ptr(src, True),
                                      *geo, hs.lay.Kdp, eng.head_npad, 0, acc | fm, fptr, hs_), hu.name + ".dgrad")
            eng._t1(e0, "dgrad", 2.0 * hs.M * (eng.head_npad + hu.cin), name=hu.name)
            if side:
                ev = torch.cuda.Event()
                ev.record(hstream)
                self.grad_events[src.buf.name] = ev
        elif side:                 # (the bias gradients of the side chain: joined before they are published)
            ev = torch.cuda.Event()
            ev.record(hstream)
            self.grad_events["head:" + hu.name] = ev
        if hf is None or any(hf.w_trainable):
            self.timed_wgrad(hu.name, 2.0 * hs.M * (hu.cin + eng.head_npad),
                             eng._ptr(src), hs.dy.data_ptr(), self.wgp, gp + 4 * hs.lay.w_off,
                             *geo, hs.lay.Kp, eng.head_npad, 0, A * (5 + nc), 0, 1.0)
        else:
            self.fork_ev = None
        self.flush_wgrads()

    def unit(self, u, ln: UnitLaunch):
        """bn/silu backward apply -> data gradient -> weight gradient of one conv unit (coefficients already in st.coef).
        ln.dgrad: "own" = this unit's launch; "skip" = none (a fused short_conv: its main_conv's launch covers it);
        "dual" = one launch for this unit and ln.partner (kodhip_conv_dgrad_dual); "none" = no data gradient (freeze plan:
        nothing upstream needs it).  ln.w_grad / ln.res_grad (freeze plan): the weight gradient / the residual pass-through
        is needed."""
        eng, lib = self.eng, self.lib
        B, H, W, s, gp, dp, wgp = self.B, self.H, self.W, self.s, self.gp, self.dp, self.wgp
        dgrad, partner, dual_w, w_grad = ln.dgrad, ln.partner, ln.dual_w, ln.w_grad
        st = self.bs.units[u.name]
        lay, C_, aff = st.lay, u.cout, st.aff.data_ptr()
        dA, res = u.dst, u.residual
        eng._stamp("m:" + u.name)
        if not ln.res_grad:
            res = None
        if not (w_grad or res is not None or dgrad != "none"):
            self.flush_wgrads()               # (only the BatchNorm affine gradients, written by the coefficient kernel)
            return
        if st.stem_fused and res is None:
            # the stem has no data gradient: dY = f(dA, y) is formed inside its weight gradient and never written
            # (csrc/conv_wgrad.hip conv_stem_bwd_fused_kernel); the launch joins the weight-gradient stream behind the
            # coefficient kernel
            fargs = (eng._ptr(u.src), eng._ptr(dA, True), dA.buf.C, dA.coff, st.raw.data_ptr(), st.raw_ld,
                     aff, aff + 4 * C_, st.coef.data_ptr())
            nb = 2.0 * (B * H * W * 3 + 2 * st.M * C_)
            if eng.opt.native.get("KODHIP_STEM_BWD_STREAM", "main") == "main":
                # on the MAIN stream, with a slab scratch of its own: it is the main chain's last kernel, and the chip is
                # otherwise left to the tail of the weight-gradient stream (small launches, one at a time) - this HBM-bound
                # kernel runs beside them instead of behind them
                e0 = eng._t0()
                chk(lib.kodhip_stem_bwd_fused(*fargs, self.bs.stem_part.data_ptr(), gp + 4 * lay.w_off,
                                              B, st.H, st.W, C_, 1.0, s), u.name + ".bwd_fused")
                eng._t1(e0, "wgrad", nb, name=u.name)
                self.flush_wgrads()
                self.join_main()          # a gradient bucket on the weight-gradient stream must see this gradient
                return
            self.fork_point()
            self.timed_wgrad(u.name, nb, "stem", *fargs, wgp, gp + 4 * lay.w_off, B, st.H, st.W, C_, 1.0)
            self.flush_wgrads()
            return
        racc = self.acc_flag(res) if res else 0
        e0 = eng._t0()
        chk(lib.kodhip_bn_act_bwd_apply(eng._ptr(dA, True), dA.buf.C, dA.coff, st.raw.data_ptr(), st.raw_ld,
                                        aff, aff + 4 * C_, st.coef.data_ptr(),
                                        eng._ptr(res, True) if res else None,
                                        res.buf.C if res else 0, res.coff if res else 0,
                                        racc, st.M, C_, eng.act_kind, eng.act_slope, s), u.name)
        eng._t1(e0, "bn_silu_bwd_apply", (6.0 + ((4.0 if racc else 2.0) if res else 0.0)) * st.M * C_, name=u.name)
        self.fork_point()
        # st.raw now holds dY
        geo = st.geo_bwd()
        if not u.stem:
            segs = () if st.segs is None else (C.cast(st.segs, C.c_void_p), len(st.segs), st.seg_slots)
            if dgrad == "skip" and dual_w:          # its weight gradient rides in the main_conv's dual launch
                self.hold = True
                return
            if dgrad == "skip":
                if w_grad:
                    self.timed_wgrad(u.name, float(st.conv_bytes()),
                                     eng._ptr(u.src), st.raw.data_ptr(), wgp, gp + 4 * lay.w_off,
                                     *geo, lay.Kp, st.raw_ld, 0, C_, 0, 1.0)
                return
            if dgrad != "none":
                fm, fptr = self.f32("dgrad", u.name, u.src)
                acc_src = self.acc_flag(u.src) | fm
                in_px = B * st.H * st.W
                # dY read once, dX written once (+ read when accumulating), + the re-read of the producers' pre-BN
                # tensors when this launch carries their BatchNorm-backward reduction
                nb = 2.0 * st.M * C_ + (4.0 if acc_src & 1 else 2.0) * in_px * u.cin
                if st.segs is not None:
                    nb += 2.0 * in_px * sum(sg.ch_count for sg in st.segs)
                e0 = eng._t0()
                if dgrad == "dual":
                    ps = self.bs.units[partner.name]
                    nb += 2.0 * ps.M * partner.cout
                    fn = lib.kodhip_conv_dgrad_dual if st.segs is None else lib.kodhip_conv_dgrad_dual_bnred
                    chk(fn(st.raw.data_ptr(), dp + 2 * lay.d_off, ps.raw.data_ptr(), dp + 2 * ps.lay.d_off, eng._ptr(u.src, True),
                           *geo[:7], lay.Kdp, st.raw_ld, 0, acc_src, fptr, *segs, s), u.name + ".dgrad2")
                elif u.k == 3 and u.s == 2 and u.p == 1:
                    if lay.s2_fold:
                        fn = lib.kodhip_conv_dgrad_s2f if st.segs is None else lib.kodhip_conv_dgrad_s2f_bnred
                    else:
                        fn = lib.kodhip_conv_dgrad_s2 if st.segs is None else lib.kodhip_conv_dgrad_s2_bnred
                    chk(fn(st.raw.data_ptr(), dp + 2 * lay.d_off, eng._ptr(u.src, True),
                           *geo[:7], st.raw_ld, 0, acc_src, fptr, *segs, s), u.name + ".dgrad")
                else:
                    fn = lib.kodhip_conv_dgrad if st.segs is None else lib.kodhip_conv_dgrad_bnred
                    chk(fn(st.raw.data_ptr(), dp + 2 * lay.d_off, eng._ptr(u.src, True),
                           *geo, lay.Kdp, st.raw_ld, 0, acc_src, fptr, *segs, s), u.name + ".dgrad")
                eng._t1(e0, "dgrad" if st.segs is None else "dgrad+bn_reduce", nb, name=u.name + ("+" + partner.name if dgrad == "dual" else ""))
        if dgrad == "dual" and dual_w:
            ps = self.bs.units[partner.name]
            self.hold = False
            self.timed_wgrad(u.name + "+" + partner.name, 2.0 * (B * st.H * st.W * u.cin + 2 * st.M * C_),
                             "dual", eng._ptr(u.src), st.raw.data_ptr(), ps.raw.data_ptr(), wgp,
                             gp + 4 * lay.w_off, gp + 4 * ps.lay.w_off, *geo[:7], lay.Kp, st.raw_ld, 0, 1.0)
            self.flush_wgrads()
            return
        if w_grad:
            self.timed_wgrad(u.name, float(st.conv_bytes()),
                             eng._ptr(u.src), st.raw.data_ptr(), wgp, gp + 4 * lay.w_off,
                             *geo, lay.Kp, st.raw_ld, 0, C_, 1 if u.stem else 0, 1.0)
        self.flush_wgrads()           # this unit's - and a fused short_conv partner's - weight gradients: after the dgrad


class BackwardMixin:
    # ------------------------------------------------------------------ backward
    def backward(self, head_grads: List[torch.Tensor], out_grads: Optional[List[torch.Tensor]] = None):
        """head_grads: d loss / d (ll, ml, hl) head tensors.  Fills the gradient arena.  Sub-network graphs: out_grads =
        d loss / d Graph.outputs (NCHW, None = zero); returns d loss / d Graph.inputs (NCHW fp32), else nothing."""
        assert self.training_ready, "backward() needs a preceding training forward()"
        self.training_ready = False
        bp = _BackwardPass(self, head_grads)
        bp.run(out_grads)
        self._publish_grads()
        if self.g.inputs:
            B, H, W = self.cur.shape
            return [self.cur.gact[v.buf.name][..., v.coff:v.coff + v.C].permute(0, 3, 1, 2).float() if v.buf.name in bp.touched
                    else torch.zeros((B, v.C, H // v.stride, W // v.stride), device=self.device) for v in self.g.inputs]

    def _frozen_f32plan(self, fz):
        """EngineOptions.dx_accum_fp32 under a freeze plan: the fp32-accumulation modes planned over the gradient writes
        that backward still issues (engine/plan.py; skipped writers change who is first / last of a buffer)."""
        from .plan import backward_writes, plan_f32_accumulation
        cached = self._f32_frozen.get(fz.key)
        if cached is None:
            ws, _ = backward_writes(self.g, {v.name for v in self._dual.values()})
            kept = []
            for w in ws:
                kind, ident = w.key
                if kind == "dgrad":
                    ok = fz.units[ident].needs_in_grad
                elif kind == "res":
                    ok = fz.units[ident].res_grad
                elif kind == "head":
                    ok = fz.heads[ident].needs_in_grad
                else:
                    ok = fz.op_in_grad[ident]
                if ok:
                    kept.append(w)
            cached = plan_f32_accumulation(kept, {b.name: b.C for b in self.g.bufs})
            self._f32_frozen[fz.key] = cached
        for name in cached.shadow_bufs:           # (a buffer that needs a shadow only with fewer writers)
            if name not in self.cur.gact32:
                self.cur.gact32[name] = torch.empty(self.cur.gact[name].shape, dtype=torch.float32, device=self.device)
        return cached

    def _comm_stream(self):
        """Stream of the gradient-bucket all-reduces.  Default (comm_overlap): the WEIGHT-GRADIENT side stream, through
        the buckets' own communicator - a bucket is enqueued right behind the last weight gradient that fills it and
        overlaps the rest of backward on the main stream (torch DDP's reducer does the same with its hooks; north_star:
        "all-reduce overlapped with the backward pass").  SyncBN sums (main stream, `comm`) and buckets (side stream,
        `comm_buckets`) never share a communicator, so no communicator sees calls from two streams; every rank enqueues
        the same program, so the order inside each stream / graph branch is the same on all ranks.
        KODHIP_COMM_OVERLAP=0: None = everything on the main stream in one order (the conservative switch)."""
        if not self.comm_overlap or self.wg_stream is None or not self.wgrad_overlap:
            return None
        return self.wg_stream

    def wait_grads(self):
        for w in self._pending:
            w.wait()
        self._pending = []
