"""Per-shape buffer sets of the engine (activations, activation gradients, pre-BN tensors, statistic slots, weight-
gradient slabs, fp32 shadows) and the shape-dependent launch plans that hold pointers into them.

A captured hipGraph bakes buffer addresses in, so every (B, H, W) keeps its own complete BufferSet and a forward at
another shape makes another set current instead of reallocating.  The decisions themselves (who writes which gradient
buffer last, which gradients need fp32 accumulation, bucket boundaries) are pure functions in engine/plan.py and
engine/ddp.py, derived once per engine (_plan_static); a set asks libkodhip for the slot / split counts of each launch at
its shape and allocates accordingly.  BufferMixin is mixed into Engine.
"""
from __future__ import annotations

from typing import Dict

import torch

from .. import _lib
from .arenas import _pad
from .plan import backward_writes, plan_f32_accumulation, plan_dual_dgrads, plan_bn_reduce_fusion


def dense(geo):
    """a backward geometry without its channel offset: what kodhip_conv_wgrad_splits_geo takes (a row stride, no view)"""
    return geo[:4] + geo[5:]


class UnitBuffers:
    """Per conv unit, per buffer set: geometry at this shape, the pre-BN tensor, statistic / coefficient buffers and the
    launch state sized by the library's queries.  `lay` is the unit's per-engine UnitLayout (offsets, K paddings)."""
    __slots__ = ("lay", "B", "H", "W", "Ho", "Wo", "M", "raw", "raw_ld", "stats", "T", "sums", "aff", "bpart", "T2",
                 "bsums", "bsums_g", "coef", "fused_red", "segs", "seg_slots", "stem_fused", "wg_dual")

    # -- the geometry arguments of a conv launch: (B, H, W, ldx, channel offset, Cin, Cout, KH, KW, sh, sw, ph, pw)
    # The stem reads the image as pixel pairs [B, H, W/2, 8] (r g b 0 of two neighbouring pixels), so its 6x6 / s2 conv
    # over 3 channels becomes a conv over 8-channel "pixels" of half the width, in three forms:
    #   forward   6x1 taps over Cin = 32: each kernel row is ONE 32-value K step (4 pixel pairs, the 4th zero - see
    #             UnitLayout.Kp_f), so that it runs on the LDS-DMA path like every other layer;
    #   backward  6x3 taps over Cin = 8 (K = 144 -> Kp = 160), what the weight-gradient slabs and the data gradient see;
    #   queries   the backward form without the channel offset: dense() above.
    def geo_fwd(self):
        """arguments of kodhip_conv_fwd_raw / kodhip_conv_fwd_fused between the pointers and the output's row stride"""
        if self.lay.u.stem:
            return (self.B, self.H, self.W, 8, 0, 32, self.lay.u.cout, 6, 1, 2, 1, 2, 1, self.lay.Kp_f)
        return self.geo_bwd() + (self.lay.Kp_f,)

    def geo_bwd(self):
        """the same for the data gradient and the weight gradient (before their own K padding)"""
        u = self.lay.u
        if u.stem:
            return (self.B, self.H, self.W, 8, 0, 8, u.cout, 6, 3, 2, 1, 2, 1)
        return (self.B, self.H, self.W, u.src.buf.C, u.src.coff, u.cin, u.cout, u.k, u.k, u.s, u.s, u.p, u.p)

    def conv_bytes(self) -> int:
        """algorithmic bytes of one conv launch over this unit (forward or weight gradient): the input read once (the
        stem: the image's 3 true channels, two pixels per pair), the output or its gradient once, bf16"""
        u = self.lay.u
        in_px = self.B * self.H * self.W
        return 2 * ((2 * in_px * 3 if u.stem else in_px * u.cin) + self.M * u.cout)


class HeadBuffers:
    """Per head, per buffer set: the level's map size, the re-laid-out output gradient `dy` and the bias-gradient
    workspace `ws`.  `lay` is the head's per-engine HeadLayout."""
    __slots__ = ("lay", "B", "H", "W", "M", "dy", "ws")

    def geo_bwd(self, npad: int):
        """geometry arguments of the head's data / weight gradient: a 1x1 conv from the source view to `npad` outputs"""
        src = self.lay.h.src
        return (self.B, self.H, self.W, src.buf.C, src.coff, self.lay.h.cin, npad, 1, 1, 1, 1, 0, 0)


class BufferSet:
    """Everything the engine holds for one input shape (B, H, W).  Built once by BufferMixin._build_set, then only made
    current or dropped: no field is copied anywhere, so a captured graph and the eager program of a shape always see the
    same addresses."""
    __slots__ = ("shape", "act", "gact", "gact32", "wg_part", "stem_part", "pool_idx", "units", "heads")

    def __init__(self, shape):
        self.shape = shape
        # buffer name -> bf16 [B, h, w, C] (image: [B, H, W/2, 8]) | its gradient | the gradient's fp32 shadow (dx_accum_fp32)
        self.act, self.gact, self.gact32 = {}, {}, {}
        # split-K slab scratch of the weight gradients | the fused stem backward's own slabs (None: not fused) | SPPF argmax
        self.wg_part, self.stem_part, self.pool_idx = None, None, []
        self.units: Dict[str, UnitBuffers] = {}          # by unit / head name: the per-shape records
        self.heads: Dict[str, HeadBuffers] = {}


class BufferMixin:
    # ------------------------------------------------------------------ shape sets
    def pin_shape(self, B: int, H: int, W: int):
        """A captured graph replays into the buffer set of this shape: keep it until every pin is released (`unpin_shape`).
        Pins are counted - a training step and several eval graphs may hold the same shape."""
        key = (B, H, W)
        self._pin_counts[key] = self._pin_counts.get(key, 0) + 1
        self._pinned.add(key)

    def unpin_shape(self, B: int, H: int, W: int):
        """Release one pin of this shape (the graph that took it is gone).  With the last pin the set becomes an ordinary
        one again: it stays until `allocate` drops it least-recently-used beyond KODHIP_MAX_SHAPE_SETS."""
        key = (B, H, W)
        n = self._pin_counts.get(key, 0)
        if n < 1:
            raise ValueError(f"unpin_shape{key}: the shape is not pinned")
        if n == 1:
            del self._pin_counts[key]
            self._pinned.discard(key)
        else:
            self._pin_counts[key] = n - 1

    def allocate(self, B: int, H: int, W: int):
        """Make the buffer set of (B, H, W) current.  Sets are kept (a dict keyed by shape, least recently used first),
        never reallocated: a forward at another shape leaves the previous set - and any hipGraph captured over it -
        intact.  Unpinned sets beyond KODHIP_MAX_SHAPE_SETS are dropped least-recently-used first."""
        key = (B, H, W)
        if self.cur is not None and self.cur.shape == key:
            return
        top = max(b.stride for b in self.g.bufs)
        assert H % top == 0 and W % top == 0, f"input size must be a multiple of {top} (the graph's coarsest map)"
        self.training_ready = False                              # a pending backward belongs to the previous set
        bs = self._sets.pop(key, None)
        if bs is None:
            for old in [k for k in self._sets if k not in self._pinned][:max(0, len(self._sets) + 1 - self.max_shape_sets)]:
                del self._sets[old]
            bs = self._build_set(B, H, W)
        self._sets[key] = bs                                     # (inserted last = most recently used)
        self.cur = bs

    def _build_set(self, B: int, H: int, W: int) -> BufferSet:
        dev, lib = self.device, self.lib
        bs = BufferSet((B, H, W))
        for b in self.g.bufs:
            shp = (B, H, W // 2, 8) if b.name == "image" else (B, H // b.stride, W // b.stride, b.C)
            bs.act[b.name] = torch.empty(shp, dtype=torch.bfloat16, device=dev)
            if b.name != "image":
                bs.gact[b.name] = torch.empty(shp, dtype=torch.bfloat16, device=dev)
        max_part = 0
        for u in self.exec_units:
            st = bs.units[u.name] = UnitBuffers()
            st.lay, st.B = self.ulayout[u.name], B
            st.H, st.W = (H, W // 2) if u.stem else (H // u.src.stride, W // u.src.stride)      # (the stem: pixel pairs)
            st.Ho, st.Wo = (H // 2, W // 2) if u.stem else (st.H // u.s, st.W // u.s)
            st.M = B * st.Ho * st.Wo
            st.raw = torch.empty((B, st.Ho, st.Wo, u.cout), dtype=torch.bfloat16, device=dev)
            st.raw_ld = u.cout                         # row stride of raw (pre-BN output / dY)
            st.T = lib.kodhip_conv_stats_slots(st.M, u.cout)
            st.stats = torch.empty(2 * u.cout * st.T, dtype=torch.float32, device=dev)
            st.sums = torch.empty(2 * u.cout, dtype=torch.float64, device=dev)
            st.aff = torch.empty(4 * u.cout, dtype=torch.float32, device=dev)        # scale|shift|mean|rstd
            st.T2 = lib.kodhip_bn_bwd_slots(st.M, u.cout)
            st.bpart = torch.empty(2 * u.cout * st.T2, dtype=torch.float32, device=dev)
            st.bsums = torch.empty(2 * u.cout, dtype=torch.float64, device=dev)
            st.bsums_g = torch.empty(2 * u.cout, dtype=torch.float64, device=dev)
            st.coef = torch.empty(3 * u.cout, dtype=torch.float32, device=dev)
            st.fused_red, st.segs, st.seg_slots, st.wg_dual = False, None, 0, 0
            nslab = lib.kodhip_conv_wgrad_splits_geo(*dense(st.geo_bwd()), st.lay.Kp, u.cout) * u.cout * st.lay.Kp
            # the stem's backward as one kernel (kodhip_stem_bwd_fused): a slab per block, 32 (cout <= 32) or 64 rows
            st.stem_fused = bool(u.stem and u.cout <= 64 and self.opt.stem_bwd_fused)
            if st.stem_fused:
                nslab = lib.kodhip_stem_bwd_fused_blocks(B, st.H, st.W, u.cout) * (32 if u.cout <= 32 else 64) * 160
                bs.stem_part = torch.empty(nslab, dtype=torch.float32, device=dev)    # (it runs on the main stream)
            # slab region [splits][cout][Kp] (floats): ONE scratch shared by all layers, reduced right after each weight
            # gradient, while it is still in the 256 MB Infinity Cache
            max_part = max(max_part, nslab)
        self._plan_bn_fusion(bs)
        # a dual pair's weight gradients as one launch (kodhip_conv_wgrad_dual): slab rows for both layers
        if self.opt.dual_wgrad:
            for mname in self._dual:
                st = bs.units[mname]
                u = st.lay.u
                st.wg_dual = lib.kodhip_conv_wgrad_dual_splits(B, st.H, st.W, u.src.buf.C, u.cin, u.cout, st.lay.Kp, st.raw_ld)
                max_part = max(max_part, st.wg_dual * 2 * u.cout * st.lay.Kp)
        if self._f32plan is not None:
            for name in self._f32plan.shadow_bufs:
                bs.gact32[name] = torch.empty(bs.gact[name].shape, dtype=torch.float32, device=dev)
        for h in self.g.heads:
            hs = bs.heads[h.name] = HeadBuffers()
            hs.lay, hs.B, hs.H, hs.W = self.hlayout[h.name], B, H // h.stride, W // h.stride
            hs.M = B * hs.H * hs.W
            hs.dy = torch.empty((hs.M, self.head_npad), dtype=torch.bfloat16, device=dev)
            hs.ws = torch.empty(2048 * self.head_npad, dtype=torch.float32, device=dev)
            splits = lib.kodhip_conv_wgrad_splits_geo(*dense(hs.geo_bwd(self.head_npad)), hs.lay.Kp, self.head_npad)
            max_part = max(max_part, splits * self.head_npad * hs.lay.Kp)
        bs.wg_part = torch.empty(_pad(max_part), dtype=torch.float32, device=dev)
        bs.pool_idx = [torch.empty((B, H // op.src.stride, W // op.src.stride, op.src.C), dtype=torch.uint8, device=dev)
                       for op in self.g.ops if op.kind == "pool"]
        return bs

    def _check_equal_local_batch(self, key):
        """SyncBN here divides the all-reduced sums by M_local * world_size (torch's SyncBatchNorm all-gathers the
        per-rank counts instead): that is only right when every rank holds the same number of pixels, so the first
        TRAINING forward of a shape under SyncBN checks it across the group and refuses uneven local batches loudly.
        (Only there: eval forwards exchange nothing, so validation on one rank, or with uneven last batches, must not
        meet a collective.)"""
        if not (self.collectives and self.sync_bn and self.world_size > 1) or key in self._checked_shapes:
            return
        self._checked_shapes.add(key)
        self._require_same_on_all_ranks(tuple(key), "SyncBN needs the same local batch shape on every rank, got {keys}: pad "
                                        "or drop the last uneven batch (DistributedSampler drop_last / padding)")

    def _plan_static(self):
        """The static plans of engine/plan.py, once per engine (they depend on the graph and on options that nothing
        changes after the arenas exist): which CSP entry convs share a dual data gradient (_dual), which multi-producer
        gradients accumulate in fp32 (_f32plan, EngineOptions.dx_accum_fp32), and which data gradients may carry the
        BatchNorm-backward reduction of the units whose output gradient they complete (_bnred_prods)."""
        units = {u.name: u for u in self.exec_units}
        # dual data gradients: a CSP layer's main_conv and short_conv (both pointwise, same input) write dX in ONE launch
        self._dual = {m: units[sh] for m, sh in plan_dual_dgrads(self.g).items()} if self.opt.dual_dgrad else {}
        # who writes which gradient buffer, in backward order
        ws, upos = backward_writes(self.g, {v.name for v in self._dual.values()})
        # activation gradients with several producers: accumulated in fp32 (one rounding) instead of bf16 read-modify-write
        self._f32plan = None
        if self.opt.dx_accum_fp32:
            self._f32plan = plan_f32_accumulation(ws, {b.name: b.C for b in self.g.bufs})
            if self.opt.debug_plan:
                print(f"[kodhip] fp32 accumulation of multi-producer gradients: shadows {sorted(self._f32plan.shadow_bufs)}; "
                      f"bf16 (unsupported) {self._f32plan.unsupported}", flush=True)
        # writer unit -> [(producer unit, first channel)]
        # (A/B knob: only fuse into launches whose reduction length is at least KODHIP_BNRED_MINK; measured best: all)
        prods = plan_bn_reduce_fusion(self.g, ws, upos) if self.opt.bn_reduce_fused else {}
        self._bnred_prods = {w: p for w, p in prods.items() if units[w].k * units[w].k * units[w].cout >= self.opt.bn_reduce_min_k}

    def _plan_bn_fusion(self, bs: BufferSet):
        """The shape half of the BatchNorm-backward reduction fused into data gradients (kodhip_conv_dgrad_*_bnred): per
        writer of _bnred_prods the library's slot query at this shape, then the segment table and the producers' partial
        buffers sized by it."""
        lib = self.lib
        for wname, prods in self._bnred_prods.items():
            wst = bs.units[wname]
            w = wst.lay.u
            s2 = int(w.k == 3 and w.s == 2 and w.p == 1)
            g = wst.geo_bwd()
            if wname in self._dual:
                slots = lib.kodhip_conv_dgrad_dual_bnred_slots(*g[:3], w.cin, w.cout, wst.raw_ld)
            elif s2 and wst.lay.s2_fold:
                slots = lib.kodhip_conv_dgrad_s2f_bnred_slots(*g[:3], w.cin, w.cout, w.cout)
            else:
                slots = lib.kodhip_conv_dgrad_bnred_slots(*g[:3], *g[5:], wst.raw_ld, s2)
            if slots <= 0:
                continue
            segs = (_lib.KodBnRedSeg * len(prods))()
            for i, (pname, ch0) in enumerate(prods):
                st = bs.units[pname]
                cout = st.lay.u.cout
                st.fused_red, st.T2 = True, slots
                st.bpart = torch.empty(2 * cout * slots, dtype=torch.float32, device=self.device)
                segs[i].ch_begin, segs[i].ch_count = ch0, cout
                segs[i].raw, segs[i].ldr = st.raw.data_ptr(), st.raw_ld
                segs[i].aff, segs[i].partials = st.aff.data_ptr(), st.bpart.data_ptr()
            wst.segs, wst.seg_slots = segs, slots
        if self.opt.debug_plan and self.opt.bn_reduce_fused:
            sep = [n for n, st in bs.units.items() if not st.fused_red]
            print(f"[kodhip] BN-backward reduction fused into a data gradient for {len(bs.units) - len(sep)} of {len(bs.units)} "
                  f"units; separate pass: {sep}", flush=True)
