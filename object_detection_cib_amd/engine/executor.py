"""Executes the static YOLOv5 program (engine/graph.py) with libkodhip kernels.

Replaces what autograd + aten do for the reference's training step
(kod/lightning/experiments/yv5_baseline/exp.py:104-138 -> net forward, loss.backward): forward and
backward are explicit op lists over pre-allocated channels-last bf16 buffers; parameters, gradients and
momentum live in flat fp32 arenas (one fused SGD launch, contiguous all-reduce buckets); weights are
re-packed to bf16 MFMA layouts once per step.

PyTorch is used for device memory, streams and torch.distributed only.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from .. import _lib
from .graph import Graph, check_head_limits
from .options import EngineOptions
from .arenas import ArenaMixin, UnitLayout, HeadLayout, _pad          # noqa: F401
from .buffers import BufferMixin, BufferSet
from .forward import ForwardMixin, BN_EPS, BN_MOMENTUM   # noqa: F401
from .backward import BackwardMixin


class Engine(ArenaMixin, BufferMixin, ForwardMixin, BackwardMixin):
    """Owns arenas + buffers for one network instance (one process, one GPU).  The work is split by concern:
    engine/options.py (every switch), engine/plan.py + engine/ddp.py + engine/freeze.py + engine/bn_mode.py (pure
    planning, CPU-testable), engine/arenas.py (parameters, packs, optimizer; per unit and head one layout record -
    `ulayout`, `hlayout` - with the arena / pack offsets, written once), engine/buffers.py (per input shape one BufferSet:
    activations, gradients, slabs and per unit / head one record of buffers and launch-plan integers; `cur` is the
    current one, made current by one assignment in allocate()), engine/forward.py / engine/backward.py (the launch
    programs; the state of one pass lives in forward._ForwardPass / backward._BackwardPass, each built over `cur`, the
    engine keeps none between calls), engine/comm.py (RCCL communicator, SyncBN peer exchange)."""

    def __init__(self, graph: Graph, params: Dict[str, torch.nn.Parameter], buffers: Dict[str, torch.Tensor],
                 options: Optional[EngineOptions] = None):
        if graph.heads:               # the class-count limit of the head / loss kernels: before anything is allocated or launched
            check_head_limits(graph.num_anchors, graph.num_classes)
        _lib.require_gpu()
        self.lib = _lib.lib()
        self.opt = options or EngineOptions.from_env()      # every switch, read once (engine/options.py)
        self.g = graph
        self.params = params          # full state_dict-style names -> Parameter (shared with the nn.Module)
        self.buffers = buffers        # running_mean / running_var / num_batches_tracked
        self.device = None
        self.cur: Optional[BufferSet] = None      # the current shape's buffer set (allocate())
        # one complete buffer set per (B, H, W): a captured hipGraph bakes buffer addresses in, so a forward at another
        # shape (validation batch, partial last batch) must never free what a graph replays into
        self._sets: Dict[tuple, BufferSet] = {}   # shape -> set, least recently used first (the current one is last)
        self._pinned = set()          # shapes a captured graph depends on: never evicted
        self._pin_counts: Dict[tuple, int] = {}   # how many graphs hold each of them (pin_shape / unpin_shape)
        self.max_shape_sets = self.opt.max_shape_sets
        self.training_ready = False
        self.bn_eps, self.bn_momentum = BN_EPS, BN_MOMENTUM     # the network's BatchNorm2d constants (set by the nn.Module that owns the engine)
        self.act_kind, self.act_slope = 0, 0.0                  # the units' activation (csrc/bn_act.hip ACT_*; 0 = SiLU), see set_activation
        self.sync_bn = False
        self.process_group = None
        self.world_size = 1
        self.wg_stream = None          # side stream of the weight-gradient kernels (see backward)
        self.wgrad_overlap = self.opt.wgrad_overlap
        self.comm = None               # RcclComm when the process group is RCCL-backed (the product path)
        self.comm_buckets = None       # second communicator: gradient buckets on the weight-gradient stream (comm_overlap)
        self.comm_overlap = self.opt.comm_overlap
        self.peer = None               # PeerExchange: SyncBN sums over IPC-mapped peer buffers instead of RCCL all-reduces
        self.peer_slots = None         # {(unit name, "f" | "b"): first granule of that exchange}
        self.collectives = False       # True when gradients / BN sums go through the process group (world > 1)
        self.bucket_bytes = int(self.opt.bucket_mb * (1 << 20))
        self._checked_shapes = set()   # local batch shapes already compared across the ranks (SyncBN, see forward)
        self._pending = []
        self._packed_key = None        # parameter half of freshness_key() the weight packs were made from
        self._fresh = None             # the last forward's reading of freshness_key()
        self.param_version = 0
        self.stats_version = 0         # bumped by every eager training forward (BatchNorm running statistics moved)
        self._eval_aff = None          # eval-mode BN constants of all units (flat), see _eval_affine_ptrs
        # BatchNorm modules of the conv units in program order (set by the owning nn.Module): their `training` flags make
        # the BatchNorm mode plan of a training forward (engine/bn_mode.py); None = every unit in train mode
        self.bn_modules = None
        self.bn_mode = None            # BnModePlan of the last training forward (None: never read)
        self._bn_mode_flags = None
        self._bn_eval_tables = {}      # (eval set, buffer addresses) -> device descriptor table of kodhip_bn_eval_constants
        self._nbt_inc = {}             # eval set -> per-unit num_batches_tracked increment (1 = train mode)
        self.br_stream = None         # side stream of the CSP short_conv branch in forward()
        self.head_stream = None       # side stream of the P3 / P4 head convolutions in forward()
        self.aux_stream = None        # side stream of work that only depends on the step's inputs (label assignment)
        self.branch_overlap = self.opt.branch_overlap
        self.profile = None           # list of (family, start_event, end_event, algorithmic bytes), see _t0 / _t1
        # KODHIP_DEBUG_STAMPS=1: device clock stamps at named points of the step, also inside a replayed hipGraph
        # (bench.py stamp_report): stamp_names[i] <-> stamp_buf[i]
        self.stamp_buf, self.stamp_names = None, []
        self.stamps_on = os.environ.get("KODHIP_DEBUG_STAMPS", "0") == "1"

    def set_activation(self, kind: int, slope: float = 0.0):
        """The conv units' activation (nn/graph_module.activation_code), to be set before the arenas are built.  Anything but
        SiLU runs the elementwise passes (kodhip_bn_act_*) only: the fused forms that carry SiLU's arithmetic - the
        BatchNorm-backward reduction in the data gradients' epilogue, the fused stem backward - are off."""
        import dataclasses
        self.act_kind, self.act_slope = int(kind), float(slope)
        if self.act_kind != 0:
            self.opt = dataclasses.replace(self.opt, bn_reduce_fused=False, stem_bwd_fused=False)
