"""Exponential moving average of the weights (YOLOv5 utils/torch_utils.py ModelEMA, on by default in train.py, which
validates, checkpoints and deploys `ema.ema`, never the raw weights).

    d = decay * (1 - exp(-updates / tau))          after updates += 1
    v *= d; v += (1 - d) * model[k]                for every floating-point entry of the state dict

The EMA lives BESIDE the training step, never inside it: masters and BatchNorm running statistics are flat arenas
(engine/arenas.py: p_arena, rm_arena, rv_arena), the shadow copies are laid out the same way, and one update is one
kodhip_ema_update launch over the three pairs (csrc/ema.hip) issued after the step - after the replay when the step is a captured
graph.  With no ModelEMA the step issues exactly the launches it always did.

Rounding contract: fp32, every operation rounded on its own, e = fl(fl(e * d) + fl(omd * m)) with d = float32(d) and
omd = float32(1.0 - d), the difference formed in double first - which is what torch computes for `v *= d; v += (1 - d) * m` on
fp32 tensors with a Python double d.  float32(1 - d) and 1 - float32(d) differ (0.36794266 against 0.36794263 at updates = 2000),
so both coefficients are formed here, on the host, and the kernel takes two arguments.

Importable without a GPU (ema_decay / ema_coefficients are host arithmetic); a ModelEMA needs the HIP network's engine and
there is no CPU fallback.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from collections import OrderedDict
from typing import Dict, Tuple

import numpy as np


def ema_decay(updates, decay: float = 0.9999, tau: float = 2000.0) -> float:
    """decay * (1 - exp(-updates / tau)) in Python doubles: YOLOv5's ramp, so that the first updates follow the weights"""
    return decay * (1 - math.exp(-updates / tau))


def ema_coefficients(updates, decay: float = 0.9999, tau: float = 2000.0) -> Tuple[np.float32, np.float32]:
    """(float32(d), float32(1.0 - d)) - the two arguments of kodhip_ema_update"""
    d = ema_decay(updates, decay, tau)
    return np.float32(d), np.float32(1.0 - d)


class ModelEMA:
    """ModelEMA(net) for a HIP network (Yolov5Network, or any module that owns an engine).  Owns shadow arenas laid out as the
    engine's p_arena / rm_arena / rv_arena, initialised as copies, and a copy of nbt_arena: as in YOLOv5 the non-floating
    entries (num_batches_tracked) are those of the network when the EMA was made or last loaded; update() never touches them.

    update()        updates += 1, then ONE launch on the current stream; no device value is read on the host
    state_dict()    the network's keys holding the EMA values (a weight file load_checkpoint reads as a bare state dict)
    applied()       context manager: the averaged weights are IN the network (one swap launch in, one out) - for validation
                    or a Detector; on exit the network's bits are exactly what they were

    Data parallel: every rank holds the same parameters after the all-reduced step, so every rank forms the same parameter
    EMA without a collective.  Without SyncBN the running statistics - and hence their averages - are per rank, as the raw
    ones already are."""

    def __init__(self, net, decay: float = 0.9999, tau: float = 2000.0, updates: int = 0):
        import torch
        if not callable(getattr(net, "engine", None)) or not hasattr(net, "_engine"):
            raise TypeError(f"ModelEMA needs a HIP network that owns an engine (Yolov5Network), got {type(net).__name__}: "
                            "the update is a HIP kernel over the engine's arenas and has no CPU fallback")
        self.net = net
        self.eng = eng = net.engine()
        self.decay, self.tau, self.updates = float(decay), float(tau), int(updates)
        self._applied = False
        # every entry of the state dict: where it lives in the shadow (kind, offset, numel)
        units = {u.name: i for i, u in enumerate(eng.exec_units)}
        self._index: Dict[str, Tuple[str, int, int]] = OrderedDict()
        self._shapes: Dict[str, tuple] = {}
        for k, v in net.state_dict().items():
            mod, _, leaf = k.rpartition(".")
            unit = mod[:-2] if mod.endswith(".1") else None
            if k in eng.layout:
                self._index[k] = ("p",) + tuple(eng.layout[k])
            elif unit in units and leaf in ("running_mean", "running_var"):
                self._index[k] = ("rm" if leaf == "running_mean" else "rv", eng.rs_layout[unit], v.numel())
            elif unit in units and leaf == "num_batches_tracked":
                self._index[k] = ("nbt", units[unit], 1)
            else:           # (a floating-point entry outside the three arenas would silently stay un-averaged)
                raise AssertionError(f"ModelEMA: state_dict entry {k!r} ({v.dtype}) is not bound into an engine arena")
            self._shapes[k] = tuple(v.shape)
        self._model = {"p": eng.p_arena, "rm": eng.rm_arena, "rv": eng.rv_arena, "nbt": eng.nbt_arena}
        self._shadow = {k: t.detach().clone() for k, t in self._model.items()}
        for k in ("p", "rm", "rv"):
            assert self._model[k].dtype == torch.float32 and self._model[k].is_contiguous()
        assert eng.nbt_arena.dtype == torch.int64
        # the by-value segment tables of the two launches (host arrays of device pointers and counts).  The update covers
        # the three float arenas; the swap also exchanges num_batches_tracked, as 2 x 32-bit words per counter.
        order = ("p", "rm", "rv", "nbt")
        words = [self._model[k].numel() * (2 if k == "nbt" else 1) for k in order]
        self._tab_model = (C.c_void_p * 4)(*[self._model[k].data_ptr() for k in order])
        self._tab_shadow = (C.c_void_p * 4)(*[self._shadow[k].data_ptr() for k in order])
        self._tab_numel = (C.c_long * 4)(*words)

    # ------------------------------------------------------------------ the two launches
    @property
    def is_applied(self) -> bool:
        return self._applied

    def _check(self, what: str):
        if self._applied:
            raise RuntimeError(f"ModelEMA.{what} while applied(): the network holds the averaged weights and the shadow the "
                               "raw ones; leave the applied() block first")
        if getattr(self.net, "_engine", None) is not self.eng:
            raise RuntimeError("ModelEMA: the network has a new engine (moved to another device?); build a new ModelEMA")

    def update(self):
        """One EMA step from the network's current parameters and running statistics (call after every optimizer step)."""
        from .. import _lib
        self._check("update()")
        self.updates += 1
        d, omd = ema_coefficients(self.updates, self.decay, self.tau)
        _lib.check(self.eng.lib.kodhip_ema_update(self._tab_model, self._tab_shadow, self._tab_numel, 3, float(d), float(omd),
                                                  self.eng._stream()), "ema_update")

    def _swap(self):
        from .. import _lib
        _lib.check(self.eng.lib.kodhip_ema_swap(self._tab_model, self._tab_shadow, self._tab_numel, 4, self.eng._stream()),
                   "ema_swap")
        # written through raw pointers: the freshness key must move (weight packs, eval-mode BatchNorm constants)
        self.eng.invalidate_eval_constants()

    @contextlib.contextmanager
    def applied(self):
        """Inside, the network computes with the averaged weights (`net.state_dict()` holds them, a Detector or a captured
        eval forward over the network sees them); update(), a nested applied() and loading are refused.  On exit the
        network's bits are exactly what they were."""
        self._check("applied()")
        self._swap()
        self._applied = True
        try:
            yield self.net
        finally:
            self._swap()
            self._applied = False

    # ------------------------------------------------------------------ state
    def _view(self, key: str):
        kind, off, n = self._index[key]
        t = self._shadow[kind]
        return t[off] if kind == "nbt" else t[off:off + n]

    def state_dict(self) -> "OrderedDict":
        """The network's keys (360 for yv5s) holding the EMA values, as copies on the device."""
        self._check("state_dict()")
        return OrderedDict((k, self._view(k).clone().view(self._shapes[k])) for k in self._index)

    def load_state_dict(self, sd):
        """Loads what state_dict() returned (or any state dict of the same network) into the shadow."""
        import torch
        self._check("load_state_dict()")
        missing, extra = [k for k in self._index if k not in sd], [k for k in sd if k not in self._index]
        if missing or extra:
            raise KeyError(f"ModelEMA.load_state_dict: missing keys {missing[:4]}, unexpected keys {extra[:4]}")
        with torch.no_grad():
            for k in self._index:
                dst = self._view(k)
                src = sd[k].to(device=dst.device, dtype=dst.dtype)
                if src.numel() != dst.numel():
                    raise ValueError(f"ModelEMA.load_state_dict: {k}: {tuple(sd[k].shape)} does not fit")
                dst.copy_(src.reshape(dst.shape))

    def copy_to(self, other_net):
        """Loads the EMA values into another network of the same architecture; returns it."""
        other_net.load_state_dict(self.state_dict())
        return other_net

    def ema_state_dict(self) -> dict:
        """what a checkpoint keeps (save_checkpoint(ema_state=...)): the counters and the EMA state dict on the host"""
        return {"updates": self.updates, "decay": self.decay, "tau": self.tau,
                "state_dict": OrderedDict((k, v.cpu()) for k, v in self.state_dict().items())}

    def load_ema_state_dict(self, state: dict):
        self.load_state_dict(state["state_dict"])
        self.updates, self.decay, self.tau = int(state["updates"]), float(state["decay"]), float(state["tau"])
