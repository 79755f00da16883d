"""Freeze plan: which gradients a training step must compute when some parameters are frozen (pure host logic, no GPU:
tests/test_freeze_plan.py).

torch's rules for fine-tuning (a frozen backbone, a frozen stem, ...): a tensor with ``requires_grad=False`` gets no
``.grad``, ``torch.optim.SGD`` skips it, and autograd computes no gradient that no trainable tensor needs.  Applied to the
static op list of engine/graph.py:

* a value REQUIRES GRAD when a trainable tensor lies upstream of it in the forward program (through conv units, concat
  views, pools, upsamples and residual adds);
* ``needs_in_grad``: the unit's input requires grad, so its data gradient must be formed;
* ``needs_out_grad``: the unit's own tensors are trainable or its input requires grad - its BatchNorm backward runs.
  Units without it form the "no-grad region": backward does nothing there.

The engine reads the flags from the parameters at every training forward and rebuilds the plan only when the key moves;
with ``is_default`` (everything trainable) it runs the unfrozen program launch for launch.  BatchNorm modules in eval mode
inside a training network are not part of this plan: engine/bn_mode.py plans them, and the backward combines the two
only where an eval unit's gamma and beta are both frozen (no coefficient kernel then).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple

from .graph import Graph, View, head_param

HEAD_KEYS = ("box", "obj", "cls")


@dataclass(frozen=True)
class UnitFreeze:
    w_trainable: bool            # conv weight ('<unit>.0.weight')
    bn_trainable: Tuple[bool, bool]   # BatchNorm (gamma, beta)
    needs_out_grad: bool
    needs_in_grad: bool
    res_grad: bool               # the residual input requires grad (the pass-through of dA is needed)

    @property
    def trainable(self) -> bool:
        return self.w_trainable or any(self.bn_trainable)


@dataclass(frozen=True)
class HeadFreeze:
    w_trainable: Tuple[bool, bool, bool]     # box / obj / cls weights
    b_trainable: Tuple[bool, bool, bool]     # box / obj / cls biases
    needs_out_grad: bool
    needs_in_grad: bool


@dataclass(frozen=True)
class FreezePlan:
    key: tuple
    is_default: bool
    units: Dict[str, UnitFreeze]
    heads: Dict[str, HeadFreeze]
    op_in_grad: Tuple[bool, ...]             # per graph op: its input view requires grad (its backward write is needed)
    trainable: Tuple[str, ...]               # trainable parameter names, in the order given
    frozen: Tuple[str, ...]
    has_inputs: bool = False                 # a sub-network graph: backward also forms its inputs' gradient

    @property
    def any_trainable(self) -> bool:
        return bool(self.trainable)

    def require_trainable(self):
        if not self.trainable and not self.has_inputs:
            raise RuntimeError("element 0 of tensors does not require grad and does not have a grad_fn: every parameter "
                               "of the network is frozen (requires_grad=False)")

    def unit_runs(self, u) -> bool:
        """backward touches this conv unit (its BatchNorm backward, or the pass-through of dA into its residual)"""
        f = self.units[u.name]
        return f.needs_out_grad or f.res_grad


def unit_param_names(u) -> Tuple[str, str, str]:
    return (u.name + ".0.weight", u.name + ".1.weight", u.name + ".1.bias")


class _Flags:
    """requires-grad flag per channel range of every buffer, filled in forward order"""

    def __init__(self):
        self.iv: Dict[str, List[Tuple[int, int, bool]]] = {}

    def set(self, v: View, flag: bool):
        self.iv.setdefault(v.buf.name, []).append((v.coff, v.coff + v.C, flag))

    def get(self, v: Optional[View]) -> bool:
        if v is None:
            return False
        lo, hi = v.coff, v.coff + v.C
        return any(f and a < hi and lo < b for a, b, f in self.iv.get(v.buf.name, ()))


def build_freeze_plan(g: Graph, requires_grad: Mapping[str, bool]) -> FreezePlan:
    """requires_grad: parameter name -> flag (names missing from the map count as trainable).  The inputs of a
    sub-network graph (Graph.inputs) count as requiring grad: its backward returns their gradient; the whole network's
    image never does."""
    rg = lambda n: bool(requires_grad.get(n, True))
    fl = _Flags()
    for v in g.inputs:
        fl.set(v, True)
    units: Dict[str, UnitFreeze] = {}
    heads: Dict[str, HeadFreeze] = {}
    op_in: List[bool] = []
    for op in g.ops:
        if op.kind == "conv":
            u = op.unit
            wn, gn, bn = unit_param_names(u)
            ing = False if u.stem else fl.get(u.src)
            resg = fl.get(u.residual)
            own = (rg(wn), (rg(gn), rg(bn)))
            out = own[0] or any(own[1]) or ing
            units[u.name] = UnitFreeze(own[0], own[1], out, ing, resg)
            fl.set(u.dst, out or resg)
            op_in.append(ing)
        elif op.kind == "head":
            h = op.unit
            ing = fl.get(h.src)
            w = tuple(rg(head_param(h, k, "weight")) for k in HEAD_KEYS)
            b = tuple(rg(head_param(h, k, "bias")) for k in HEAD_KEYS)
            heads[h.name] = HeadFreeze(w, b, any(w) or any(b) or ing, ing)
            op_in.append(ing)
        else:                                  # pool / up: pass-through of the gradient
            ing = fl.get(op.src)
            fl.set(op.dst, ing)
            op_in.append(ing)
    names = []
    for op in g.ops:
        if op.kind == "conv":
            names.extend(unit_param_names(op.unit))
        elif op.kind == "head":
            names.extend(head_param(op.unit, k, w) for w in ("weight", "bias") for k in HEAD_KEYS)
    trainable = tuple(n for n in names if rg(n))
    frozen = tuple(n for n in names if not rg(n))
    key = frozen
    default = not frozen
    return FreezePlan(key, default, units, heads, tuple(op_in), trainable, frozen, bool(g.inputs))


def trainable_span(unit_starts, plan: FreezePlan, layout: Mapping[str, Tuple[int, int]]) -> int:
    """Index of the first exec unit (conv units, then heads, as in Engine.unit_starts) that holds a trainable tensor:
    gradient buckets tile the arena from that unit's start to its end.  -1 when nothing is trainable."""
    first = min((layout[n][0] for n in plan.trainable), default=None)
    if first is None:
        return -1
    i = 0
    while i + 1 < len(unit_starts) and unit_starts[i + 1] <= first:
        i += 1
    return i


class UnitLaunch(NamedTuple):
    """What backward launches for one conv unit of a group (BackwardPass.unit)"""
    dgrad: str                   # "own" | "skip" (its main_conv's dual launch covers it) | "dual" | "none" (nobody needs it)
    partner: object              # the short_conv a "dual" data gradient also serves, else None
    dual_w: bool                 # the pair's weight gradients are one launch
    w_grad: bool                 # the weight gradient is needed
    res_grad: bool               # the residual pass-through is needed


def group_launches(group: Sequence, plan: Optional[FreezePlan], dual, wg_dual: bool) -> List[Optional[UnitLaunch]]:
    """The backward launches of one unit group ([unit] or [short_conv, main_conv]), one entry per unit in group order;
    None = the unit lies outside the plan's grad region and launches nothing (its gradient-bucket tick stays, in order).
    plan None = the default plan (everything trainable): the same answer without a plan object.  dual: the main_convs
    that have a dual data gradient (engine/plan.py plan_dual_dgrads); wg_dual: the pair has a dual weight gradient.  The
    pair's dual forms are used only when both partners run them - one data gradient when the shared input needs a
    gradient, one weight gradient when both weights are trainable - and fall back to the single forms otherwise."""
    if plan is None:
        flags = [UnitFreeze(True, (True, True), True, not u.stem, u.residual is not None) for u in group]
    else:
        flags = [plan.units[u.name] for u in group]
    runs = [i for i, f in enumerate(flags) if f.needs_out_grad or f.res_grad]
    is_dual = dual_w = False
    if len(runs) == 2:
        is_dual = flags[0].needs_in_grad and group[1].name in dual
        dual_w = is_dual and wg_dual and flags[0].w_trainable and flags[1].w_trainable
    elif len(group) == 2 and len(runs) == 1:
        # a CSP entry pair reads one full buffer: the partner outside the grad region means it needs no data gradient
        assert not flags[runs[0]].needs_in_grad, (group[0].name, group[1].name)
    out: List[Optional[UnitLaunch]] = []
    for i, f in enumerate(flags):
        if i not in runs:
            out.append(None)
        elif is_dual:
            out.append(UnitLaunch("skip" if i == 0 else "dual", group[0] if i == 1 else None, dual_w, f.w_trainable, f.res_grad))
        else:
            out.append(UnitLaunch("own" if f.needs_in_grad else "none", None, dual_w, f.w_trainable, f.res_grad))
    return out
