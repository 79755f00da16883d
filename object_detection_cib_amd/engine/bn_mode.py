"""BatchNorm mode plan: which units of a TRAINING forward normalise with their running statistics because their BatchNorm
module is in eval mode (pure host logic, no GPU: tests/test_bn_eval_plan.py).

The usual fine-tuning recipe freezes the backbone's BatchNorm with ``net.train(); net.backbone.eval()``.  torch then
treats such a unit ("eval unit") inside the training network like this:

* it normalises with ``running_mean`` / ``running_var``;
* it leaves ``running_mean``, ``running_var`` and ``num_batches_tracked`` untouched;
* its backward is the eval-mode one, dX = gamma * rstd * dZ, with no terms through the batch moments;
* under SyncBN it exchanges nothing.

The engine reads the modules' ``training`` flags at every training forward and rebuilds the plan only when the key (the
eval set) moves; with ``is_default`` (no eval unit) it runs the program without any of this, launch for launch.  The
backward combines this plan with the freeze plan (engine/freeze.py) in one place only: an eval unit whose gamma and beta
are both frozen needs no coefficient kernel (``coef_kind``), its coefficients come with the forward's eval constants.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import FrozenSet, List, Mapping, Sequence, Tuple

from .graph import Graph

TRAIN, EVAL, NONE = "train", "eval", "none"


@dataclass(frozen=True)
class BnModePlan:
    key: Tuple[str, ...]                 # the eval units' names, in program order
    is_default: bool                     # no eval unit: the program of a network whose BatchNorm is all in train mode
    eval_units: FrozenSet[str]
    units: Tuple[str, ...]               # every conv unit, in program order

    def is_eval(self, name: str) -> bool:
        return name in self.eval_units

    @property
    def any_train(self) -> bool:
        """some unit normalises with batch statistics (running statistics move, stats_version moves)"""
        return len(self.eval_units) < len(self.units)

    def train_mask(self) -> Tuple[int, ...]:
        """per conv unit (program order): 1 = train mode (its num_batches_tracked advances)"""
        return tuple(0 if n in self.eval_units else 1 for n in self.units)

    def stat_group(self, group: Sequence) -> List:
        """The units of a forward statistics group (a unit, or a CSP sibling pair sharing one SyncBN exchange) that take
        batch statistics: eval units have no statistics stage and no place in an exchange."""
        return [u for u in group if u.name not in self.eval_units]


def conv_units(g: Graph) -> List[str]:
    return [op.unit.name for op in g.ops if op.kind == "conv"]


def build_bn_mode_plan(g: Graph, training: Mapping[str, bool]) -> BnModePlan:
    """training: conv unit name -> its BatchNorm module's `training` flag (names missing from the map count as train)"""
    names = conv_units(g)
    ev = tuple(n for n in names if not bool(training.get(n, True)))
    return BnModePlan(ev, not ev, frozenset(ev), tuple(names))


def coef_kind(plan: BnModePlan, fz, name: str) -> str:
    """How backward forms a unit's BatchNorm coefficients.  TRAIN: the batch-statistics kernels (SyncBN exchange
    included); EVAL: the eval-mode kernel (parameter gradients + coef = (gamma*rstd, 0, 0), no exchange); NONE: an eval
    unit whose gamma and beta are both frozen (fz: the active freeze plan or None) - its coefficients were written by
    the forward's eval-constants launch, nothing runs."""
    if not plan.is_eval(name):
        return TRAIN
    if fz is not None and not any(fz.units[name].bn_trainable):
        return NONE
    return EVAL


def coef_launches(plan: BnModePlan, fz, names: Sequence[str], sync: bool) -> List[Tuple[str, Tuple[str, ...], Tuple[int, ...]]]:
    """The coefficient launches of one backward group (a unit, or [short_conv, main_conv]) under a non-default plan:
    [(kind, unit names, eval flags)] with kind "mode2" (one two-unit launch, a mode per job - only without SyncBN, whose
    train-mode units take the exchange), "eval" (one eval-mode unit) or "train" (the train-mode units of the group,
    through the existing single / paired / exchanged launches)."""
    kinds = {n: coef_kind(plan, fz, n) for n in names}
    runs = [n for n in names if kinds[n] != NONE]
    if not runs:
        return []
    if not sync and len(runs) == 2:
        if all(kinds[n] == TRAIN for n in runs):
            return [("train", tuple(runs), (0, 0))]
        return [("mode2", tuple(runs), tuple(int(kinds[n] == EVAL) for n in runs))]
    out = [("eval", (n,), (1,)) for n in runs if kinds[n] == EVAL]
    train = tuple(n for n in runs if kinds[n] == TRAIN)
    if train:
        out.append(("train", train, (0,) * len(train)))
    return out


def eval_constant_units(plan: BnModePlan, fz) -> List[Tuple[str, bool]]:
    """The descriptors of the forward's eval-constants launch: [(unit name, also write the backward coefficients)]"""
    return [(n, coef_kind(plan, fz, n) == NONE) for n in plan.units if plan.is_eval(n)]
