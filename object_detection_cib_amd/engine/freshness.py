"""Freshness of what the engine derives from parameters and BatchNorm buffers (pure host logic, CPU-testable).

The engine keeps derived copies: the bf16 weight packs (engine/arenas.py pack_weights) and the eval-mode BatchNorm
constants (engine/forward.py _eval_affine_ptrs).  Both are rebuilt when the key below moved.  The key has to see every
way the values can change:

* the engine's own writers go through raw pointers (fused SGD, the running-statistic update, a graph replay) and bump the
  engine's counters `param_version` / `stats_version` by hand;
* an edit of a whole arena (`eng.p_arena.copy_(ema)`) moves that arena's `_version`;
* an edit through the module's own tensors - `p.mul_()` under no_grad, `nn.init.*_`, a torch.optim step, `load_state_dict`,
  `bn.reset_running_stats()` - moves the `_version` of that Parameter / buffer and of nothing else: a tensor re-pointed
  into an arena with `p.data = arena[...]` keeps its own version counter;
* an edit through `p.data` (`p.data.copy_(w)`, `p.data.clamp_()`) moves no counter at all in stock torch: `.data` hands out
  a tensor with a fresh counter.  `track_data_edits` therefore gives the bound Parameters a `.data` that shares theirs.
  BatchNorm buffers are plain tensors and stay as they are: an edit through `buffer.data` needs
  `Engine.invalidate_eval_constants()`.

Version counters only ever grow, so a sum moves exactly when one of its terms does.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch
import torch.nn as nn


class _ArenaParameter(nn.Parameter):
    """nn.Parameter whose `.data` is `detach()`: the same storage, requires_grad False, but the version counter shared
    with the Parameter, so an in-place edit through `.data` is seen by freshness_key.  Assigning `p.data = t` is torch's.
    (The network is one autograd node that saves no parameter, so no backward ever objects to such an edit.)"""

    @property
    def data(self):
        return self.detach()

    @data.setter
    def data(self, value):
        torch.Tensor.data.__set__(self, value)


def track_data_edits(p: nn.Parameter) -> nn.Parameter:
    """Make in-place edits through `p.data` move `p._version` (see _ArenaParameter).  Only exact nn.Parameters are
    touched; the object, its storage, its hooks and its place in modules and optimizers stay the same."""
    if type(p) is nn.Parameter:
        p.__class__ = _ArenaParameter
    return p


def version_sum(tensors: Sequence[torch.Tensor]) -> int:
    return sum([t._version for t in tensors])


def freshness_key(param_version: int, stats_version: int, param_tensors: Sequence[torch.Tensor],
                  stat_tensors: Sequence[torch.Tensor]) -> Tuple[int, int]:
    """(parameter half, statistics half).  param_tensors: the parameter arena and every Parameter bound into it;
    stat_tensors: the running-mean / running-variance arenas and every buffer bound into them.  The weight packs depend on
    the first half alone (a training forward moves only the second); the eval-mode BatchNorm constants on both."""
    return (param_version + version_sum(param_tensors), stats_version + version_sum(stat_tensors))
