"""Gradient accumulation (Lightning's Trainer(accumulate_grad_batches=N); YOLOv5 train.py's `accumulate`): N micro-batches
run forward, loss and backward, one optimizer step runs on the sum of their gradients.

    window gradient = ((g1 + g2) + g3) + ... + gk       fp32, each add rounded once, in micro-batch order

which is what autograd's `.grad +=` gives.  The first micro-batch of a window is copied, not added to zero (-0.0 stays -0.0).
Every micro-batch runs with the upstream scale B / N (Lightning's `loss / accumulate_grad_batches` on the reference's
`B * (loc + cls + obj)`), also in a partial window at an epoch's end (Lightning's `is_final_batch` rule).

* `AccumulationWindow`: where in the window the next micro-batch falls - host, pure Python, importable without a GPU.
* `yolov5_accumulate`: train.py's choice of N and of the weight-decay scale for a batch size - a helper, nothing calls it.
* The device side is one kodhip_grad_accumulate launch per micro-batch (csrc/accumulate.hip) into an accumulator laid out
  like the gradient arena: `Engine.configure_accumulation`, `accumulate_grads_device`,
  `step_accumulated_device` (engine/arenas.py).  With N = 1 none of it exists.
"""
from __future__ import annotations

import operator
from typing import Tuple


def check_accumulate_grad_batches(n) -> int:
    """N as an int >= 1; ValueError for anything else (bools and floats included: 2.0 is not a count)"""
    if isinstance(n, bool):
        raise ValueError(f"accumulate_grad_batches {n!r}: expected an int >= 1")
    try:
        k = operator.index(n)
    except TypeError:
        raise ValueError(f"accumulate_grad_batches {n!r}: expected an int >= 1") from None
    if k < 1:
        raise ValueError(f"accumulate_grad_batches {n!r}: expected an int >= 1")
    return k


class AccumulationWindow:
    """Position in a window of `n` micro-batches.

    first          the next micro-batch opens a window (its gradient is copied into the accumulator)
    advance()      one micro-batch has been accumulated; True when it closed the window (the optimizer step is due)
    flush_needed   a window is open: micro-batches have been accumulated and no step has consumed them
    reset()        drop an open window (its gradients are discarded with the next copy)
    state / restore: (position,) for capture(preserve_state=True)"""

    def __init__(self, n: int = 1):
        self.n = check_accumulate_grad_batches(n)
        self.pos = 0                  # micro-batches in the open window, 0 .. n - 1

    @property
    def first(self) -> bool:
        return self.pos == 0

    @property
    def flush_needed(self) -> bool:
        return self.pos > 0

    def advance(self) -> bool:
        self.pos += 1
        if self.pos >= self.n:
            self.pos = 0
            return True
        return False

    def reset(self):
        self.pos = 0


def yolov5_accumulate(batch_size: int, nbs: int = 64) -> Tuple[int, float]:
    """YOLOv5 train.py: `accumulate = max(round(nbs / batch_size), 1)` and `weight_decay *= batch_size * accumulate / nbs`, so
    that every batch size trains at the nominal batch size `nbs`.  Returns (accumulate, weight_decay_scale)."""
    if int(batch_size) < 1 or int(nbs) < 1:
        raise ValueError(f"yolov5_accumulate: batch_size {batch_size!r}, nbs {nbs!r}: expected >= 1")
    accumulate = max(round(nbs / batch_size), 1)
    return accumulate, batch_size * accumulate / nbs
