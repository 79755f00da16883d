"""Test-time augmentation plan (YOLOv5 models/yolo.py::_forward_augment): which three views of a letterboxed batch go
through the network, and where each view's predictions land in the merged tensor.  Pure host arithmetic: no GPU, no torch.

Views, in this order: (ratio 1, as is), (0.83, flipped left-right), (0.67, as is).  A view that is scaled is
`int(H * ratio) x int(W * ratio)` pixels (Python doubles, utils/torch_utils.py::scale_img), placed top-left in a canvas of
`ceil(H * ratio / 32) * 32` rows and likewise columns, the rest filled with fp32(0.447).  The first view loses its last
pyramid level and the last view its first (`_clip_augmented`); rows stay in (view, level, anchor, y, x) order.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Tuple

TTA_VIEWS = ((1.0, False), (0.83, True), (0.67, False))          # (ratio, flip left-right)
TTA_PAD = 0.447                                                  # scale_img's fill (the ImageNet mean)
STRIDES = (8, 16, 32)
ANCHORS_PER_CELL = 3
GRID = 32                                                        # the network's coarsest stride: every canvas is a multiple


class TtaView(NamedTuple):
    ratio: float
    flip: bool
    h: int                # the resized image inside the canvas
    w: int
    Hp: int               # the canvas = the network's input shape for this view
    Wp: int
    level_mask: int       # bit l: pyramid level l (stride 8, 16, 32) contributes its rows
    row_offset: int       # first row of this view in the merged tensor
    rows: int             # rows this view contributes


class TtaPlan(NamedTuple):
    H: int
    W: int
    views: Tuple[TtaView, TtaView, TtaView]
    rows: int             # rows of the merged tensor

    def shapes(self):
        """the distinct (Hp, Wp) canvases, in first-use order: one engine buffer set each"""
        out = []
        for v in self.views:
            if (v.Hp, v.Wp) not in out:
                out.append((v.Hp, v.Wp))
        return out


def level_rows(Hp: int, Wp: int, level_mask: int = 7):
    """rows of each pyramid level of an Hp x Wp input (0 for a level that the mask leaves out)"""
    return [ANCHORS_PER_CELL * (Hp // s) * (Wp // s) if (level_mask >> l) & 1 else 0 for l, s in enumerate(STRIDES)]


def tta_plan(H: int, W: int) -> TtaPlan:
    H, W = int(H), int(W)
    if H < GRID or W < GRID or H % GRID or W % GRID:
        raise ValueError(f"test-time augmentation needs a batch of multiples of {GRID} pixels, got {H} x {W}")
    views, off = [], 0
    last = len(TTA_VIEWS) - 1
    for i, (ratio, flip) in enumerate(TTA_VIEWS):
        if ratio == 1.0:
            h, w, Hp, Wp = H, W, H, W
        else:
            h, w = int(H * ratio), int(W * ratio)
            Hp, Wp = math.ceil(H * ratio / GRID) * GRID, math.ceil(W * ratio / GRID) * GRID
        mask = 7 & ~(4 if i == 0 else 0) & ~(1 if i == last else 0)
        rows = sum(level_rows(Hp, Wp, mask))
        views.append(TtaView(ratio, flip, h, w, Hp, Wp, mask, off, rows))
        off += rows
    return TtaPlan(H, W, tuple(views), off)
