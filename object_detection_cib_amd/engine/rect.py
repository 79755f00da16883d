"""Rectangular inference and validation (YOLOv5 detect.py's minimum-padding letterbox, val.py's `rect`): which canvas a batch
of images is letterboxed onto, and in which order a set of images forms batches.  Pure host arithmetic: no GPU, no torch.

The resize is the square letterbox's - LongestMaxSize(image_size), albumentations' rounding - so an image has the same
(nh, nw) on every canvas; only the canvas shrinks, to the smallest multiple of the network's largest stride that holds every
member of the batch, and PadIfNeeded's centre position is taken on that canvas.  A 1280 x 720 frame at image_size 640 becomes
360 x 640 on a 384 x 640 canvas: 0.60 of the square's pixels go through the network.  Sorting a dataset by aspect ratio
before it is chunked (val.py) puts images of alike shapes into one batch: 5 000 random shapes with sides 200..1200 in batches
of 16 keep 0.65 of the square's pixels sorted, all of them unsorted.

Every distinct canvas is an input shape of its own to the engine: a buffer set, and a captured graph where forwards are
graphed (engine/graphed.GraphCache bounds those).
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from .tiles import GRID, letterbox_geometry

MIN_SIDE = 64                    # the smallest input side the network is tested at


def rect_canvas(shapes: Sequence[Sequence[int]], image_size: int, stride: int = GRID, min_side: int = MIN_SIDE) -> Tuple[int, int]:
    """(H, W) of the smallest canvas for images of these (h, w): each side the largest letterboxed side rounded up to a
    multiple of `stride`, at least `min_side` and at most `image_size`"""
    shapes = [(int(h), int(w)) for h, w in shapes]
    if not shapes:
        raise ValueError("rect_canvas: expected at least one shape")
    image_size, stride = int(image_size), int(stride)
    if image_size < stride or image_size % stride:
        raise ValueError(f"image_size {image_size}: expected a multiple of {stride}")
    for h, w in shapes:
        if h < 1 or w < 1:
            raise ValueError(f"empty image ({h} x {w})")
    sizes = [letterbox_geometry(h, w, image_size)[:2] for h, w in shapes]
    side = lambda n: min(image_size, max(int(min_side), -(-n // stride) * stride))
    return side(max(nh for nh, _ in sizes)), side(max(nw for _, nw in sizes))


def rect_geometry(h: int, w: int, image_size: int, H: int, W: int) -> Tuple[int, int, int, int]:
    """(new_h, new_w, pad_top, pad_left) of A.LongestMaxSize(image_size) followed by A.PadIfNeeded(H, W), centre position;
    with H = W = image_size it is the square letterbox"""
    return letterbox_geometry(h, w, image_size, H, W)


def rect_order(shapes: Sequence[Sequence[int]]) -> np.ndarray:
    """indices that sort the images by aspect ratio h / w (val.py's order), equal ratios in the given order"""
    a = np.asarray([(int(h), int(w)) for h, w in shapes], dtype=np.float64).reshape(-1, 2)
    return np.argsort(a[:, 0] / a[:, 1], kind="stable")


def rect_batches(shapes: Sequence[Sequence[int]], image_size: int, batch_size: int, sort: bool = True) -> List[Tuple[List[int], int, int]]:
    """[(indices, H, W)]: consecutive chunks of `batch_size` images in `rect_order` (sort=False: in the given order), each
    with the `rect_canvas` of its members"""
    if int(batch_size) < 1:
        raise ValueError(f"batch_size {batch_size}: expected >= 1")
    shapes = [(int(h), int(w)) for h, w in shapes]
    order = rect_order(shapes).tolist() if sort else list(range(len(shapes)))
    out = []
    for i in range(0, len(order), int(batch_size)):
        idx = order[i:i + int(batch_size)]
        out.append((idx, *rect_canvas([shapes[k] for k in idx], image_size)))
    return out


def pixel_share(plan: Sequence[Tuple[Sequence[int], int, int]], image_size: int) -> float:
    """pixels per image of the plan's canvases over those of as many image_size x image_size batches (every batch counted
    full: a partial one is padded to the batch size)"""
    return sum(H * W for _, H, W in plan) / float(len(plan) * int(image_size) ** 2) if len(plan) else 1.0
