"""Tiled-inference plan (sliced inference, as the SAHI tool does it): which views of a large image go through the network, and
the row that brings each view's boxes back into the image.  Pure host arithmetic: no GPU, no torch.

Along an axis of length n with tile side S and `o = int(S * overlap)` pixels of overlap (step = S - o): the only origin is 0
when n <= S; otherwise k * step for k = 0, 1, ... while k * step + S < n, then one final origin n - S - that is
ceil((n - S) / step) + 1 origins, never a duplicate (n = 150, S = 64, o = 16: 0, 48, 86; n = 160: 0, 48, 96).  Tiles are
ordered row-major (y outer, x inner) and are cut at scale 1; an image smaller than the tile is padded on the right and
below.  With `full_view` one more view comes last: the whole image letterboxed to S exactly as `Detector` does it, so that
objects larger than a tile are still found; it is left out when the image has one tile and max(h, w) == S (the same pixels).

Every view carries its KodLetterbox row (left, top, scale_x, scale_y, width, height) for kodhip_nms_ex: (-x0, -y0, 1, 1, w, h)
for the tile at (x0, y0), the row of `inference.letterbox_table` for the full view (the two quotients as Python doubles;
their fp32 rounding happens where the table is built).
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

GRID = 32                                                        # the network's coarsest stride: the tile is a multiple


class TileView(NamedTuple):
    full: bool                   # the letterboxed whole image (False: a tile at scale 1)
    x0: int                      # the tile's corner in the image (0, 0 for the full view)
    y0: int
    letterbox: Tuple[float, float, float, float, float, float]


class TilePlan(NamedTuple):
    h: int
    w: int
    tile: int
    overlap_px: int
    xs: Tuple[int, ...]          # tile origins along x
    ys: Tuple[int, ...]
    views: Tuple[TileView, ...]  # tiles row-major, then the full view (if any)

    @property
    def n_tiles(self) -> int:
        return len(self.xs) * len(self.ys)


def axis_origins(n: int, tile: int, overlap_px: int) -> List[int]:
    """tile origins along an axis of n pixels"""
    step = tile - overlap_px
    if step < 1:
        raise ValueError(f"overlap of {overlap_px} px leaves no step at tile {tile}")
    if n <= tile:
        return [0]
    out, k = [], 0
    while k * step + tile < n:
        out.append(k * step)
        k += 1
    out.append(n - tile)
    return out


def _py3round(v: float) -> int:
    """albumentations' py3round (geometric/functional.py): exact halves round away from zero."""
    if abs(round(v) - v) == 0.5:
        return int(2.0 * round(v / 2.0))
    return int(round(v))


def letterbox_geometry(h: int, w: int, S: int, H: Optional[int] = None, W: Optional[int] = None):
    """(new_h, new_w, pad_top, pad_left) of A.LongestMaxSize(S) followed by A.PadIfNeeded(H, W), centre position
    (kod/data/sample_reader.py:16-40); H, W None: the S x S square.  THE letterbox geometry of the package:
    data.device_pipeline.letterbox_geometry and engine.rect.rect_geometry are this function (it lives here because this
    module imports without torch)."""
    h, w, S = int(h), int(w), int(S)
    H, W = S if H is None else int(H), S if W is None else int(W)
    scale = S / float(max(w, h))
    nh, nw = (_py3round(h * scale), _py3round(w * scale)) if scale != 1.0 else (h, w)
    top = int((H - nh) / 2.0) if nh < H else 0
    left = int((W - nw) / 2.0) if nw < W else 0
    return nh, nw, top, left


_letterbox_geometry = letterbox_geometry


def tile_plan(h: int, w: int, tile: int, overlap: float = 0.2, full_view: bool = True) -> TilePlan:
    h, w, tile, overlap = int(h), int(w), int(tile), float(overlap)
    if tile < GRID or tile % GRID:
        raise ValueError(f"tile {tile}: expected a multiple of {GRID} (the network's largest stride)")
    if not 0.0 <= overlap < 1.0:
        raise ValueError(f"overlap {overlap}: expected a fraction in [0, 1)")
    if h < 1 or w < 1:
        raise ValueError(f"empty image ({h} x {w})")
    o = int(tile * overlap)
    xs, ys = axis_origins(w, tile, o), axis_origins(h, tile, o)
    views = [TileView(False, x0, y0, (-x0, -y0, 1.0, 1.0, w, h)) for y0 in ys for x0 in xs]
    if full_view and not (len(views) == 1 and max(h, w) == tile):
        nh, nw, top, left = letterbox_geometry(h, w, tile)
        if nh < 1 or nw < 1:
            raise ValueError(f"{h} x {w} letterboxes to {nh} x {nw} at {tile}")
        views.append(TileView(True, 0, 0, (left, top, w / float(nw), h / float(nh), w, h)))
    return TilePlan(h, w, tile, o, tuple(xs), tuple(ys), tuple(views))
