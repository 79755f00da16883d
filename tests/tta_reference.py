"""Plain references of test-time augmentation (YOLOv5 models/yolo.py::_forward_augment, utils/torch_utils.py::scale_img)
and the constructed inputs that tests/test_tta_reference.py (CPU) and tests/test_hip_tta.py (GPU) run.

Nothing here touches the HIP library or the package's own planner.  Written from the definition, not from the kernels:

* `tta_plan_ref`     the three views (ratio, flip) = (1, no), (0.83, left-right), (0.67, no): a scaled view is
                     int(H * ratio) x int(W * ratio) in a canvas of ceil(H * ratio / 32) * 32 rows (columns alike); the first
                     view loses its last pyramid level, the last view its first; row offsets in (view, level, ...) order.
* `scale_view_ref`   numpy fp32, every operation rounded on its own, in the prescribed order: flip, then per axis
                     scale = fp32(n_in) / fp32(n_out), src = max(fp32(fp32(dst + .5) * scale) - .5, 0), i0 = int(src),
                     i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1, out = hy0 * (wx0 * a + wx1 * b) + hy1 * (wx0 * c +
                     wx1 * d); the rest of the canvas is fp32(0.447).  ratio = 1: the (flipped) batch itself.  The device
                     kernel is held to this bit for bit; tests/test_tta_reference.py anchors it to torch's CPU
                     F.interpolate + F.pad within ulp32(src_y) + ulp32(src_x) <= 2 * 2^-14 (sizes below 1024, pixels in [0, 1]).
* `descale_ref`      fp64, on `val_reference.decode_ref` at the view's own shape: cx, cy, w, h divided by fp32(ratio),
                     cx = W - cx for a flipped view, corners again.  All levels of the view (untrimmed).
* `descale_f32`      the same in numpy fp32 in the operation order the device documents (IEEE division, corners cx -+ .5 * w):
                     what a de-scaled decode costs in fp32, measured against `descale_ref` below.
* `merge_ref`        the trim and the concatenation of three untrimmed per-view tensors.

Tolerance.  The box error of a row is taken in fp32 ulps of max(|cx|, |cy|, w, h, W) of the de-scaled row (W: a flipped
centre is a difference from the full width).  `descale_f32` against `descale_ref` over the 128 / 192 / 640 plans, nc 1 / 3,
B 1 / 2, with val_reference.decode_case's logits (+-20, +-88, +-100, +-inf in every field), measured on an x86-64 host:
at most 2.80 ulp.  Recorded rounded UP to 3 ulp; the CPU test holds the restatement to the recorded value, the device gets
twice it (another expf may differ by 1 - 2 ulp), as val_reference does for the plain decode.  Scores are not touched by the
de-scaling: DECODE_SCORE_REL as it stands.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

import val_reference as V

TTA_BOX_ULP_MEASURED = 3.0
TTA_BOX_ULP = 2 * TTA_BOX_ULP_MEASURED                  # 6 ulp32, the device tolerance
VIEWS = ((1.0, False), (0.83, True), (0.67, False))
PAD = np.float32(0.447)
RESIZE_BOUND = 2 * 2.0 ** -14                           # ulp32(src_y) + ulp32(src_x), sizes below 1024, pixels in [0, 1]
PLAN_SIZES = ((128, 128), (192, 192), (64, 128))        # (H, W) of the GPU cases; 640 x 640 joins them on the CPU


class ViewRef(NamedTuple):
    ratio: float
    flip: bool
    h: int
    w: int
    Hp: int
    Wp: int
    levels: tuple         # which of the three pyramid levels contribute
    row_offset: int
    rows: int


def level_rows_ref(Hp, Wp):
    return [3 * (Hp // s) * (Wp // s) for s in V.STRIDES]


def tta_plan_ref(H, W):
    """-> (views, merged rows)"""
    views, off = [], 0
    for i, (ratio, flip) in enumerate(VIEWS):
        if ratio == 1.0:
            h, w, Hp, Wp = H, W, H, W
        else:
            h, w = int(H * ratio), int(W * ratio)
            Hp, Wp = math.ceil(H * ratio / 32) * 32, math.ceil(W * ratio / 32) * 32
        levels = tuple(l for l in range(3) if not (i == 0 and l == 2) and not (i == len(VIEWS) - 1 and l == 0))
        rows = sum(level_rows_ref(Hp, Wp)[l] for l in levels)
        views.append(ViewRef(ratio, flip, h, w, Hp, Wp, levels, off, rows))
        off += rows
    return views, off


# ------------------------------------------------------------------------------------------------------ view input
def _axis(n_in, n_out):
    f = np.float32
    scale = f(n_in) / f(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    src = np.maximum((dst + f(0.5)) * scale - f(0.5), f(0))
    i0 = src.astype(np.int64)
    assert int(i0.max()) <= n_in - 1
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float32)
    l0 = f(1) - l1
    assert src.dtype == l0.dtype == l1.dtype == np.float32
    return i0, i1, l0, l1


def resize_ref(x, h, w):
    """x [B, 3, H, W] fp32 -> [B, 3, h, w] fp32, the prescribed arithmetic"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    y0, y1, hy0, hy1 = _axis(x.shape[2], h)
    x0, x1, wx0, wx1 = _axis(x.shape[3], w)
    r0, r1 = x[:, :, y0, :], x[:, :, y1, :]
    top = wx0 * r0[..., x0] + wx1 * r0[..., x1]
    bot = wx0 * r1[..., x0] + wx1 * r1[..., x1]
    out = hy0[:, None] * top + hy1[:, None] * bot
    assert out.dtype == np.float32
    return out


def scale_view_ref(x, view):
    """x [B, 3, H, W] fp32 numpy -> the view's network input [B, 3, Hp, Wp] fp32"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    if view.flip:
        x = x[..., ::-1]
    if view.ratio == 1.0:
        return np.ascontiguousarray(x)
    out = np.full(x.shape[:2] + (view.Hp, view.Wp), PAD, np.float32)
    out[:, :, :view.h, :view.w] = resize_ref(x, view.h, view.w)
    return out


def scale_view_torch(x, view):
    """the same through torch's CPU F.interpolate + F.pad (what YOLOv5's scale_img calls)"""
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(x)[..., ::-1] if view.flip else x))
    if view.ratio == 1.0:
        return t.numpy()
    t = F.interpolate(t, size=(view.h, view.w), mode="bilinear", align_corners=False)
    return F.pad(t, [0, view.Wp - view.w, 0, view.Hp - view.h], value=0.447).numpy()


def image_batch(B, H, W, seed):
    """pixels in [0, 1) with exact 0 and 1 planted in the corners that a flip exchanges"""
    x = np.random.default_rng(seed).random((B, 3, H, W), dtype=np.float32)
    x[:, :, 0, 0], x[:, :, 0, -1], x[:, :, -1, 0], x[:, :, -1, -1] = 0.0, 1.0, 1.0, 0.0
    return x


# ---------------------------------------------------------------------------------------------- predictions -> full frame
def _cxcywh(box):
    return (box[..., 0] + box[..., 2]) / 2, (box[..., 1] + box[..., 3]) / 2, box[..., 2] - box[..., 0], box[..., 3] - box[..., 1]


def descale_ref(raws, view, W):
    """three [B, 3, h, w, 5+nc] fp32 head tensors of the view's shape -> [B, all rows of the view, 5+nc] fp64 in the full frame"""
    d = V.decode_ref(raws, V.STRIDES, V.ANCHORS, view.Wp, view.Hp).numpy().copy()
    s = float(np.float32(view.ratio))
    cx, cy, w, h = (v / s for v in _cxcywh(d[..., :4]))
    if view.flip:
        cx = float(W) - cx
    d[..., 0], d[..., 1], d[..., 2], d[..., 3] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    return d


def descale_f32(raws, view, W):
    """the fp32 restatement, every operation rounded on its own: sigmoid = 1 / (1 + exp(-x)), cx = (sx * 2 + gx - .5) * stride,
    w = (sw * 2) * (sw * 2) * anchor, each of cx, cy, w, h divided by fp32(ratio), cx = fp32(W) - cx when flipped, corners
    cx -+ .5 * w.  -> [B, all rows of the view, 5+nc] fp32"""
    f = np.float32
    out = []
    with np.errstate(over="ignore"):
        for raw, stride, anc in zip(raws, V.STRIDES, V.ANCHORS):
            r = np.asarray(raw, dtype=np.float32)
            B, A, h, w, P = r.shape
            sg = f(1) / (f(1) + np.exp(-r))
            gy = np.arange(h, dtype=np.float32).reshape(1, 1, h, 1)
            gx = np.arange(w, dtype=np.float32).reshape(1, 1, 1, w)
            aw = np.asarray([a[0] for a in anc], np.float32).reshape(1, A, 1, 1)
            ah = np.asarray([a[1] for a in anc], np.float32).reshape(1, A, 1, 1)
            cx = (sg[..., 0] * f(2) + gx - f(0.5)) * f(stride)
            cy = (sg[..., 1] * f(2) + gy - f(0.5)) * f(stride)
            bw = (sg[..., 2] * f(2)) * (sg[..., 2] * f(2)) * aw
            bh = (sg[..., 3] * f(2)) * (sg[..., 3] * f(2)) * ah
            out.append((cx, cy, bw, bh, sg[..., 4:]))
    return np.concatenate([_finish_f32(cx, cy, bw, bh, sc, view, W) for cx, cy, bw, bh, sc in out], 1)


def _finish_f32(cx, cy, bw, bh, scores, view, W):
    f = np.float32
    s = f(view.ratio)
    cx, cy, bw, bh = cx / s, cy / s, bw / s, bh / s
    if view.flip:
        cx = f(W) - cx
    box = np.stack((cx - f(0.5) * bw, cy - f(0.5) * bh, cx + f(0.5) * bw, cy + f(0.5) * bh), -1)
    d = np.concatenate((box, scores), -1)
    assert d.dtype == np.float32
    return d.reshape(d.shape[0], -1, d.shape[-1])


def merge_ref(per_view, views):
    """three untrimmed [B, all rows of view i, P] arrays -> [B, merged rows, P]: view 0 without its last level, view 2
    without its first, rows in (view, level, anchor, y, x) order"""
    parts = []
    for d, v in zip(per_view, views):
        n = level_rows_ref(v.Hp, v.Wp)
        assert d.shape[1] == sum(n)
        start = np.concatenate(([0], np.cumsum(n)))
        parts += [d[:, start[l]:start[l + 1]] for l in v.levels]
    return np.concatenate(parts, 1)


def trim_ref(d, view):
    """one untrimmed view -> its own rows of the merged tensor"""
    return merge_ref([d], [view])


def box_errors(got, ref, W):
    """got fp32 / ref fp64 [B, rows, 5+nc] arrays -> (max box error in ulp32 of the row's max(|cx|, |cy|, w, h, W), max score
    error relative beyond the FLT_MIN floor)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    cx, cy, w, h = _cxcywh(ref[..., :4])
    scale = V.ulp32(np.maximum(np.maximum(np.maximum(np.abs(cx), np.abs(cy)), np.maximum(w, h)), float(W)))
    box = float((np.abs(got[..., :4] - ref[..., :4]).max(-1) / scale).max())
    s, g = ref[..., 4:], got[..., 4:]
    over = np.maximum(np.abs(g - s) - V.FLT_MIN, 0.0)
    rel = float(np.where(over > 0, over / np.where(s != 0, np.abs(s), 1.0), 0.0).max())
    return box, rel


# ------------------------------------------------------------------------------------------------------------- cases
class TtaDecodeCase(NamedTuple):
    H: int
    W: int
    nc: int
    views: list
    rows: int
    raws: list            # per view: three [B, 3, h, w, 5+nc] fp32 head tensors of the view's shape
    facts: dict


def decode_view_case(H, W, nc, B, seed) -> TtaDecodeCase:
    """val_reference.decode_case logits (random x 2, every special value in every field) for each view's own shape"""
    views, rows = tta_plan_ref(H, W)
    raws = [V.decode_case(v.Wp, v.Hp, nc, B, seed + i).raws for i, v in enumerate(views)]
    merged = merge_ref([descale_ref(r, v, W) for r, v in zip(raws, views)], views)
    facts = dict(view_rows=[v.rows for v in views], offsets=[v.row_offset for v in views], rows=rows,
                 sizes=[(v.Hp, v.Wp) for v in views], merged_shape=merged.shape, finite=bool(np.isfinite(merged).all()),
                 first_trim=sum(level_rows_ref(views[0].Hp, views[0].Wp)) - views[0].rows,
                 last_trim=sum(level_rows_ref(views[2].Hp, views[2].Wp)) - views[2].rows)
    return TtaDecodeCase(H, W, nc, views, rows, raws, facts)


def planted_case(H, W, nc=3, B=1):
    """Every logit -20 (objectness ~ 2e-9) except ONE cell per view, off-centre at grid cell (gy, gx) = (1, 2) of the
    stride-16 level, anchor 1, whose box logits are 0 (sigmoid 1/2: the centre sits in the middle of the cell, the size is the
    anchor) and whose objectness / class-0 logits are +20.  -> (case, expected): per view the merged row index and the
    de-scaled (cx, cy, w, h) computed by hand in fp64."""
    views, rows = tta_plan_ref(H, W)
    gy, gx, an, lvl = 1, 2, 1, 1
    stride, (aw, ah) = V.STRIDES[lvl], V.ANCHORS[lvl][an]
    raws, expected = [], []
    for v in views:
        rs = [torch.full((B, 3, v.Hp // s, v.Wp // s, 5 + nc), -20.0) for s in V.STRIDES]
        rs[lvl][:, an, gy, gx, :4] = 0.0
        rs[lvl][:, an, gy, gx, 4:6] = 20.0
        raws.append(rs)
        s = float(np.float32(v.ratio))
        cx, cy = (gx + 0.5) * stride / s, (gy + 0.5) * stride / s
        if v.flip:
            cx = W - cx
        n = level_rows_ref(v.Hp, v.Wp)
        in_view = sum(n[l] for l in v.levels if l < lvl) + (an * (v.Hp // stride) + gy) * (v.Wp // stride) + gx
        expected.append(dict(row=v.row_offset + in_view, cxcywh=(cx, cy, aw / s, ah / s)))
    return TtaDecodeCase(H, W, nc, views, rows, raws, dict(cell=(gy, gx, an, lvl))), expected
