"""Plain references of multi-scale training (YOLOv5 train.py --multi-scale) that tests/test_multiscale_reference.py (CPU)
and tests/test_hip_multiscale.py (GPU) run.  Nothing here touches the HIP library or the package; written from the
definitions, not from the code under test:

* `draw_ref`          YOLOv5's draw with Python floats on random.Random(seed): S = max(H, W),
                      sz = rng.randrange(int(S * lo), int(S * hi) + gs) // gs * gs (or rng.choice(sizes)), sf = sz / S,
                      (h, w) = (H, W) if sf == 1 else ceil(x * sf / gs) * gs per axis; a new draw every `interval` steps.
* `resize_ref`        tests/tta_reference.resize_ref: the singly rounded fp32 bilinear arithmetic (the same arithmetic, up- and
                      down-scaling; its own assert keeps i0 <= n_in - 1).
* `to_pairs_ref` / `widen_pairs_ref` / `resize_pairs_ref`   the bf16 pixel-pair form [B, H, W, 4] (uint16 bit patterns, channel 3
                      zero): fp32 -> bf16 round to nearest even, bf16 -> fp32 exact.
* `scale_boxes_ref`   fp64: x * (float(w) / float(W)), y * (float(h) / float(H)), one rounded multiply each.
"""
from __future__ import annotations

import math
import random

import numpy as np

from tta_reference import image_batch, resize_ref  # noqa: F401  (re-exported)


def canvas_ref(H, W, sz, gs=32):
    S = max(H, W)
    sf = sz / S
    if sf == 1:
        return H, W
    return math.ceil(H * sf / gs) * gs, math.ceil(W * sf / gs) * gs


def draw_ref(H, W, seed, steps, scale_range=(0.5, 1.5), gs=32, interval=1, sizes=None):
    """-> [(sz, (h, w))] of `steps` consecutive steps"""
    rng = random.Random(seed)
    S = max(H, W)
    lo, hi = scale_range
    out, cur = [], None
    for k in range(steps):
        if k % interval == 0:
            sz = rng.choice(list(sizes)) if sizes is not None else rng.randrange(int(S * lo), int(S * hi) + gs) // gs * gs
            cur = (sz, canvas_ref(H, W, sz, gs))
        out.append(cur)
    return out


def bf16_bits(x):
    """fp32 array -> uint16 bf16 bit patterns, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_widen(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_pairs_ref(x):
    """[B, 3, H, W] fp32 -> [B, H, W, 4] uint16 (the memory of bf16 [B, H, W/2, 8]); channel 3 is zero"""
    x = np.asarray(x, dtype=np.float32)
    B, _, H, W = x.shape
    out = np.zeros((B, H, W, 4), np.uint16)
    out[..., :3] = bf16_bits(x.transpose(0, 2, 3, 1))
    return out


def widen_pairs_ref(p):
    """[B, H, W, 4] uint16 -> [B, 3, H, W] fp32"""
    return np.ascontiguousarray(bf16_widen(np.asarray(p)[..., :3]).transpose(0, 3, 1, 2))


def resize_pairs_ref(p, h, w):
    """pairs source -> (out_f32 [B, 3, h, w], out_pairs [B, h, w, 4] uint16)"""
    f = resize_ref(widen_pairs_ref(p), h, w)
    return f, to_pairs_ref(f)


def scale_boxes_ref(boxes, H, W, h, w):
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    sx, sy = float(w) / float(W), float(h) / float(H)
    return b * np.array([sx, sy, sx, sy], dtype=np.float64)
