"""Plain numpy / CPU torch references of the small kernels at both ends of the training step (csrc/misc_ops.hip): image
re-layout, weight packing, the SPPF max-pools, the nearest x2 upsample.  tests/test_hip_small_ops.py compares the kernels
with these bit for bit; tests/test_small_ops_reference.py pins every function here to torch (F.conv2d, F.max_pool2d,
F.interpolate, autograd in float64) on the CPU, so the GPU tests compare the kernels with torch's semantics and the
documented layouts (include/kodhip.h), not with a transcription of the kernel sources.  Nothing here imports the
package's kernels.

Conventions: activations are channels-last numpy arrays [B, H, W, C]; a bf16 tensor is its uint16 bit pattern
(`bf16_bits`, `bits_to_f32`); sums are formed in `dtype` (float32 like the kernels, or float64 to show that a test's
inputs make every sum exact).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


# ---------------------------------------------------------------- bf16
def bf16_bits(x) -> np.ndarray:
    """fp32 -> bf16 bit pattern (uint16), round to nearest, ties to even, by integer arithmetic on the fp32 bits: add
    0x7fff plus the lowest kept bit, drop the low half (a carry into the exponent is the correct rounding, up to inf).
    Domain: finite normal values, +-0 and +-inf; a NaN maps to some NaN (sign kept, quiet bit set).  Subnormal fp32
    inputs are NOT pinned by this reference: whether a device conversion keeps or flushes them depends on the denormal
    mode of the code that converts, which the suite cannot observe - tests keep them out of their inputs."""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    r = np.where(nan, (u >> 16) | 0x0040, r)
    return r.astype(np.uint16)


def bits_to_f32(b) -> np.ndarray:
    """bf16 bit pattern (uint16) -> the fp32 value it stands for (exact)."""
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bits_is_nan(b) -> np.ndarray:
    b = np.asarray(b, dtype=np.uint16)
    return ((b & 0x7F80) == 0x7F80) & ((b & 0x007F) != 0)


def rounded_share(total) -> float:
    """share of the elements of an fp32 / fp64 array that the rounding to bf16 changes"""
    t = np.asarray(total)
    return float(np.mean(bits_to_f32(bf16_bits(t.astype(np.float32))).astype(np.float64) != t.astype(np.float64)))


# ---------------------------------------------------------------- image re-layout
def nhwc4(x) -> np.ndarray:
    """[B, C, H, W] fp32 (C <= 4) -> [B, H, W, 4] bf16 bits, channels >= C zero (kodhip_nchw_to_nhwc4)."""
    x = np.asarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    if not 1 <= C <= 4:
        raise ValueError("1 .. 4 channels")
    out = np.zeros((B, H, W, 4), dtype=np.uint16)
    out[..., :C] = bf16_bits(x.transpose(0, 2, 3, 1))
    return out


# ---------------------------------------------------------------- weight packs
def _up(n, a=32):
    return (n + a - 1) // a * a


PLAIN, STEM, S2_CLASSES, S2_FOLDED = 0, 1, 2, 3

# 3x3 / stride 2 / pad 1: input pixel i receives tap kh from output o where i = 2 o - 1 + kh.  An even i takes kh = 1 only,
# an odd i takes kh = 0 and kh = 2: the taps of parity p along one axis, in ascending order
_S2_TAPS = ((1,), (0, 2))


def s2_class_taps(py, px):
    """(kh, kw) taps of output-pixel parity class (py, px), row-major ascending: 1, 2, 2, 4 of them"""
    return [(kh, kw) for kh in _S2_TAPS[py] for kw in _S2_TAPS[px]]


def pack_gather(descs, f_size, d_size):
    """Gather form of kodhip_pack_weights: for every element of the forward pack arena (f_size) and of the dgrad pack
    arena (d_size) the master-arena index it must hold, or -1 where it stays zero.  descs: rows of 13 integers
    {w_off, f_off, d_off, N, Cin, KH, KW, Kp, Kdp, Ntot, n_off, stem, blk_begin} (include/kodhip.h); the weight is
    master[w_off + ((n * Cin + ci) * KH + kh) * KW + kw].  Raises when an element is claimed twice or lies outside its
    arena.  Layouts:
      plain (stem 0)   f[f_off + n * Kp + tap * up32(Cin) + ci], d[d_off + ci * Kdp + tap * up32(Ntot) + n_off + n]
                       (d_off = -1: no dgrad pack), tap = kh * KW + kw;
      stem (1)         6 x 6 taps over pixel pairs, k = kh * 32 + (kw >> 1) * 8 + (kw & 1) * 4 + ci; forward pack only;
      classes (2)      forward pack as plain; dgrad: four packs [Cin][ntaps * up32(N)] one after the other in class order
                       2 py + px, holding the class's taps (`s2_class_taps`) in ascending row-major order;
      folded (3)       forward pack as plain; dgrad: row = class * Cin + ci of length 4 * up32(N),
                       k = (2 (kh == 0) + (kw == 0)) * up32(N) + n.
    """
    fg = np.full(int(f_size), -1, dtype=np.int64)
    dg = np.full(int(d_size), -1, dtype=np.int64)

    def claim(arena, pos, src, what):
        pos, src = pos.reshape(-1), src.reshape(-1)
        if pos.size == 0:
            return
        if pos.min() < 0 or pos.max() >= arena.size:
            raise ValueError(f"{what}: element outside its arena")
        if np.unique(pos).size != pos.size or (arena[pos] >= 0).any():
            raise ValueError(f"{what}: an element is claimed twice")
        arena[pos] = src

    for li, row in enumerate(np.asarray(descs, dtype=np.int64).reshape(-1, 13)):
        w_off, f_off, d_off, N, Cin, KH, KW, Kp, Kdp, Ntot, n_off, stem, _ = (int(v) for v in row)
        n, ci, kh, kw = np.indices((N, Cin, KH, KW))
        src = w_off + ((n * Cin + ci) * KH + kh) * KW + kw
        tap = kh * KW + kw
        if stem == STEM:
            if (KH, KW) != (6, 6) or Cin > 4:
                raise ValueError("stem form: 6 x 6 taps, at most 4 channels")
            claim(fg, f_off + n * Kp + kh * 32 + (kw >> 1) * 8 + (kw & 1) * 4 + ci, src, f"desc {li} forward")
            continue
        claim(fg, f_off + n * Kp + tap * _up(Cin) + ci, src, f"desc {li} forward")
        if d_off < 0:
            continue
        if stem == PLAIN:
            claim(dg, d_off + ci * Kdp + tap * _up(Ntot) + n_off + n, src, f"desc {li} dgrad")
            continue
        if (KH, KW) != (3, 3):
            raise ValueError("stride-2 forms: 3 x 3 taps")
        ns = _up(N)
        if stem == S2_CLASSES:
            base = d_off
            for py in (0, 1):
                for px in (0, 1):
                    taps = s2_class_taps(py, px)
                    for t, (a, b) in enumerate(taps):
                        m = (kh == a) & (kw == b)
                        claim(dg, base + ci[m] * (len(taps) * ns) + t * ns + n[m], src[m], f"desc {li} class {2 * py + px}")
                    base += Cin * len(taps) * ns
        elif stem == S2_FOLDED:
            cls = 2 * (kh != 1) + (kw != 1)
            k = (2 * (kh == 0) + (kw == 0)) * ns + n
            claim(dg, d_off + (cls * Cin + ci) * (4 * ns) + k, src, f"desc {li} folded")
        else:
            raise ValueError(f"desc {li}: unknown form {stem}")
    return fg, dg


def gather_bits(master, gather) -> np.ndarray:
    """the pack a gather table describes: bf16_bits(master)[gather], zero where gather < 0"""
    bits = bf16_bits(master)
    return np.where(gather >= 0, bits[np.maximum(gather, 0)], 0).astype(np.uint16)


# ---------------------------------------------------------------- max-pool K x K / stride 1 / pad K // 2
def maxpool_fwd(x, K):
    """x [B, H, W, C] float -> (values, idx byte dy * 16 + dx of the winning tap), by torch's scan
    (aten/src/ATen/native/cpu/MaxPoolKernel.cpp): row-major over the window's taps inside the image, `val > max or
    isnan(val)` replaces, the maximum starts at -inf and the index at the first tap inside the image."""
    x = np.asarray(x)
    B, H, W, C = x.shape
    r = K // 2
    if not (1 <= K <= 15 and K % 2 == 1):
        raise ValueError("odd windows 1 .. 15")
    xp = np.full((B, H + 2 * r, W + 2 * r, C), -np.inf, dtype=x.dtype)
    xp[:, r:r + H, r:r + W] = x
    best = np.full(x.shape, -np.inf, dtype=x.dtype)
    oy, ox = np.indices((H, W))
    first = (np.maximum(r - oy, 0) * 16 + np.maximum(r - ox, 0)).astype(np.uint8)
    idx = np.broadcast_to(first[None, :, :, None], x.shape).copy()
    for dy in range(K):
        for dx in range(K):
            v = xp[:, dy:dy + H, dx:dx + W]
            take = (v > best) | np.isnan(v)
            best = np.where(take, v, best)
            idx = np.where(take, np.uint8(dy * 16 + dx), idx)
    return best, idx


def maxpool_bwd_sum(dy, idx, K, base, dtype=np.float32):
    """base + sum over the outputs whose winning tap points at the element of dy, accumulated in `dtype`"""
    dy, idx = np.asarray(dy), np.asarray(idx)
    B, H, W, C = dy.shape
    r = K // 2
    acc = np.array(base, dtype=dtype, copy=True)
    g = dy.astype(dtype)
    for a in range(K):
        for b in range(K):
            # output (oy, ox) with tap (a, b) points at input (oy + a - r, ox + b - r)
            oy0, oy1 = max(0, r - a), min(H, H + r - a)
            ox0, ox1 = max(0, r - b), min(W, W + r - b)
            if oy0 >= oy1 or ox0 >= ox1:
                continue
            m = idx[:, oy0:oy1, ox0:ox1] == a * 16 + b
            acc[:, oy0 + a - r:oy1 + a - r, ox0 + b - r:ox1 + b - r] += np.where(m, g[:, oy0:oy1, ox0:ox1], 0)
    return acc


def maxpool_bwd(dy, idx, K, base) -> np.ndarray:
    """kodhip_maxpool_bwd: bf16(fp32(base) + sum of the routed dy), one rounding.  base: the fp32 shadow when one is
    given, otherwise the old bf16 dx (as fp32 values)."""
    return bf16_bits(maxpool_bwd_sum(dy, idx, K, base, np.float32))


# ---------------------------------------------------------------- nearest x2 upsample
def upsample_fwd(x) -> np.ndarray:
    """[B, H, W, C] -> [B, 2H, 2W, C]: a copy of the elements, whatever they are (bit patterns included)"""
    return np.repeat(np.repeat(np.asarray(x), 2, axis=1), 2, axis=2)


def upsample_bwd_sum(dy, accumulate, dx_old, shadow, dtype=np.float32):
    dy = np.asarray(dy).astype(dtype)
    B, H2, W2, C = dy.shape
    if accumulate:
        acc = np.array(shadow if shadow is not None else dx_old, dtype=dtype, copy=True)
    else:
        acc = np.zeros((B, H2 // 2, W2 // 2, C), dtype=dtype)
    for s in range(4):                      # (2 iy, 2 ix), (2 iy, 2 ix + 1), (2 iy + 1, 2 ix), (2 iy + 1, 2 ix + 1)
        acc = acc + dy[:, (s >> 1)::2, (s & 1)::2]
    return acc


def upsample_bwd(dy, accumulate, dx_old=None, shadow=None) -> np.ndarray:
    """kodhip_upsample2x_bwd: bf16(start + the four dy of the 2 x 2 block); start = 0 without `accumulate`, else the fp32
    shadow when given, else the old bf16 dx.  What is not the start is not read."""
    return bf16_bits(upsample_bwd_sum(dy, accumulate, dx_old, shadow, np.float32))


# ---------------------------------------------------------------- SPPF: concat of pools and its input gradient
def _sppf(x, dcat, pools):
    """pools(x64 NCHW) -> list of the concat's members; returns (concat values [B,H,W,nC], d sum(cat * dcat) / dx)"""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    cat = torch.cat(pools(xt), dim=1)
    g = torch.from_numpy(np.asarray(dcat, dtype=np.float64)).permute(0, 3, 1, 2)
    cat.backward(g)
    return cat.detach().permute(0, 2, 3, 1).numpy(), xt.grad.permute(0, 2, 3, 1).numpy()


def sppf_cascade_grad(x, k, n, dcat):
    """cat[x, p(x), p(p(x)), ...] of n pools of window k, each reading the one before"""
    def pools(xt):
        out = [xt]
        for _ in range(n):
            out.append(F.max_pool2d(out[-1], k, 1, k // 2))
        return out
    return _sppf(x, dcat, pools)


def sppf_grad(x, kernel_sizes, dcat):
    """The reference module's pooling stage (SPPFBottleneck.forward between its two convs) by CPU fp64 autograd:
    x [B, H, W, C], dcat [B, H, W, (n + 1) C] -> (concat values, input gradient).  An int is the cascade of three pools;
    a sequence is [x] + [pool_k(x) for k in kernel_sizes], every pool reading x."""
    if isinstance(kernel_sizes, int):
        return sppf_cascade_grad(x, kernel_sizes, 3, dcat)
    return _sppf(x, dcat, lambda xt: [xt] + [F.max_pool2d(xt, int(k), 1, int(k) // 2) for k in kernel_sizes])


# ---------------------------------------------------------------- test inputs shared by the CPU and the GPU tests
def halfway_values() -> np.ndarray:
    """fp32 values around exact bf16 halfway points: low half 0x7fff / 0x8000 / 0x8001 under an even and an odd upper
    half, both signs, several exponents (one pair carries into the exponent, one into inf's neighbourhood)"""
    out = []
    for upper in (0x3F80, 0x3F81, 0x3FFF, 0x4000, 0x0080, 0x0081, 0x7F7E, 0x7F7F, 0x42FF, 0x3B00):
        for low in (0x7FFF, 0x8000, 0x8001):
            for sign in (0, 0x80000000):
                out.append(sign | (upper << 16) | low)
    return np.array(out, dtype=np.uint32).view(np.float32)


def special_values() -> np.ndarray:
    """the halfway patterns, +-0, +-inf, the largest finite fp32 (rounds to inf), one NaN, and k / 255 for k = 0 .. 255"""
    k255 = (np.arange(256, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    return np.concatenate([halfway_values(),
                           np.array([0.0, -0.0, np.inf, -np.inf, np.finfo(np.float32).max, np.nan], dtype=np.float32), k255])


def dyadic(shape, rng) -> np.ndarray:
    """multiples of 2^-6 in [-4, 4] (all of them bf16 values): fp32 sums of a few hundred are exact in any order"""
    return (rng.integers(-256, 257, size=shape) / 64.0).astype(np.float32)


def tie_values(shape, rng, inf=True) -> np.ndarray:
    """values from {-1.5 .. 1.5 step 0.5}: most windows hold their maximum several times; +-inf sprinkled in"""
    x = (rng.integers(-3, 4, size=shape) / 2.0).astype(np.float32)
    x = np.where(x == 0, np.float32(0.0), x)                # (+0 only: a +0 / -0 tie is a documented deviation of the 5x5 kernel)
    if inf:
        u = rng.random(size=shape)
        x = np.where(u < 0.02, np.float32(np.inf), np.where(u > 0.95, np.float32(-np.inf), x))
    return x.astype(np.float32)


POOL_WINDOWS = (1, 3, 5, 7, 9, 11, 13, 15)
POOL_SHAPES = ((2, 1, 1, 8), (2, 3, 9, 8), (1, 5, 7, 16), (2, 6, 13, 8), (3, 13, 13, 32))      # B, H, W, C
UPSAMPLE_SHAPES = ((1, 1, 1, 8), (2, 3, 5, 16), (2, 7, 4, 8))                                  # B, H, W, C (input side)
SPPF_FORMS = (5, 3, (5, 9, 13), (3, 5, 7), (3, 7), (7,))
SPPF_SHAPE = (2, 9, 11, 8)


def pool_case(K, si):
    """(x tie-heavy with +-inf and no NaN, dy dyadic, base dyadic) of pool window K on POOL_SHAPES[si]"""
    rng = np.random.default_rng(1600000 + 1000 * K + si)        # (seeds at which every case, the 16-element one too, rounds)
    shape = POOL_SHAPES[si]
    return tie_values(shape, rng), dyadic(shape, rng), dyadic(shape, rng)


def upsample_case(si):
    """(dy dyadic [B, 2H, 2W, C], old dx dyadic, shadow dyadic) on UPSAMPLE_SHAPES[si]"""
    rng = np.random.default_rng(1050 + si)
    B, H, W, C = UPSAMPLE_SHAPES[si]
    return dyadic((B, 2 * H, 2 * W, C), rng), dyadic((B, H, W, C), rng), dyadic((B, H, W, C), rng)


def sppf_case(kernel_sizes, seed=0):
    """(x from {-1.5 .. 1.5 step 0.5} plus +-inf, gradient of the concat from {-1, 0, 1}) on SPPF_SHAPE"""
    rng = np.random.default_rng(seed)
    n = 3 if isinstance(kernel_sizes, int) else len(kernel_sizes)
    B, H, W, C = SPPF_SHAPE
    return tie_values(SPPF_SHAPE, rng), rng.integers(-1, 2, size=(B, H, W, (n + 1) * C)).astype(np.float32)
