"""Float64 reference of the convolution operators and the number-format helpers of the exact regime.

Exact regime (tests/test_hip_conv_exact.py): integer operands that bf16 holds exactly and a reduction whose sum of
absolute products stays below 2^24.  Then every product and every fp32 partial sum is an exact integer, whatever the
summation order, the split-K order or the MFMA's internal rounding, so the result of a kernel is determined:
    forward / data gradient     bf16_rne(S)
    weight gradient             S * scale in fp32 (scale a power of two)
    accumulate (bit 0)          bf16_rne(bf16_rne(S) + prior)           two roundings
    fp32 multi-producer modes   bf16_rne(S + prior32)                   ONE rounding
and the comparison is torch.equal, without a tolerance.

Real-valued regime (tests/test_hip_ops.py): the standard bound of a sum of n exact products accumulated in fp32 in ANY
order, |fl(sum) - sum| <= gamma(n - 1) * sum |a_i b_i|; the tests use gamma(n + 2) (padding terms, slab reduction, scale)
and add the unit roundoff of the output format: bf16 has 8 significant bits, u = 2^-8 for round to nearest.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)
U16 = 2.0 ** -8           # unit roundoff of bf16: 8 significant bits


def gamma(n: int) -> float:
    return n * U32 / (1.0 - n * U32)


def _quantum(t: torch.Tensor) -> torch.Tensor:
    """Spacing of the bf16 numbers around every element of a float64 tensor (normal range; 0 -> the smallest spacing
    that matters here)."""
    _, e = torch.frexp(t)                                     # |t| = m * 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(t), e - 8)             # 8 significant bits: ulp = 2^(e - 8)


def bf16_rne(t: torch.Tensor) -> torch.Tensor:
    """float64 -> nearest bf16 (ties to even), returned as float64.  Own arithmetic, not torch's conversion: the scaled
    value t / ulp is exact in float64 (a power-of-two division) and torch.round rounds halves to even."""
    t = t.double()
    q = _quantum(t)
    return torch.round(t / q) * q


def is_bf16(t: torch.Tensor) -> torch.Tensor:
    t = t.double()
    return bf16_rne(t) == t


def is_rne_tie(t: torch.Tensor) -> torch.Tensor:
    """True where the float64 value lies exactly half way between two neighbouring bf16 numbers."""
    t = t.double()
    s = (t / _quantum(t)).abs()
    return (s - torch.floor(s)) == 0.5


def single_rounding(S: torch.Tensor, prior: torch.Tensor) -> torch.Tensor:
    """What the fp32 multi-producer modes store in dx: the fp32 sum rounded once."""
    return bf16_rne(S.double() + prior.double())


def double_rounding(S: torch.Tensor, prior: torch.Tensor) -> torch.Tensor:
    """What bf16 partial sums would give: both terms rounded, then the sum rounded."""
    return bf16_rne(bf16_rne(S) + bf16_rne(prior))


def accumulate_bf16(S: torch.Tensor, prior_bf16: torch.Tensor) -> torch.Tensor:
    """The read-modify-write form (accumulate bit 0): the partial is rounded, then the sum with dx's bf16 content."""
    return bf16_rne(bf16_rne(S) + prior_bf16.double())


def conv_ref(x, w, stride, padding, dy=None):
    """F.conv2d and its autograd in float64.  x [B,C,H,W], w [N,C,KH,KW] (any float dtype holding the operand values).
    Returns (y, dx, dw); dx, dw are None without dy."""
    xr = x.double().clone().requires_grad_(True)
    wr = w.double().clone().requires_grad_(True)
    y = F.conv2d(xr, wr, None, stride, padding)
    if dy is None:
        return y.detach(), None, None
    y.backward(dy.double())
    return y.detach(), xr.grad, wr.grad


def conv_abs(x, w, stride, padding, dy=None):
    """The same three operators on the absolute values: sum |a_i b_i| per output element (the bound tensors)."""
    return conv_ref(x.abs(), w.abs(), stride, padding, None if dy is None else dy.abs())


def int_tensor(shape, bound, gen, scale=1.0):
    """Independent integers in [-bound, bound] (times a power-of-two scale), as float32."""
    return torch.randint(-bound, bound + 1, shape, generator=gen).float() * scale


def first_mismatch(got: torch.Tensor, want: torch.Tensor, bm: int = 128, bn: int = 128) -> str:
    """Where two NHWC tensors first differ: (image, row, column, channel) and the (pixel tile, tile row, channel tile,
    tile column) it maps to for bm x bn tiles over the flattened pixel axis; the epilogue's accumulator lane of that
    element is (tile row % 32) + 32 * ((tile column % 8) // 4)."""
    ne = (got.double() != want.double()) | (torch.isnan(got.double()) != torch.isnan(want.double()))
    if not bool(ne.any()):
        return "equal"
    idx = torch.nonzero(ne)[0].tolist()
    while len(idx) < 4:
        idx.insert(0, 0)
    b, r, c, ch = idx[-4:]
    H, W = got.shape[-3], got.shape[-2]
    m = (b * H + r) * W + c
    row, col = m % bm, ch % bn
    return (f"{int(ne.sum())}/{ne.numel()} differ; first at (image {b}, row {r}, column {c}, channel {ch}): got "
            f"{got[tuple(idx)].item()!r} want {want[tuple(idx)].item()!r}; pixel {m} = tile {m // bm} row {row}, channel tile "
            f"{ch // bn} column {col}, lane {row % 32 + 32 * ((col % 8) // 4)}")
