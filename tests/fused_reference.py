"""Cases and float64 references of the fused eval-forward epilogue (kodhip_conv_fwd_fused), shared by the GPU test
(tests/test_hip_conv_fused.py) and the CPU test of the cases' own conditions (tests/test_eval_fused_host.py).

Epilogue contract, S the fp32 accumulator of output channel n:
    z = fma(S, scale[n], shift[n])    a = act(z)    o = bf16_rne(a)    out = residual ? bf16_rne(o + r) : o

Exact regime (Identity / ReLU / LeakyReLU): integer x in [-16, 16] and w in [-8, 8], scale = +-2^-e, shift a multiple of
0.25 in [-8, 8], integer residual in [-16, 16], slope 0.125.  Where (conv(|x|, |w|) |scale| + |shift|) / 2^-5 < 2^24 and z,
act(z), bf16_rne(act(z)) + r are fp32 numbers, no fp32 operation of the kernel rounds, so the stored value is determined
and the comparison is torch.equal.

SiLU / Hardswish: the same operands (z exact in fp32, |z| <= 128); the kernel's fp32 activation carries a relative error
below DELTA = 2^-16 (the exponent argument's rounding is at most 128 log2(e) 2^-24 ~ 1.1e-5, one ulp each for v_exp_f32
and v_rcp_f32, two fp32 roundings ~ 2.4e-7 together), so the stored bf16 value is bf16_rne of the float64 activation
except where that lies within DELTA |a| of a rounding boundary; there the neighbouring bf16 number is allowed too.
"""
from __future__ import annotations

import functools

import torch

from conv_reference import _quantum, bf16_rne, conv_abs, conv_ref, int_tensor, is_bf16

ACT_SILU, ACT_RELU, ACT_LEAKY, ACT_HARDSWISH, ACT_IDENTITY = 0, 1, 2, 3, 4
SLOPE = 0.125
DELTA = 2.0 ** -16
LIMIT = float(2 ** 24)
EXACT_ACTS = (ACT_IDENTITY, ACT_RELU, ACT_LEAKY)

# id: ((B, Cin, H, W, N, k, s, p), (bm, bn, row3) of the forward plan, input read from a channel slice, persistent blocks)
CASES = {
    # K tail (16 -> 32), one ragged 128-pixel tile, 32-column tile
    "pw16_n32": ((2, 16, 9, 7, 32, 1, 1, 0), (128, 32, 0), True, False),
    # 1x1 with a K tail (48 -> 64), two channel tiles
    "pw48_n64": ((2, 48, 10, 6, 64, 1, 1, 0), (128, 32, 0), False, False),
    # ragged second channel tile (160 = 64 + 64 + 32)
    "pw512_n160": ((1, 512, 9, 7, 160, 1, 1, 0), (128, 64, 0), False, False),
    # ROW3, rows shorter than a DMA piece
    "r3_32_n32": ((2, 32, 10, 6, 32, 3, 1, 1), (128, 32, 1), True, False),
    # ROW3, tiles across image borders
    "r3_48_n64": ((3, 48, 9, 7, 64, 3, 1, 1), (128, 32, 1), False, False),
    # ROW3, ragged channel tile
    "r3_80_n160": ((1, 80, 7, 9, 160, 3, 1, 1), (128, 64, 1), False, False),
    # ROW3, longest reduction
    "r3_512_n64": ((1, 512, 5, 7, 64, 3, 1, 1), (128, 32, 1), False, False),
    # stride 2
    "s2_32_n32": ((2, 32, 10, 6, 32, 3, 2, 1), (128, 32, 0), True, False),
    # stride 2, wider layer
    "s2_96_n128": ((1, 96, 10, 10, 128, 3, 2, 1), (128, 64, 0), False, False),
    # 256 x 64 tiles, last tile half full
    "t256_pw_n64": ((1, 512, 129, 128, 64, 1, 1, 0), (256, 64, 0), False, False),
    # 256 x 128 tiles
    "t256_pw_n128": ((1, 512, 129, 128, 128, 1, 1, 0), (256, 128, 0), False, False),
    # persistent blocks over several pixel tiles: the per-channel constants must survive the tile loop
    "multi_pw": ((1, 32, 258, 128, 512, 1, 1, 0), (128, 128, 0), False, True),
}
# the stem, driven through the pixel-pair layout: (N, B, H, W, bn): the dedicated kernel, conv_igemm_stem_kernel<32>, <64>
STEM_CASES = [(32, 2, 20, 72, 32), (48, 2, 20, 72, 32), (64, 1, 520, 520, 64)]
# SiLU / Hardswish: the 1x1 Cin 16 case, ROW3 32 -> 32, ROW3 512 -> 64, ROW3 80 -> 160
SMOOTH_CASES = ("pw16_n32", "r3_32_n32", "r3_512_n64", "r3_80_n160")


def is_fp32(t: torch.Tensor) -> torch.Tensor:
    t = t.double()
    return t.float().double() == t


def act64(z: torch.Tensor, act: int) -> torch.Tensor:
    """The activation in float64."""
    if act == ACT_IDENTITY:
        return z
    if act == ACT_RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == ACT_LEAKY:
        return torch.where(z > 0, z, z * SLOPE)
    if act == ACT_SILU:
        return z * torch.sigmoid(z)
    if act == ACT_HARDSWISH:
        return z * torch.clamp(z + 3.0, 0.0, 6.0) / 6.0
    raise ValueError(act)


def constants(N, exps, gen):
    """scale[n] = +-2^-e with e drawn from `exps`, shift[n] a multiple of 0.25 in [-8, 8]"""
    e = torch.tensor(exps)[torch.randint(0, len(exps), (N,), generator=gen)]
    sign = torch.randint(0, 2, (N,), generator=gen) * 2 - 1
    scale = sign.double() * torch.ldexp(torch.ones(N, dtype=torch.float64), -e)
    shift = torch.randint(-32, 33, (N,), generator=gen).double() * 0.25
    return scale, shift


def _problem(seed, xshape, wshape, s, p, exps, smooth):
    g = torch.Generator().manual_seed(seed)
    x, w = int_tensor(xshape, 16, g), int_tensor(wshape, 8, g)
    S = conv_ref(x, w, s, p)[0]
    S_abs = conv_abs(x, w, s, p)[0]
    N = wshape[0]
    if smooth:
        # one exponent per case (and the next one), the smallest that keeps |z| <= 128
        e0 = 0
        while float(S_abs.max()) * 2.0 ** -e0 + 8.0 > 128.0:
            e0 += 1
        exps = (e0, e0 + 1)
    scale, shift = constants(N, exps, g)
    res = int_tensor(S.shape, 16, g)
    z = S * scale.view(1, N, 1, 1) + shift.view(1, N, 1, 1)
    bound = S_abs * scale.abs().view(1, N, 1, 1) + shift.abs().view(1, N, 1, 1)
    return dict(x=x, w=w, scale=scale, shift=shift, res=res, z=z, bound=float(bound.max()))


@functools.lru_cache(maxsize=4)
def problem(cid, smooth=False):
    (B, Cin, H, W, N, k, s, p), _, _, _ = CASES[cid]
    exps = (1, 2, 3) if Cin == 512 else (0, 1, 2, 3)
    return _problem(sum(map(ord, cid)) + (977 if smooth else 0), (B, Cin, H, W), (N, Cin, k, k), s, p, exps, smooth)


@functools.lru_cache(maxsize=2)
def stem_problem(N, B, H, W):
    return _problem(4000 + N + H, (B, 3, H, W), (N, 3, 6, 6), 2, 2, (0, 1, 2, 3), False)


def _exact(pr, act):
    """per problem and activation, computed once: bf16_rne(act(z)), the two-rounding residual result (float64), and the
    conditions and shares check_exact_conditions reports (the one-rounding alternative is only counted against)"""
    memo = pr.setdefault("_exact", {})
    if act not in memo:
        a = act64(pr["z"], act)
        o = bf16_rne(a)
        r = pr["res"].double()
        two, one = bf16_rne(o + r), bf16_rne(a + r)
        memo[act] = dict(o=o, two=two, fp32=bool(is_fp32(pr["z"]).all()) and bool(is_fp32(a).all()),
                         sum_fp32=bool(is_fp32(o + r).all()), share=(~is_bf16(a)).double().mean().item(),
                         differ=(two != one).double().mean().item())
    return memo[act]


def expected_exact(pr, act, residual):
    """(stored value,) in float64"""
    e = _exact(pr, act)
    return (e["two"] if residual else e["o"],)


def check_exact_conditions(what, pr, act, residual):
    """The conditions under which the exact comparison is determined, and that it is not vacuous; on inputs and reference alone.
    Returns (share of act(z) that is no bf16 number, share of elements where two roundings and one differ)."""
    assert pr["bound"] * 32.0 < LIMIT, f"{what}: (sum |x w| |scale| + |shift|) / 2^-5 reaches {pr['bound'] * 32.0:.0f} >= 2^24"
    e = _exact(pr, act)
    assert e["fp32"], f"{what}: z and act(z) must be fp32 numbers"
    assert e["sum_fp32"], f"{what}: bf16(act(z)) + r must be an fp32 number"
    share, differ = e["share"], e["differ"]
    assert share >= 0.10, f"{what}: only {share:.4f} of act(z) needs rounding"
    if residual:
        assert differ >= 0.01, f"{what}: two roundings and one differ on only {differ:.4f} of the elements"
    return share, differ


def near_boundary(a: torch.Tensor) -> torch.Tensor:
    """True where the float64 value lies within DELTA |a| of a bf16 rounding boundary (the midpoint of two neighbours)."""
    q = _quantum(a)
    frac = a / q - torch.floor(a / q)
    return (frac - 0.5).abs() * q <= DELTA * a.abs()


def bf16_neighbours(a: torch.Tensor):
    """the bf16 numbers below and above a float64 value (equal where it is one itself)"""
    q = _quantum(a)
    return torch.floor(a / q) * q, torch.ceil(a / q) * q


def allowance(pr, act) -> torch.Tensor:
    """Where the stored value may be the other bf16 neighbour: near a rounding boundary - and, for Hardswish, only inside
    |z| < 3.  Outside, the kernel's own arithmetic is exact: z + 3 is an fp32 number, the clamp gives 6 or 0, z * 6 is an
    fp32 number (asserted in check_smooth_conditions) and the correctly rounded division by 6 returns z (or 0) itself, so
    the exact ties that large z produce are rounded to even like the reference's."""
    near = near_boundary(act64(pr["z"], act))
    return near & (pr["z"].abs() < 3.0) if act == ACT_HARDSWISH else near


def check_smooth_conditions(what, pr, act):
    z = pr["z"]
    assert float(z.abs().max()) <= 128.0 and bool(is_fp32(z).all()), f"{what}: |z| <= 128 and exact in fp32"
    if act == ACT_HARDSWISH:
        assert bool(is_fp32(z + 3.0).all()) and bool(is_fp32(z * 6.0).all()), f"{what}: z + 3 and 6 z must be fp32 numbers"
    near = allowance(pr, act).double().mean().item()
    assert near <= 0.05, f"{what}: {near:.4f} of the elements lie near a rounding boundary"
    return near


def check_smooth(what, got64, pr, act):
    """got == bf16_rne(reference) except, by one bf16 step, where the reference is near a rounding boundary."""
    a = act64(pr["z"], act)
    want = bf16_rne(a)
    ne = got64 != want
    lo, hi = bf16_neighbours(a)
    one_step = (got64 == lo) | (got64 == hi)
    near = allowance(pr, act)
    rel = ((got64 - a).abs() / a.abs().clamp_min(1e-300))[ne]
    print(f"SMOOTH {what}: {int(ne.sum())}/{ne.numel()} one step off ({ne.double().mean().item():.5f}); allowed on "
          f"{near.double().mean().item():.5f}")
    assert bool(one_step[ne].all()), f"{what}: {int((ne & ~one_step).sum())} elements are more than one bf16 step off (worst relative {float(rel.max()):.3e})"
    assert bool(near[ne].all()), f"{what}: {int((ne & ~near).sum())} mismatches away from every rounding boundary"
