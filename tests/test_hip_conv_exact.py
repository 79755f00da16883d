"""The convolution kernels (csrc/conv_igemm.hip, csrc/conv_wgrad.hip) bit for bit against float64.

Exact regime (tests/conv_reference.py): activations are integers in [-16, 16], weights and output gradients integers in
[-8, 8] - all bf16 numbers - and every case asserts that conv(|x|, |w|) stays below 2^24.  Then every product and every
fp32 partial sum is an exact integer in any summation order, the result is determined (y, dX = bf16_rne(S), dW = S * scale)
and the comparison is torch.equal.  One dropped, duplicated or misplaced reduction term changes S by an integer, so it
shows unless it hides behind the final bf16 rounding of one element; a case has hundreds to millions of elements.

The inputs must make that rounding matter: every compared bf16 tensor differs from its float64 value on at least 1 % of
its elements, and over the forward cases together at least 5 % of the sums are exact round-to-even ties.  These are
conditions on inputs and reference alone; test_inputs_are_exact_and_not_vacuous checks them without a GPU.

Every case names the launch plan it was written for (kodhip_conv_plan_query / kodhip_conv_wgrad_plan_query) and asserts it
- on the CPU too (test_plans_reached) - so a change of the dispatch that leaves a kernel form unreached fails here.

The kernel bodies behind KODHIP_ROW3=0, KODHIP_NO_FAST=1, KODHIP_WGRAD_ROW3=2, KODHIP_WGRAD_DMA=none,
KODHIP_S2_SEPARATE=1 and KODHIP_FORCE_BN=128 run this file again in a child process each (test_bodies_behind_the_knobs); plan expectations that
depend on a knob are read under the same environment (KNOB below).
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch

from object_detection_cib_amd import _lib  # noqa: E402
from conv_reference import (accumulate_bf16, bf16_rne, conv_abs, conv_ref, double_rounding, first_mismatch, int_tensor,  # noqa: E402
                            is_bf16, is_rne_tie, single_rounding)
from hip_helpers import nhwc, pack, pad, stream  # noqa: E402

gpu = pytest.mark.gpu
LIMIT = float(2 ** 24)
XS, YS, FS = 2.0 ** 100, 776.0, -12345.0       # sentinels: input buffers (finite: a padded K column multiplies it by 0), bf16 outputs, fp32 buffers

KNOB = {k: os.environ.get(k) for k in ("KODHIP_ROW3", "KODHIP_NO_FAST", "KODHIP_WGRAD_ROW3", "KODHIP_WGRAD_DMA", "KODHIP_S2_SEPARATE",
                                             "KODHIP_FORCE_BN")}
NO_FAST = bool(KNOB["KODHIP_NO_FAST"])
ROW3_OFF = KNOB["KODHIP_ROW3"] == "0"
S2_SEP = bool(KNOB["KODHIP_S2_SEPARATE"])
WG_ROW3_ALL = KNOB["KODHIP_WGRAD_ROW3"] == "2"
WG_NO_DMA = (KNOB["KODHIP_WGRAD_DMA"] or "")[:1] == "n"
FORCE_BN = int(KNOB["KODHIP_FORCE_BN"] or 0)


# ---- plans -------------------------------------------------------------------------------------------------------------
def conv_plan(op, B, Cin, H, W, N, k, s, p):
    """{bm, bn, row3, fast, tiles_m, tiles_n, groups_m, merged} of op 0 forward / 1 dgrad / 2 parity classes / 3 folded /
    4 dual for a layer Cin -> N on B x H x W inputs, contiguous tensors."""
    out = (C.c_int * 8)()
    Kp = {0: k * k * pad(Cin, 32), 1: k * k * pad(N, 32), 2: 0, 3: 0, 4: pad(N, 32)}[op]
    _lib.check(_lib.lib().kodhip_conv_plan_query(op, B, H, W, Cin, 0, Cin, N, k, k, s, s, p, p, Kp, N, 0, out), "plan")
    return dict(zip(("bm", "bn", "row3", "fast", "tiles_m", "tiles_n", "groups_m", "merged"), out))


def wgrad_plan(B, Cin, H, W, N, k, s, p, dual=0, Kp=None, kw=None, sw=None, pw=None, ldx=None):
    out = (C.c_int * 8)()
    kw, sw, pw = kw or k, sw or s, p if pw is None else pw
    Kp = Kp or pad(k * kw * Cin, 32)
    _lib.check(_lib.lib().kodhip_conv_wgrad_plan_query(B, H, W, ldx or Cin, Cin, N, k, kw, s, sw, p, pw, Kp, N, dual, out), "wplan")
    return dict(zip(("tn", "tk", "row3", "wn", "rn", "wc", "splits", "dma"), out))


def expect_conv_plan(got, want, what, n_out=0):
    """want: (bm, bn, row3) written for the default environment; under a knob the knob's own property is asserted and the
    tile shape only where the knob leaves it alone.  n_out: GEMM columns (for KODHIP_FORCE_BN)."""
    bm, bn, row3 = want
    if FORCE_BN and n_out > FORCE_BN // 2:
        bn = FORCE_BN                                           # the widest tile is taken wherever N admits it
    if NO_FAST:
        assert got["fast"] == 0 and got["row3"] == 0 and got["bm"] == 128, (what, got)
        return
    if ROW3_OFF and row3:
        assert got["row3"] == 0, (what, got)
        return
    assert (got["bm"], got["bn"], got["row3"]) == (bm, bn, row3), (what, got, want)


# ---- cases -------------------------------------------------------------------------------------------------------------
# id: (B, Cin, H, W, N, k, s, p, ops, plans): ops f forward, d kodhip_conv_dgrad, c parity classes, o folded, w weight gradient.
# plans: per op the (bm, bn, row3) the case was written for; "w": (tn, tk, row3) of the weight gradient; "fast_d": 0 where the
# plain data gradient is meant to leave the FAST path.  One line per case: the form it reaches and why it is the smallest.
CASES = {
    # 1x1.  Cin 16: every half step a K tail (16 -> 32); 126 pixels: one ragged 128-pixel tile; narrowest channel tile.
    "pw16_n32": (2, 16, 9, 7, 32, 1, 1, 0, "fdw", {"f": (128, 32, 0), "d": (128, 32, 0), "w": (32, 32, 0)}),
    # Cin 48: half-step FAST form with a K tail (48 -> 64) in both directions; N 33..64; 120 pixels of 6-pixel rows.
    "pw48_n64": (2, 48, 10, 6, 64, 1, 1, 0, "fdw", {"f": (128, 32, 0), "d": (128, 32, 0), "w": (64, 64, 0)}),
    # Cin 80 (yv5x width): 2.5 K steps; N = 96 is 64 < N <= 128 (forward: two 64-column tiles win at one round); 189 pixels: a full
    # and a ragged tile.
    "pw80_n96": (3, 80, 9, 7, 96, 1, 1, 0, "fdw", {"f": (128, 64, 0), "d": (128, 64, 0), "w": (128, 128, 0)}),
    # Cin 512, N = 160 > 128: two channel tiles, the second ragged (32 of its columns); 63 pixels.
    "pw512_n160": (1, 512, 9, 7, 160, 1, 1, 0, "fdw", {"f": (128, 64, 0), "d": (128, 64, 0), "w": (64, 128, 0)}),
    # the 32 -> 32 pointwise layer: the weakest rounding share of the set (dX: 2-3 % of the sums are no bf16 numbers).
    "pw32_n32": (2, 32, 16, 16, 32, 1, 1, 0, "fdw", {"f": (128, 32, 0), "d": (128, 32, 0), "w": (32, 32, 0)}),
    # Cin 96 -> 128 (yv5m widths), 128 -> 96: whole K steps, 128-column tile exactly full / three quarters used.
    "pw96_n128": (2, 96, 9, 7, 128, 1, 1, 0, "fdw", {"f": (128, 64, 0), "d": (128, 64, 0), "w": (128, 128, 0)}),
    "pw128_n96": (1, 128, 10, 6, 96, 1, 1, 0, "fdw", {"f": (128, 64, 0), "d": (128, 64, 0), "w": (128, 128, 0)}),
    # 3x3 / stride 1 / pad 1: the ROW3 form (row segments shared by three taps, border taps masked per lane).
    # rows of 6 pixels: shorter than a DMA piece, every lane group meets both borders; N <= 32; dW: ROW3 <1, 1, 1>.
    "r3_32_n32": (2, 32, 10, 6, 32, 3, 1, 1, "fdw", {"f": (128, 32, 1), "d": (128, 32, 1), "w": (32, 32, 1)}),
    # Cin 48: K tail inside every tap (48 -> 64); odd 9 x 7 images, a tile spans image boundaries; N = 64.
    "r3_48_n64": (3, 48, 9, 7, 64, 3, 1, 1, "fdw", {"f": (128, 32, 1), "d": (128, 32, 1), "w": (64, 128, 0)}),
    # Cin 16: every half step is a new tap; N = 128.
    "r3_16_n128": (2, 16, 9, 7, 128, 3, 1, 1, "fdw", {"f": (128, 64, 1), "d": (128, 32, 1), "w": (128, 128, 0)}),
    # Cin 80, N = 160 > 128 (ragged second channel tile), 7 x 9.
    "r3_80_n160": (1, 80, 7, 9, 160, 3, 1, 1, "fdw", {"f": (128, 64, 1), "d": (128, 64, 1), "w": (64, 128, 0)}),
    # Cin 96 -> 48 and 128 -> 96: three / four whole chunks per tap.
    "r3_96_n48": (2, 96, 10, 6, 48, 3, 1, 1, "fdw", {"f": (128, 32, 1), "d": (128, 64, 1), "w": (64, 128, 0)}),
    "r3_128_n96": (1, 128, 9, 7, 96, 3, 1, 1, "fdw", {"f": (128, 64, 1), "d": (128, 64, 1), "w": (128, 128, 0)}),
    # Cin 512 (K = 4608, the longest reduction of the set: sum |x w| <= 589 824), 5 x 7; dW: ROW3 <1, 2, 2> by default (Cin >= 256).
    "r3_512_n64": (1, 512, 5, 7, 64, 3, 1, 1, "fdw", {"f": (128, 32, 1), "d": (128, 64, 1), "w": (64, 64, 1)}),
    # 3x3 / stride 2 / pad 1: forward on the FAST path, plain data gradient on the register-staged path (strided gather), the
    # parity classes in one merged launch, the folded form.  10 x 6 -> 5 x 3 outputs.
    "s2_32_n32": (2, 32, 10, 6, 32, 3, 2, 1, "fdcow", {"f": (128, 32, 0), "d": (128, 32, 0), "c": (128, 32, 0), "o": (128, 64, 0), "w": (32, 288, 0), "fast_d": 0}),
    "s2_48_n64": (2, 48, 10, 6, 64, 3, 2, 1, "fdcow", {"f": (128, 32, 0), "d": (128, 32, 0), "c": (128, 32, 0), "o": (128, 64, 0), "w": (64, 128, 0), "fast_d": 0}),
    "s2_16_n48": (2, 16, 8, 8, 48, 3, 2, 1, "fdcow", {"f": (128, 32, 0), "d": (128, 32, 0), "c": (128, 32, 0), "o": (128, 32, 0), "w": (64, 128, 0), "fast_d": 0}),
    # dY with 48 channels gathered by the merged launch in half steps; Cin 96: the class launch's 128-column tile three quarters used.
    "s2_96_n128": (1, 96, 10, 10, 128, 3, 2, 1, "fdcow", {"f": (128, 64, 0), "d": (128, 64, 0), "c": (128, 64, 0), "o": (128, 64, 0), "w": (128, 128, 0), "fast_d": 0}),
    "s2_128_n160": (1, 128, 12, 10, 160, 3, 2, 1, "fdcow", {"f": (128, 64, 0), "d": (128, 64, 0), "c": (128, 64, 0), "o": (128, 64, 0), "w": (64, 128, 0), "fast_d": 0}),
    # Cin = 512 at stride 2 (16 chunks per tap; dX tiles of 512 / 2048 columns), 6 x 6 -> 3 x 3.
    "s2_512_n32": (1, 512, 6, 6, 32, 3, 2, 1, "fdcow", {"f": (128, 32, 0), "d": (128, 64, 0), "c": (128, 64, 0), "o": (128, 64, 0), "w": (32, 128, 0), "fast_d": 0}),
    # odd 9 x 7 input (5 x 4 outputs): the forms that need even dims do not apply.
    "s2_80_odd": (2, 80, 9, 7, 64, 3, 2, 1, "fdw", {"f": (128, 32, 0), "d": (128, 64, 0), "w": (64, 128, 0), "fast_d": 0}),
    # ---- 256-pixel tiles (8 waves, 3-stage ring): bm = 256 needs M >= 16384, K >= 512, N > 32 and no ROW3.
    # 1x1, Cin = 512 (K / 32 = 16, not a multiple of the ring depth), M = 16384 + 128 (65 tiles, the last half full): 256 x 64, 256 x 128.
    "t256_pw_n64": (1, 512, 129, 128, 64, 1, 1, 0, "f", {"f": (256, 64, 0)}),
    "t256_pw_n128": (1, 512, 129, 128, 128, 1, 1, 0, "f", {"f": (256, 128, 0)}),
    # 3x3 / stride 2 forward, K = 576 (18 steps), output 4 x 64 x 64 = 16384 pixels; its parity-class data gradient: dY 128 channels, the
    # four-tap class K = 512, 16384 pixels per class: conv_igemm_x4_kernel<256, 64>; the folded form of the same layer: 256 x 128.
    "t256_s2": (4, 64, 128, 128, 128, 3, 2, 1, "fco", {"f": (256, 128, 0), "c": (256, 64, 0), "o": (256, 128, 0)}),
    # the plain data gradient on 256-pixel tiles (conv_igemm_kernel<256, 64, MODE_PLAIN>): 1x1, dY 512 channels (K = 512), 16384 pixels.
    "t256_dgrad": (1, 64, 128, 128, 512, 1, 1, 0, "d", {"d": (256, 64, 0)}),
    # ---- persistent blocks that loop over several pixel tiles (tiles_m > groups_m): N = 512 makes the per-tile block target small.
    # ROW3: 8 channel tiles of 64 -> 96 blocks per tile for 130 pixel tiles.
    "multi_r3": (1, 32, 130, 128, 512, 3, 1, 1, "f", {"f": (128, 64, 1), "multi": 1}),
    # plain FAST form: 4 channel tiles of 128 -> 256 blocks per tile for 258 pixel tiles.
    "multi_pw": (1, 32, 258, 128, 512, 1, 1, 0, "f", {"f": (128, 128, 0), "multi": 1}),
}
CASE_IDS = list(CASES)
# under KODHIP_ROW3=0 the 3x3 / stride 1 layers take the generic FAST kernel: its 256-pixel tiles need their own case
CASES_ROW3_OFF = {"t256_3x3": (4, 64, 64, 64, 128, 3, 1, 1, "fd", {"f": (256, 128, 0), "d": (256, 64, 0)})}


@functools.lru_cache(maxsize=3)
def reference(cid, bx=16, bw=8):
    B, Cin, H, W, N, k, s, p, ops, _ = {**CASES, **CASES_ROW3_OFF}[cid]
    g = torch.Generator().manual_seed(sum(map(ord, cid)))
    x = int_tensor((B, Cin, H, W), bx, g)
    w = int_tensor((N, Cin, k, k), bw, g)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = int_tensor((B, N, Ho, Wo), 8, g)
    r = dict(x=x, w=w, dy=dy)
    # sum |a b| per output element: conv(|x|, |w|); the large cases take its upper bound (operand bounds x reduction length)
    big = B * H * W > 4096
    if "f" in ops:
        r["y"] = conv_ref(x, w, s, p)[0]
        r["y_abs"] = float(bx * bw * k * k * Cin) if big else conv_abs(x, w, s, p)[0].max().item()
    if set(ops) & set("dco"):
        r["dx"] = torch.nn.grad.conv2d_input(x.shape, w.double(), dy.double(), s, p)
        r["dx_abs"] = (float(8 * bw * k * k * N) if big else
                       torch.nn.grad.conv2d_input(x.shape, w.double().abs(), dy.double().abs(), s, p).max().item())
    if "w" in ops:
        r["dw"] = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), s, p)
        r["dw_abs"] = torch.nn.grad.conv2d_weight(x.double().abs(), w.shape, dy.double().abs(), s, p).max().item()
    return r


def rounding_share(S):
    return (~is_bf16(S)).double().mean().item()


def check_inputs(cid, r):
    """< 2^24 precondition and the non-vacuity share of every compared bf16 tensor; returns the forward tie share."""
    for key in ("y", "dx", "dw"):
        if key in r:
            assert r[key + "_abs"] < LIMIT, f"{cid}: sum |a b| of {key} reaches {r[key + '_abs']:.0f} >= 2^24"
    for key in ("y", "dx"):
        if key in r:
            share = rounding_share(r[key])
            assert share >= 0.01, f"{cid}: only {share:.4f} of {key} needs rounding"
    return is_rne_tie(r["y"]).double().mean().item() if "y" in r else None


def test_inputs_are_exact_and_not_vacuous():
    """Conditions on inputs and reference alone (no GPU): every case below 2^24, >= 1 % of each bf16 tensor rounds, and >= 5 % of
    all forward sums are exact round-to-even ties."""
    ties, count = 0.0, 0
    for cid in CASE_IDS:
        if CASES[cid][0] * CASES[cid][2] * CASES[cid][3] > 4096:
            continue                                   # the large cases check themselves on the GPU (same function)
        r = reference(cid)
        t = check_inputs(cid, r)
        if t is not None:
            ties += t * r["y"].numel(); count += r["y"].numel()
        print(f"INPUTS {cid}: y rounds {rounding_share(r['y']) if 'y' in r else -1:.3f} ties {t if t is not None else -1:.3f} "
              f"dx rounds {rounding_share(r['dx']) if 'dx' in r else -1:.3f}")
    assert ties / count >= 0.05, f"only {ties / count:.4f} of the forward sums are ties"


@pytest.fixture(scope="module")
def built():
    """The library, built if it is not there yet (the CPU tests of this file must run on their own in a clean checkout)."""
    from object_detection_cib_amd import build
    return build.build(verbose=False)


@pytest.mark.parametrize("cid", CASE_IDS + list(CASES_ROW3_OFF))
def test_plans_reached(built, cid):
    """Every case reaches the kernel form it was written for (no GPU needed: the query launches nothing)."""
    check_plans(cid)


def check_plans(cid):
    off = cid in CASES_ROW3_OFF
    B, Cin, H, W, N, k, s, p, ops, plans = (CASES_ROW3_OFF if off else CASES)[cid]
    if off and not ROW3_OFF:
        got = conv_plan(0, B, Cin, H, W, N, k, s, p)
        assert NO_FAST or got["row3"] == 1 and got["bm"] == 128, got      # by default ROW3 keeps 3x3 / stride 1 on 128-pixel tiles
        return
    for op, code in (("f", 0), ("d", 1), ("c", 2), ("o", 3)):
        if op not in ops or (NO_FAST and op == "o"):            # the folded form exists on the FAST path only
            continue
        got = conv_plan(code, B, Cin, H, W, N, k, s, p)
        if op == "d" and plans.get("fast_d") == 0:
            assert got["fast"] == 0 and got["bm"] == 128, (cid, got)
            continue
        if off:
            assert (got["bm"], got["bn"], got["row3"]) == plans[op], (cid, op, got)
            continue
        expect_conv_plan(got, plans[op], (cid, op), {"f": N, "o": 4 * Cin}.get(op, Cin))
        if op == "c" and not NO_FAST:
            assert (got["merged"] == 0) if S2_SEP else (got["merged"] == plans[op][0]), (cid, got)
        if plans.get("multi") and not NO_FAST and not ROW3_OFF:
            assert got["tiles_m"] > got["groups_m"], (cid, got)
    if "w" in ops:
        got = wgrad_plan(B, Cin, H, W, N, k, s, p)
        tn, tk, row3 = plans["w"]
        eligible = (k, s, p) == (3, 1, 1) and Cin % 32 == 0
        if WG_ROW3_ALL and eligible:
            assert got["row3"] == 1, (cid, got)
        elif KNOB["KODHIP_WGRAD_ROW3"] == "0":
            assert got["row3"] == 0, (cid, got)
        else:
            assert (got["tn"], got["tk"], got["row3"]) == (tn, tk, row3), (cid, got)
        assert got["dma"] == (0 if WG_NO_DMA and not got["row3"] else 1), (cid, got)


# ---- GPU plumbing --------------------------------------------------------------------------------------------------------
def sliced(t_nchw, ld, coff, fill, dtype=torch.bfloat16):
    """NCHW values as channels [coff, coff + C) of a sentinel-filled [B, H, W, ld] device buffer."""
    B, Cc, H, W = t_nchw.shape
    buf = torch.full((B, H, W, ld), fill, dtype=dtype)
    buf[..., coff:coff + Cc] = t_nchw.permute(0, 2, 3, 1).to(dtype)
    return buf.cuda()


def expect_buf(t_nchw64, ld, coff, fill, dtype=torch.bfloat16):
    B, Cc, H, W = t_nchw64.shape
    buf = torch.full((B, H, W, ld), fill, dtype=torch.float64)
    buf[..., coff:coff + Cc] = t_nchw64.permute(0, 2, 3, 1)
    return buf


def same(got_dev, want64, what, bm=128, bn=128):
    got = got_dev.cpu().double()
    assert torch.equal(got, want64), f"{what}: {first_mismatch(got, want64, bm, bn)}"


def stats_exact(stats, y_stored64, N, what):
    """Slot sums of the stored outputs and of their squares, exact where they stay below 2^24."""
    assert bool((y_stored64 == y_stored64.round()).all()), f"{what}: the stored outputs must be integers"
    v = y_stored64.reshape(-1, N).to(torch.int64)
    s1, s2 = v.sum(0), (v * v).sum(0)
    assert int(s2.max()) < 2 ** 24, f"{what}: sum y^2 reaches {int(s2.max())}"
    st = stats.cpu().double()
    assert bool(torch.isfinite(st).all()), f"{what}: a statistics slot was left unwritten"
    assert torch.equal(st[0].sum(-1), s1.double()), f"{what}: slot sums of y"
    assert torch.equal(st[1].sum(-1), s2.double()), f"{what}: slot sums of y^2"


def fwd_launch(x, w, s, p, ld_in=None, ci=0, ld_out=None, co=0):
    lib = _lib.lib()
    B, Cin, H, W = x.shape
    N, _, k, _ = w.shape
    ld_in, ld_out = ld_in or Cin, ld_out or N
    pk = pack([w])
    xb = sliced(x, ld_in, ci, XS)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    out = torch.full((B, Ho, Wo, ld_out), YS, dtype=torch.bfloat16, device="cuda")
    T = lib.kodhip_conv_stats_slots(B * Ho * Wo, N)
    stats = torch.full((2 * N * T,), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.kodhip_conv_fwd_raw(xb.data_ptr(), pk["f"].data_ptr(), out.data_ptr(), stats.data_ptr(), B, H, W, ld_in, ci, Cin,
                                       N, k, k, s, s, p, p, pk["Kp"], ld_out, co, stream()), "conv_fwd_raw")
    torch.cuda.synchronize()
    return out, stats.view(2, N, T)


def dgrad_launch(form, dy, w, xshape, s, p, dx, ld, coff, acc, shadow=None, ld_dy=None, cdy=0, dy2=None, w2=None, bnred=False):
    """form: plain | classes | folded | dual.  dx: device buffer [B, H, W, ld]; returns the return code."""
    lib = _lib.lib()
    B, Cin, H, W = xshape
    N, k = w.shape[0], w.shape[2]
    ld_dy = ld_dy or N
    dyb = sliced(dy, ld_dy, cdy, XS)
    sh = shadow.data_ptr() if shadow is not None else None
    pk = pack([w], s2={"classes": True, "folded": "fold"}.get(form, False))
    tail = ()
    if bnred:
        slots = {"plain": lambda: lib.kodhip_conv_dgrad_bnred_slots(B, H, W, Cin, N, k, k, s, s, p, p, ld_dy, 0),
                 "classes": lambda: lib.kodhip_conv_dgrad_bnred_slots(B, H, W, Cin, N, 3, 3, 2, 2, 1, 1, ld_dy, 1),
                 "folded": lambda: lib.kodhip_conv_dgrad_s2f_bnred_slots(B, H, W, Cin, N, ld_dy),
                 "dual": lambda: lib.kodhip_conv_dgrad_dual_bnred_slots(B, H, W, Cin, N, ld_dy)}[form]()
        assert slots > 0, "this geometry must carry the fused reduction"
        seg = (_lib.KodBnRedSeg * 1)()
        raw = torch.zeros((B * H * W, Cin), dtype=torch.bfloat16, device="cuda")
        aff = torch.cat([torch.ones(Cin), torch.zeros(Cin)]).cuda()
        part = torch.full((2 * Cin * slots,), float("nan"), device="cuda")
        seg[0].ch_begin, seg[0].ch_count, seg[0].raw, seg[0].ldr = 0, Cin, raw.data_ptr(), Cin
        seg[0].aff, seg[0].partials = aff.data_ptr(), part.data_ptr()
        tail = (C.cast(seg, C.c_void_p), 1, slots)
    if form == "plain":
        fn = lib.kodhip_conv_dgrad_bnred if bnred else lib.kodhip_conv_dgrad
        rc = fn(dyb.data_ptr(), pk["d"].data_ptr(), dx.data_ptr(), B, H, W, ld, coff, Cin, N, k, k, s, s, p, p, pk["Kdp"], ld_dy, cdy,
                acc, sh, *tail, stream())
    elif form in ("classes", "folded"):
        fn = {("classes", False): lib.kodhip_conv_dgrad_s2, ("classes", True): lib.kodhip_conv_dgrad_s2_bnred,
              ("folded", False): lib.kodhip_conv_dgrad_s2f, ("folded", True): lib.kodhip_conv_dgrad_s2f_bnred}[(form, bnred)]
        rc = fn(dyb.data_ptr(), pk["d"].data_ptr(), dx.data_ptr(), B, H, W, ld, coff, Cin, N, ld_dy, cdy, acc, sh, *tail, stream())
    else:
        fn = lib.kodhip_conv_dgrad_dual_bnred if bnred else lib.kodhip_conv_dgrad_dual
        pk2 = pack([w2])
        dyb2 = sliced(dy2, ld_dy, cdy, XS)
        rc = fn(dyb.data_ptr(), pk["d"].data_ptr(), dyb2.data_ptr(), pk2["d"].data_ptr(), dx.data_ptr(), B, H, W, ld, coff, Cin, N,
                pk["Kdp"], ld_dy, cdy, acc, sh, *tail, stream())
    torch.cuda.synchronize()
    if bnred and rc == 0:
        assert bool(torch.isfinite(part).all()), "a partial slot of the fused reduction was left unwritten"
    return rc


def wgrad_launch(x, dy, wshape, s, p, scale=1.0, n_valid=None, ld_in=None, ci=0, ld_dy=None, cdy=0, part_offset=0):
    """-> (grad buffer [N * Cin * k * k + 64] sentinel-filled, splits)"""
    lib = _lib.lib()
    B, Cin, H, W = x.shape
    N, _, k, _ = wshape
    ld_in, ld_dy = ld_in or Cin, ld_dy or N
    Kp = pad(k * k * Cin, 32)
    xb, dyb = sliced(x, ld_in, ci, XS), sliced(dy, ld_dy, cdy, XS)
    splits = lib.kodhip_conv_wgrad_splits_geo(B, H, W, ld_in, Cin, N, k, k, s, s, p, p, Kp, ld_dy)
    part = torch.full((splits * N * Kp + 4,), float("nan"), dtype=torch.float32, device="cuda")
    grad = torch.full((N * Cin * k * k + 64,), FS, dtype=torch.float32, device="cuda")
    _lib.check(lib.kodhip_conv_wgrad(xb.data_ptr(), dyb.data_ptr(), part.data_ptr() + 4 * part_offset, grad.data_ptr(), B, H, W, ld_in, ci,
                                     Cin, N, k, k, s, s, p, p, Kp, ld_dy, cdy, n_valid or N, 0, scale, stream()), "wgrad")
    torch.cuda.synchronize()
    return grad.cpu(), splits


STAT_RANGES = ((16, 8), (8, 8), (8, 4), (4, 4), (4, 2), (2, 2), (2, 1), (1, 1))


def stats_ranges(M, n_terms):
    """Operand ranges [-bx, bx] x [-bw, bw], halving in turn from [-16, 16] x [-8, 8], worth trying for exact statistics:
    those whose EXPECTED sum y^2 per channel (M outputs of n_terms products of independent uniform integers, variance
    b (b + 1) / 3 each) leaves a factor 1.5 below 2^24.  The caller still verifies the true sums."""
    return [(bx, bw) for bx, bw in STAT_RANGES if 1.5 * M * n_terms * bx * (bx + 1) * bw * (bw + 1) / 9 < LIMIT]


def stats_operands(cid):
    """The largest operand ranges at which sum bf16(y)^2 per channel stays below 2^24 (stated by the caller's print)."""
    B, Cin, H, W, N, k, s, p = {**CASES, **CASES_ROW3_OFF}[cid][:8]
    M = B * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1)
    for bx, bw in stats_ranges(M, k * k * Cin):
        r = reference(cid, bx, bw)
        ys = bf16_rne(r["y"])
        if float((ys * ys).sum((0, 2, 3)).max()) < LIMIT:
            return bx, bw, r
    raise AssertionError(f"{cid}: no operand range keeps the statistics exact")


# ---- the operators, case by case ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cid", CASE_IDS + (list(CASES_ROW3_OFF) if ROW3_OFF else []))
def test_exact_fwd_dgrad_wgrad(cid):
    """Forward (+ statistics), every data-gradient form the geometry admits (+ accumulate on independent prior content) and
    the weight gradient, bit for bit; inputs and outputs are channel slices of sentinel-filled buffers."""
    B, Cin, H, W, N, k, s, p, ops, plans = {**CASES, **CASES_ROW3_OFF}[cid]
    check_plans(cid)
    r = reference(cid)
    check_inputs(cid, r)
    x, w, dy = r["x"], r["w"], r["dy"]
    big = B * H * W > 4096
    ld_in, ci = (Cin, 0) if big else (Cin + 24, 8)          # the large cases run contiguous (the slices are the small cases' job)
    ld_out, co = (N, 0) if big else (N + 24, 16)
    if "f" in ops:
        bm, bn = plans["f"][:2]
        out, stats = fwd_launch(x, w, s, p, ld_in, ci, ld_out, co)
        ys = bf16_rne(r["y"])
        same(out, expect_buf(ys, ld_out, co, YS), f"{cid} forward", bm, bn)
        assert bool(torch.isfinite(stats).all()), f"{cid}: a statistics slot was left unwritten"
        if k * k * pad(Cin, 32) <= 288:
            # exact statistics: the looping-block cases (several pixel tiles summed into one slot) included
            bx, bw, rs = stats_operands(cid)
            out, stats = fwd_launch(rs["x"], rs["w"], s, p, ld_in, ci, ld_out, co)
            ys = bf16_rne(rs["y"])
            print(f"STATS {cid}: operands in [-{bx}, {bx}] x [-{bw}, {bw}], {rounding_share(rs['y']):.3f} of y rounds")
            same(out, expect_buf(ys, ld_out, co, YS), f"{cid} forward (statistics operands)", bm, bn)
            stats_exact(stats, ys.permute(0, 2, 3, 1), N, cid)
    g = torch.Generator().manual_seed(len(cid))
    for op, form in (("d", "plain"), ("c", "classes"), ("o", "folded")):
        if op not in ops or (NO_FAST and form == "folded"):       # the folded form needs the FAST path by contract
            continue
        bm, bn = plans[op][:2]
        S = r["dx"]
        dx = torch.full((B, H, W, ld_in), YS, dtype=torch.bfloat16, device="cuda")
        rc = dgrad_launch(form, dy, w, x.shape, s, p, dx, ld_in, ci, 0, ld_dy=ld_out, cdy=co)
        _lib.check(rc, form)
        same(dx, expect_buf(bf16_rne(S), ld_in, ci, YS), f"{cid} dgrad {form}", bm, bn)
        # accumulate: the prior content is independent of the kernel's own output
        prior = int_tensor(S.shape, 256, g)
        dx = sliced(prior, ld_in, ci, YS)
        _lib.check(dgrad_launch(form, dy, w, x.shape, s, p, dx, ld_in, ci, 1, ld_dy=ld_out, cdy=co), form + " accumulate")
        want = accumulate_bf16(S, prior)
        assert (want != 2 * bf16_rne(S)).double().mean() > 0.9
        same(dx, expect_buf(want, ld_in, ci, YS), f"{cid} dgrad {form} accumulate", bm, bn)
    if "w" in ops:
        for scale in (1.0, 2.0 ** -7):
            grad, _ = wgrad_launch(x, dy, w.shape, s, p, scale, ld_in=ld_in, ci=ci, ld_dy=ld_out, cdy=co)
            want = torch.cat([(r["dw"] * scale).reshape(-1), torch.full((64,), FS, dtype=torch.float64)])
            assert torch.equal(grad.double(), want), f"{cid} wgrad scale {scale}: {first_mismatch(grad[:-64].view(N, Cin, k, k), (r['dw'] * scale))}"


# ---- weight gradient: every launch configuration, n_valid, the scalar reduction -----------------------------------------
# (B, Cin, H, W, N, k, s, p) -> (tn, tk) of wgrad_partial's generic table; 2 x 70 x 65 = 9100 rows give 36 slabs, so both loops of the
# slab reduction run (four chains over 8 split lanes, then the tail).  Kp = 160 / 288 with N <= 32 are the one-block-over-K forms.
WGRAD_CFG = [
    ((2, 128, 70, 65, 128, 1, 1, 0), (128, 128)), ((2, 96, 70, 65, 64, 1, 1, 0), (64, 128)), ((2, 160, 70, 65, 32, 1, 1, 0), (32, 160)),
    ((2, 32, 140, 130, 32, 3, 2, 1), (32, 288)), ((2, 128, 70, 65, 24, 1, 1, 0), (32, 128)), ((2, 64, 70, 65, 96, 1, 1, 0), (128, 64)),
    ((2, 48, 70, 65, 160, 1, 1, 0), (64, 64)), ((2, 64, 70, 65, 32, 1, 1, 0), (32, 64)), ((2, 32, 70, 65, 128, 1, 1, 0), (128, 32)),
    ((2, 16, 70, 65, 64, 1, 1, 0), (64, 32)), ((2, 24, 70, 65, 16, 1, 1, 0), (32, 32)),
]


@functools.lru_cache(maxsize=2)
def wref(geo):
    B, Cin, H, W, N, k, s, p = geo
    g = torch.Generator().manual_seed(sum(geo))
    x = int_tensor((B, Cin, H, W), 16, g)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = int_tensor((B, N, Ho, Wo), 8, g)
    dw = torch.nn.grad.conv2d_weight(x.double(), (N, Cin, k, k), dy.double(), s, p)
    top = torch.nn.grad.conv2d_weight(x.double().abs(), (N, Cin, k, k), dy.double().abs(), s, p).max().item()
    assert top < LIMIT, (geo, top)
    return x, dy, dw


@gpu
@pytest.mark.parametrize("geo,cfg", WGRAD_CFG, ids=lambda v: "x".join(map(str, v)))
def test_wgrad_every_launch_configuration(geo, cfg):
    """One case per (tn, tk) of wgrad_partial; scale 1 and 2^-7; n_valid < N into a sentinel-filled grad (exactly
    n_valid * Cin * KH * KW floats are written - include/kodhip.h); partials offset by one float: the scalar
    wgrad_reduce_kernel<1>, bit-identical to the 16-byte wgrad_reduce_kernel<4>."""
    B, Cin, H, W, N, k, s, p = geo
    got = wgrad_plan(*geo)
    assert (got["tn"], got["tk"], got["row3"]) == (*cfg, 0), got
    assert got["dma"] == (0 if WG_NO_DMA else 1)
    x, dy, dw = wref(geo)
    per = Cin * k * k
    tailv = torch.full((64,), FS, dtype=torch.float64)
    grad, splits = wgrad_launch(x, dy, dw.shape, s, p)
    assert splits == got["splits"] and splits >= 33, splits
    assert torch.equal(grad.double(), torch.cat([dw.reshape(-1), tailv])), f"{geo}: {first_mismatch(grad[:-64].view(dw.shape), dw)}"
    nv = N - 8
    g2, _ = wgrad_launch(x, dy, dw.shape, s, p, 2.0 ** -7, n_valid=nv, ld_in=Cin + 8, ci=8, ld_dy=N + 16, cdy=8)
    want = torch.cat([dw[:nv].reshape(-1) * 2.0 ** -7, torch.full((8 * per,), FS, dtype=torch.float64), tailv])
    assert torch.equal(g2.double(), want), f"{geo} n_valid: rows [0, {nv}) written, the rest untouched"
    g3, _ = wgrad_launch(x, dy, dw.shape, s, p, part_offset=1)
    assert torch.equal(g3, grad), "scalar slab reduction differs from the 16-byte route"


# 1x1 / stride 2: the smallest geometry that sends a narrow-K tile (Kp = 32) through the LDS-DMA kernel's two-division X gather
# (conv_wgrad_dma_kernel<1, 1, 1, 1, .., GM = 0>: launch_cfg takes GM = 1 for 1x1 / stride 1 / no padding only, and every other case
# with Kp <= 64 in this file is such a layer).  10 x 6 -> 5 x 3 outputs: 30 rows, one ragged 32-row stage whose gather skips every
# second pixel and every second image row.
WGRAD_S2PW = ((2, 16, 10, 6, 32, 1, 2, 0), (32, 32))


def check_s2pw_plan():
    got = wgrad_plan(*WGRAD_S2PW[0])
    assert (got["tn"], got["tk"], got["row3"]) == (*WGRAD_S2PW[1], 0), got
    assert got["dma"] == (0 if WG_NO_DMA else 1), got
    return got


def test_wgrad_strided_pointwise_plan(built):
    check_s2pw_plan()


@gpu
def test_wgrad_strided_pointwise_narrow_k():
    """Bit for bit, contiguous and as channel slices of sentinel-filled buffers, scale 1 and 2^-7."""
    geo = WGRAD_S2PW[0]
    B, Cin, H, W, N, k, s, p = geo
    got = check_s2pw_plan()
    x, dy, dw = wref(geo)
    tailv = torch.full((64,), FS, dtype=torch.float64)
    grad, splits = wgrad_launch(x, dy, dw.shape, s, p)
    assert splits == got["splits"], splits
    assert torch.equal(grad.double(), torch.cat([dw.reshape(-1), tailv])), f"{geo}: {first_mismatch(grad[:-64].view(dw.shape), dw)}"
    g2, _ = wgrad_launch(x, dy, dw.shape, s, p, 2.0 ** -7, ld_in=Cin + 24, ci=8, ld_dy=N + 24, cdy=16)
    want = torch.cat([dw.reshape(-1) * 2.0 ** -7, tailv])
    assert torch.equal(g2.double(), want), f"{geo} sliced: {first_mismatch(g2[:-64].view(dw.shape), dw * 2.0 ** -7)}"


# 3x3 / stride 1 / pad 1 with whole 32-channel chunks: (Cin, N) -> ROW3 <WN, RN, WC>; by default only N <= 32 (and Cin >= 256) take it,
# the others under KODHIP_WGRAD_ROW3=2 (the child run).  2 x 20 x 12 images: 480 rows, rows of 12 pixels against 32-row stages.
WGRAD_ROW3 = [((32, 32), (1, 1, 1)), ((64, 32), (1, 1, 2)), ((32, 64), (1, 2, 1)), ((64, 64), (1, 2, 2)), ((32, 96), (2, 2, 1)), ((64, 96), (2, 2, 2))]


@gpu
@pytest.mark.parametrize("cn,tpl", WGRAD_ROW3, ids=lambda v: "x".join(map(str, v)))
def test_wgrad_row3_templates(cn, tpl):
    geo = (2, cn[0], 20, 12, cn[1], 3, 1, 1)
    got = wgrad_plan(*geo)
    if WG_ROW3_ALL or (KNOB["KODHIP_WGRAD_ROW3"] is None and cn[1] <= 32):
        assert (got["row3"], got["wn"], got["rn"], got["wc"]) == (1, *tpl), got
    else:
        assert got["row3"] == 0, got
    x, dy, dw = wref(geo)
    for scale in (1.0, 2.0 ** -7):
        grad, _ = wgrad_launch(x, dy, dw.shape, 1, 1, scale, ld_in=cn[0] + 8, ci=8)
        assert torch.equal(grad[:-64].double(), (dw * scale).reshape(-1)), f"{geo}: {first_mismatch(grad[:-64].view(dw.shape), dw * scale)}"
        assert bool((grad[-64:] == FS).all())


# (B, Cin, H, W, N) -> (tn, tk) of the dual form; the last two (the small shape of the ROW3 list: 480 rows): N <= 32 with
# Kp = 160 / 288, one block over all of K, the <1, 5, 1, 1> / <1, 9, 1, 1> instances as the single form launches them.
WGRAD_DUAL = [((2, 64, 70, 65, 32), (32, 64)), ((2, 96, 9, 7, 48), (64, 128)), ((1, 256, 30, 20, 128), (128, 128)),
              ((2, 160, 20, 12, 32), (32, 160)), ((2, 288, 20, 12, 16), (32, 288))]


@gpu
@pytest.mark.parametrize("geo,cfg", WGRAD_DUAL, ids=lambda v: "x".join(map(str, v)))
def test_wgrad_dual_exact(geo, cfg):
    """kodhip_conv_wgrad_dual: two pointwise layers over one input (a channel slice), one launch; 48-channel pair: n tiles wider
    than a layer."""
    if WG_NO_DMA:
        assert wgrad_plan(geo[0], geo[1], geo[2], geo[3], geo[4], 1, 1, 0, dual=1, Kp=pad(geo[1], 32))["splits"] == 0
        return                                         # the form does not exist without the DMA kernel: the engine launches twice
    B, Cin, H, W, N = geo
    lib = _lib.lib()
    g = torch.Generator().manual_seed(sum(geo))
    x = int_tensor((B, Cin, H, W), 16, g)
    dys = [int_tensor((B, N, H, W), 8, g) for _ in range(2)]
    Kp = pad(Cin, 32)
    got = wgrad_plan(B, Cin, H, W, N, 1, 1, 0, dual=1, Kp=Kp, ldx=Cin + 16)
    assert (got["tn"], got["tk"]) == cfg, got
    sp = lib.kodhip_conv_wgrad_dual_splits(B, H, W, Cin + 16, Cin, N, Kp, N)
    assert sp == got["splits"] > 0
    xb = sliced(x, Cin + 16, 8, XS)
    dyb = [nhwc(d) for d in dys]
    part = torch.full((sp * 2 * N * Kp,), float("nan"), dtype=torch.float32, device="cuda")
    for scale in (1.0, 2.0 ** -7):
        gw = [torch.full((N * Cin + 64,), FS, dtype=torch.float32, device="cuda") for _ in range(2)]
        _lib.check(lib.kodhip_conv_wgrad_dual(xb.data_ptr(), dyb[0].data_ptr(), dyb[1].data_ptr(), part.data_ptr(), gw[0].data_ptr(),
                                              gw[1].data_ptr(), B, H, W, Cin + 16, 8, Cin, N, Kp, N, 0, scale, stream()), "wgrad_dual")
        torch.cuda.synchronize()
        X = x.double().permute(0, 2, 3, 1).reshape(-1, Cin)
        for i in range(2):
            D = dys[i].double().permute(0, 2, 3, 1).reshape(-1, N)
            assert float(D.abs().t().matmul(X.abs()).max()) < LIMIT
            want = torch.cat([(D.t() @ X).reshape(-1) * scale, torch.full((64,), FS, dtype=torch.float64)])
            assert torch.equal(gw[i].cpu().double(), want), f"{geo} layer {i} scale {scale}"


# ---- the stem ----------------------------------------------------------------------------------------------------------
# N = 32: the dedicated kernel; 48 / 64 at 2 x 20 x 72: conv_igemm_stem_kernel<32> (two 32-column tiles: at one round of blocks the
# plan prefers the narrower tile); N = 64 on a 520 x 520 image (529 pixel tiles: 1058 narrow tiles would need a second round):
# conv_igemm_stem_kernel<64>, the smallest image at which the plan takes it.
STEM_CASES = [(32, 2, 20, 72, 32), (48, 2, 20, 72, 32), (64, 2, 20, 72, 32), (64, 1, 520, 520, 64)]


@gpu
@pytest.mark.parametrize("N,B,H,W,bn", STEM_CASES, ids=lambda v: str(v))
def test_stem_exact(N, B, H, W, bn):
    """6x6 / stride 2 / pad 2 on an integer image through the pixel-pair layout: the dedicated kernel and both tile widths of the
    generic stem body; 36 pixel pairs per row (ragged tiles, both horizontal borders); the weight gradient's stem form
    (Kw = 160)."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(N)
    x, w = int_tensor((B, 3, H, W), 16, g), int_tensor((N, 3, 6, 6), 8, g)
    y, _, _ = conv_ref(x, w, 2, 2)
    assert conv_abs(x, w, 2, 2)[0].max().item() < LIMIT and rounding_share(y) >= 0.01
    dy = int_tensor(y.shape, 8, g)
    out = (C.c_int * 8)()
    _lib.check(lib.kodhip_conv_plan_query(0, B, H, W // 2, 8, 0, 32, N, 6, 1, 2, 1, 2, 1, 192, N, 0, out), "plan")
    if not NO_FAST:
        assert (out[0], out[1], out[2], out[3]) == (128, bn, 0, 1), list(out)
    img = torch.empty((B, H, W // 2, 8), dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.kodhip_nchw_to_nhwc4(x.cuda().data_ptr(), img.data_ptr(), B, 3, H, W, stream()), "nhwc4")
    pk = pack([w], stem=True)
    ob = torch.full((B, H // 2, W // 2, N + 16), YS, dtype=torch.bfloat16, device="cuda")
    M = B * (H // 2) * (W // 2)
    T = lib.kodhip_conv_stats_slots(M, N)
    stats = torch.full((2 * N * T,), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.kodhip_conv_fwd_raw(img.data_ptr(), pk["f"].data_ptr(), ob.data_ptr(), stats.data_ptr(), B, H, W // 2, 8, 0, 32, N, 6, 1, 2, 1, 2, 1,
                                 pk["Kp"], N + 16, 8, stream())
    if NO_FAST:
        assert rc < 0 and b"FAST" in lib.kodhip_last_error()       # wide-pixel taps exist on the FAST path only
    else:
        _lib.check(rc, "stem")
        torch.cuda.synchronize()
        same(ob, expect_buf(bf16_rne(y), N + 16, 8, YS), f"stem forward N={N}")
        assert bool(torch.isfinite(stats).all())
        # exact statistics (the dedicated kernel has its own statistics path and block cap) on scaled-down operands
        for bx, bw in stats_ranges(M, 108):
            gs = torch.Generator().manual_seed(N + bx)
            xs_, ws_ = int_tensor((B, 3, H, W), bx, gs), int_tensor((N, 3, 6, 6), bw, gs)
            ys_ = bf16_rne(conv_ref(xs_, ws_, 2, 2)[0])
            if float((ys_ * ys_).sum((0, 2, 3)).max()) < LIMIT:
                break
        else:
            raise AssertionError("no operand range keeps the stem statistics exact")
        print(f"STATS stem N={N} {H}x{W}: operands in [-{bx}, {bx}] x [-{bw}, {bw}], {rounding_share(conv_ref(xs_, ws_, 2, 2)[0]):.3f} of y rounds")
        _lib.check(lib.kodhip_nchw_to_nhwc4(xs_.cuda().data_ptr(), img.data_ptr(), B, 3, H, W, stream()), "nhwc4")
        pks = pack([ws_], stem=True)
        ob.fill_(YS); stats.fill_(float("nan"))
        _lib.check(lib.kodhip_conv_fwd_raw(img.data_ptr(), pks["f"].data_ptr(), ob.data_ptr(), stats.data_ptr(), B, H, W // 2, 8, 0, 32, N, 6, 1, 2,
                                           1, 2, 1, pks["Kp"], N + 16, 8, stream()), "stem (statistics operands)")
        torch.cuda.synchronize()
        same(ob, expect_buf(ys_, N + 16, 8, YS), f"stem forward N={N} (statistics operands)")
        stats_exact(stats.view(2, N, T), ys_.permute(0, 2, 3, 1), N, f"stem N={N}")
        _lib.check(lib.kodhip_nchw_to_nhwc4(x.cuda().data_ptr(), img.data_ptr(), B, 3, H, W, stream()), "nhwc4")      # back for the weight gradient
    dw = torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), 2, 2)
    assert torch.nn.grad.conv2d_weight(x.double().abs(), w.shape, dy.double().abs(), 2, 2).max().item() < LIMIT
    got = wgrad_plan(B, 8, H, W // 2, N, 6, 2, 2, Kp=160, kw=3, sw=1, pw=1)
    assert (got["tn"], got["tk"]) == ((32, 160) if N <= 32 else (64, 128)), got
    dyb = nhwc(dy)
    splits = lib.kodhip_conv_wgrad_splits_geo(B, H, W // 2, 8, 8, N, 6, 3, 2, 1, 2, 1, 160, N)
    part = torch.full((splits * N * 160,), float("nan"), dtype=torch.float32, device="cuda")
    for scale in (1.0, 2.0 ** -7):
        gw = torch.full((N * 108 + 64,), FS, dtype=torch.float32, device="cuda")
        _lib.check(lib.kodhip_conv_wgrad(img.data_ptr(), dyb.data_ptr(), part.data_ptr(), gw.data_ptr(), B, H, W // 2, 8, 0, 8, N, 6, 3, 2, 1, 2, 1,
                                         160, N, 0, N, 1, scale, stream()), "stem wgrad")
        torch.cuda.synchronize()
        want = torch.cat([dw.reshape(-1) * scale, torch.full((64,), FS, dtype=torch.float64)])
        assert torch.equal(gw.cpu().double(), want), f"stem wgrad N={N}: {first_mismatch(gw[:-64].cpu().view(dw.shape), dw * scale)}"


# ---- fp32 accumulation across producers (accumulate >> 8) -----------------------------------------------------------------
# form -> (B, Cin = dX channels, H, W, N = dY channels, k, s, p): the three output index forms (plain rows: pointwise, ROW3, dual;
# parity classes; folded depth-to-space), small ragged images.
F32_GEO = {"plain": (2, 48, 9, 7, 64, 1, 1, 0), "row3": (2, 32, 10, 6, 32, 3, 1, 1), "classes": (2, 48, 10, 6, 32, 3, 2, 1),
           "folded": (2, 32, 10, 6, 64, 3, 2, 1), "dual": (2, 64, 9, 7, 32, 1, 1, 0),
           # the fp32-mode instantiation of the 256-pixel tiles: dY 512 channels (K = 512), 16384 pixels, dX 64 channels
           "plain256": (1, 64, 128, 128, 512, 1, 1, 0)}


def f32_problem(form, seed):
    B, Cin, H, W, N, k, s, p = F32_GEO[form]
    g = torch.Generator().manual_seed(seed)
    w = int_tensor((N, Cin, k, k), 8, g)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = int_tensor((B, N, Ho, Wo), 8, g)
    xs = (B, Cin, H, W)
    S = torch.nn.grad.conv2d_input(xs, w.double(), dy.double(), s, p)
    kw = {}
    if form == "dual":
        w2, dy2 = int_tensor((N, Cin, 1, 1), 8, g), int_tensor((B, N, H, W), 8, g)
        S = S + torch.nn.grad.conv2d_input(xs, w2.double(), dy2.double(), 1, 0)
        kw = dict(dy2=dy2, w2=w2)
    assert float(S.abs().max()) < 2 ** 17                   # S + prior (multiples of 2^-6 below 2^10) is exact in fp32
    # priors: integers with fractional parts in steps of 2^-6
    prior = int_tensor(xs, 512, g) + torch.randint(0, 64, xs, generator=g).float() / 64
    return dict(w=w, dy=dy, S=S, prior=prior.double(), xs=xs, s=s, p=p, kw=kw, lform={"row3": "plain", "plain256": "plain"}.get(form, form))


@gpu
@pytest.mark.parametrize("bnred", [False, True], ids=["", "bnred"])
@pytest.mark.parametrize("form", list(F32_GEO))
def test_f32_modes(form, bnred):
    """Modes 1-4 of every entry point that takes dx_f32, on sentinel-filled dx and shadow buffers wider than the slice: the
    shadow's content, the SINGLE rounding of dx (the inputs make it differ from double rounding on >= 1 % of the elements),
    the shadow untouched by mode 3 and outside the slice, mode 4 without a shadow, modes 1-3 refused without one."""
    lib = _lib.lib()
    pr = f32_problem(form, 7)
    B, Cin, H, W = pr["xs"]
    S, prior = pr["S"], pr["prior"]
    if form == "plain256":
        assert conv_plan(1, *F32_GEO[form])["bm"] == 256
    ld, coff = Cin + 24, 8
    one, two = single_rounding(S, prior), double_rounding(S, prior)
    share = (one != two).double().mean().item()
    print(f"F32 {form}: single != double rounding on {share:.3f}")
    assert share >= 0.01, share
    run = lambda dx, mode, shadow: dgrad_launch(pr["lform"], pr["dy"], pr["w"], pr["xs"], pr["s"], pr["p"], dx, ld, coff, mode << 8, shadow,
                                                bnred=bnred, **pr["kw"])
    fresh = lambda: torch.full((B, H, W, ld), YS, dtype=torch.bfloat16, device="cuda")
    # mode 1
    dx, sh = fresh(), torch.full((B, H, W, ld), FS, dtype=torch.float32, device="cuda")
    _lib.check(run(dx, 1, sh), "mode 1")
    same(sh, expect_buf(S, ld, coff, FS), f"{form} mode 1 shadow")
    same(dx, expect_buf(bf16_rne(S), ld, coff, YS), f"{form} mode 1 dx")
    # mode 2
    dx, sh = fresh(), sliced(prior, ld, coff, FS, torch.float32)
    _lib.check(run(dx, 2, sh), "mode 2")
    same(sh, expect_buf(prior + S, ld, coff, FS), f"{form} mode 2 shadow")
    same(dx, expect_buf(one, ld, coff, YS), f"{form} mode 2 dx")
    # mode 3
    dx, sh = fresh(), sliced(prior, ld, coff, FS, torch.float32)
    before = sh.clone()
    _lib.check(run(dx, 3, sh), "mode 3")
    assert torch.equal(sh.view(torch.int32), before.view(torch.int32)), f"{form} mode 3 wrote the shadow"
    same(dx, expect_buf(one, ld, coff, YS), f"{form} mode 3 dx")
    # mode 4: dx's own bf16 content, no shadow
    g = torch.Generator().manual_seed(3)
    own = int_tensor(pr["xs"], 256, g) * 2.0
    dx = sliced(own, ld, coff, YS)
    _lib.check(run(dx, 4, None), "mode 4")
    want4 = bf16_rne(S + own.double())
    assert (want4 != accumulate_bf16(S, own)).double().mean() >= 0.01
    same(dx, expect_buf(want4, ld, coff, YS), f"{form} mode 4 dx")
    # modes 1-3 without a shadow: refused, nothing written
    for mode in (1, 2, 3):
        dx = fresh()
        assert run(dx, mode, None) < 0 and b"shadow" in lib.kodhip_last_error()
        assert bool((dx == YS).all())


@gpu
@pytest.mark.parametrize("form,bnred", [("dual", False)] + [(f, True) for f in ("plain", "row3", "classes", "folded", "dual")],
                         ids=lambda v: {True: "bnred", False: "unfused"}.get(v, v))
def test_twins_plain_and_accumulate(form, bnred):
    """The dual form and the fused-reduction twin of every data-gradient form with accumulate = 0 and with accumulate = 1 on
    independent prior content (the plain entry points are in test_exact_fwd_dgrad_wgrad)."""
    pr = f32_problem(form, 11)
    B, Cin, H, W = pr["xs"]
    S = pr["S"]
    assert rounding_share(S) >= 0.01
    ld, coff = Cin + 24, 8
    run = lambda dx, acc: dgrad_launch(pr["lform"], pr["dy"], pr["w"], pr["xs"], pr["s"], pr["p"], dx, ld, coff, acc, None, bnred=bnred, **pr["kw"])
    dx = torch.full((B, H, W, ld), YS, dtype=torch.bfloat16, device="cuda")
    _lib.check(run(dx, 0), form)
    same(dx, expect_buf(bf16_rne(S), ld, coff, YS), f"{form} bnred={bnred}")
    prior = int_tensor(pr["xs"], 256, torch.Generator().manual_seed(5))
    dx = sliced(prior, ld, coff, YS)
    _lib.check(run(dx, 1), form + " accumulate")
    same(dx, expect_buf(accumulate_bf16(S, prior), ld, coff, YS), f"{form} bnred={bnred} accumulate")


@gpu
@pytest.mark.parametrize("form", ["plain", "classes", "folded"])
def test_f32_producer_chain(form):
    """First, middle and last producer over one buffer: dx = bf16_rne(S1 + S2 + S3), rounded once; the shadow ends as S1 + S2."""
    prs = [f32_problem(form, 20 + i) for i in range(3)]
    B, Cin, H, W = prs[0]["xs"]
    ld, coff = Cin + 24, 8
    dx = torch.full((B, H, W, ld), YS, dtype=torch.bfloat16, device="cuda")
    sh = torch.full((B, H, W, ld), FS, dtype=torch.float32, device="cuda")
    for mode, pr in zip((1, 2, 3), prs):
        _lib.check(dgrad_launch(pr["lform"], pr["dy"], pr["w"], pr["xs"], pr["s"], pr["p"], dx, ld, coff, mode << 8, sh, **pr["kw"]), f"mode {mode}")
    total = prs[0]["S"] + prs[1]["S"] + prs[2]["S"]
    chain = bf16_rne(bf16_rne(bf16_rne(prs[0]["S"]) + bf16_rne(prs[1]["S"])) + bf16_rne(prs[2]["S"]))
    assert (bf16_rne(total) != chain).double().mean() >= 0.01
    same(sh, expect_buf(prs[0]["S"] + prs[1]["S"], ld, coff, FS), f"{form} chain shadow")
    same(dx, expect_buf(bf16_rne(total), ld, coff, YS), f"{form} chain dx")


# ---- the bodies behind the knobs -------------------------------------------------------------------------------------------
KNOB_RUNS = [
    # KODHIP_ROW3=0: 3x3 / stride 1 through the generic FAST kernel (conv_igemm_kernel<.., FAST>), its 256-pixel tiles included
    ("KODHIP_ROW3", "0", ""),
    # KODHIP_NO_FAST=1: every convolution through the register-staged kernel (conv_igemm_kernel<.., false>); fp32 modes, the fused
    # reduction and the folded form are refused there by design
    ("KODHIP_NO_FAST", "1", "not test_f32 and not test_twins and not test_wgrad"),
    # KODHIP_WGRAD_ROW3=2: every eligible 3x3 / stride 1 weight gradient through conv_wgrad_row3_kernel (all six wave layouts)
    ("KODHIP_WGRAD_ROW3", "2", "test_wgrad or test_exact"),
    # KODHIP_WGRAD_DMA=none: the register-staged conv_wgrad_kernel
    ("KODHIP_WGRAD_DMA", "none", "test_wgrad or test_exact or test_stem"),
    # KODHIP_S2_SEPARATE=1: the parity classes as four launches of conv_igemm_kernel in place of conv_igemm_x4_kernel (the fused
    # reduction of the classes exists in the merged launch only: kodhip_conv_dgrad_bnred_slots answers 0)
    ("KODHIP_S2_SEPARATE", "1", "(s2 or classes) and not bnred"),
    # KODHIP_FORCE_BN=128: the 128-column tiles (plain, ROW3, merged classes, their fp32-mode instantiations) at the small shapes;
    # by default the plan takes them only where narrower tiles would need a second round of blocks (multi_pw)
    ("KODHIP_FORCE_BN", "128", "test_exact or test_f32 or test_twins"),
]


@gpu
@pytest.mark.parametrize("knob,value,select", KNOB_RUNS, ids=[k + "=" + v for k, v, _ in KNOB_RUNS])
def test_bodies_behind_the_knobs(knob, value, select):
    """This file again in a fresh process per setting (the knobs are read once per process); one child at a time."""
    if any(v is not None for v in KNOB.values()):
        pytest.skip("already inside a knob run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **{knob: value})
    k = "not test_bodies_behind_the_knobs" + (f" and ({select})" if select else "")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k", k],
                       capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "passed" in r.stdout
