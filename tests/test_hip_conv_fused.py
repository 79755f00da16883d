"""kodhip_conv_fwd_fused (eval forward: BatchNorm + activation (+ residual) in the convolution's epilogue) against float64.

Identity / ReLU / LeakyReLU in the exact regime of tests/fused_reference.py: torch.equal against bf16_rne(act(z)), with a
residual against bf16_rne(bf16_rne(act(z)) + r) - the two-rounding contract, which differs from one rounding on 1.7 - 18 %
of the elements (asserted on the CPU in tests/test_eval_fused_host.py).  SiLU / Hardswish: equal to bf16_rne of the
float64 activation, or one bf16 step off where that lies within 2^-16 |a| of a rounding boundary.

Every geometry asserts the launch plan it was written for (kodhip_conv_plan_query op 0: the fused mode shares the plan of
kodhip_conv_fwd_raw) under the knob conventions of tests/test_hip_conv_exact.py; the bodies behind KODHIP_NO_FAST=1 and
KODHIP_ROW3=0 run this file again in a child process each.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from object_detection_cib_amd import _lib  # noqa: E402
from fused_reference import (ACT_HARDSWISH, ACT_SILU, CASES, EXACT_ACTS, SLOPE, SMOOTH_CASES, STEM_CASES, check_exact_conditions,  # noqa: E402
                             check_smooth, check_smooth_conditions, expected_exact, problem, stem_problem)
from hip_helpers import pack, stream  # noqa: E402
from test_hip_conv_exact import NO_FAST, ROW3_OFF, XS, YS, conv_plan, expect_buf, expect_conv_plan, same, sliced  # noqa: E402

gpu = pytest.mark.gpu


def fused_launch(pr, geo, act, residual, pk, xb, ld_in, ci):
    """-> output buffer [B, Ho, Wo, N + 16] (slice at channel 8) pre-filled with the sentinel"""
    lib = _lib.lib()
    B, Cin, H, W, N, k, s, p = geo
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    out = torch.full((B, Ho, Wo, N + 16), YS, dtype=torch.bfloat16, device="cuda")
    sc, sh = pr["scale"].float().cuda(), pr["shift"].float().cuda()
    rb = sliced(pr["res"], N + 24, 16, XS) if residual else None
    _lib.check(lib.kodhip_conv_fwd_fused(xb.data_ptr(), pk["f"].data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                         rb.data_ptr() if residual else None, N + 24 if residual else 0, 16 if residual else 0,
                                         out.data_ptr(), B, H, W, ld_in, ci, Cin, N, k, k, s, s, p, p, pk["Kp"], N + 16, 8,
                                         act, SLOPE, stream()), "conv_fwd_fused")
    torch.cuda.synchronize()
    return out


def operands(cid, pr):
    geo, _, slice_in, _ = CASES[cid]
    Cin = geo[1]
    ld_in, ci = (Cin + 16, 8) if slice_in else (Cin, 0)
    return pack([pr["w"]]), sliced(pr["x"], ld_in, ci, XS), ld_in, ci


def assert_plan(cid):
    geo, plan, _, multi = CASES[cid]
    B, Cin, H, W, N, k, s, p = geo
    got = conv_plan(0, B, Cin, H, W, N, k, s, p)
    expect_conv_plan(got, plan, (cid, "fused"), N)
    if multi and not NO_FAST and not ROW3_OFF:
        assert got["tiles_m"] > got["groups_m"], (cid, got)
    return got


@gpu
@pytest.mark.parametrize("cid", list(CASES))
def test_fused_exact(cid):
    """Identity / ReLU / LeakyReLU, without and with a residual: the stored value is determined, the sentinel survives
    outside the output slice."""
    geo, _, _, _ = CASES[cid]
    N = geo[4]
    got = assert_plan(cid)
    pr = problem(cid)
    pk, xb, ld_in, ci = operands(cid, pr)
    for act in EXACT_ACTS:
        for residual in (False, True):
            what = f"{cid} act {act}{' + residual' if residual else ''}"
            share, differ = check_exact_conditions(what, pr, act, residual)
            print(f"EXACT {what}: act(z) rounds {share:.3f}, two roundings differ from one on {differ:.3f}")
            out = fused_launch(pr, geo, act, residual, pk, xb, ld_in, ci)
            same(out, expect_buf(expected_exact(pr, act, residual)[0], N + 16, 8, YS), what, got["bm"], got["bn"])


@gpu
@pytest.mark.parametrize("N,B,H,W,bn", STEM_CASES, ids=lambda v: str(v))
def test_fused_stem_exact(N, B, H, W, bn):
    """The stem through the pixel-pair layout: the dedicated kernel (N = 32) and both tile widths of the generic stem body."""
    lib = _lib.lib()
    pr = stem_problem(N, B, H, W)
    out8 = (C.c_int * 8)()
    _lib.check(lib.kodhip_conv_plan_query(0, B, H, W // 2, 8, 0, 32, N, 6, 1, 2, 1, 2, 1, 192, N, 0, out8), "plan")
    if not NO_FAST:
        assert (out8[0], out8[1], out8[2], out8[3]) == (128, bn, 0, 1), list(out8)
    img = torch.empty((B, H, W // 2, 8), dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.kodhip_nchw_to_nhwc4(pr["x"].cuda().data_ptr(), img.data_ptr(), B, 3, H, W, stream()), "nhwc4")
    pk = pack([pr["w"]], stem=True)
    sc, sh = pr["scale"].float().cuda(), pr["shift"].float().cuda()
    for act in EXACT_ACTS:
        for residual in (False, True):
            what = f"stem N={N} act {act}{' + residual' if residual else ''}"
            check_exact_conditions(what, pr, act, residual)
            ob = torch.full((B, H // 2, W // 2, N + 16), YS, dtype=torch.bfloat16, device="cuda")
            rb = sliced(pr["res"], N + 24, 16, XS) if residual else None
            rc = lib.kodhip_conv_fwd_fused(img.data_ptr(), pk["f"].data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                           rb.data_ptr() if residual else None, N + 24 if residual else 0, 16 if residual else 0,
                                           ob.data_ptr(), B, H, W // 2, 8, 0, 32, N, 6, 1, 2, 1, 2, 1, pk["Kp"], N + 16, 8,
                                           act, SLOPE, stream())
            if NO_FAST:
                assert rc < 0 and b"FAST" in lib.kodhip_last_error()       # wide-pixel taps exist on the FAST path only
                continue
            _lib.check(rc, what)
            torch.cuda.synchronize()
            same(ob, expect_buf(expected_exact(pr, act, residual)[0], N + 16, 8, YS), what, 128, bn)


@gpu
@pytest.mark.parametrize("act", [ACT_SILU, ACT_HARDSWISH], ids=["silu", "hardswish"])
@pytest.mark.parametrize("cid", SMOOTH_CASES)
def test_fused_silu_hardswish(cid, act):
    """bf16_rne of the float64 activation, one bf16 step off only within 2^-16 |a| of a rounding boundary."""
    geo, _, _, _ = CASES[cid]
    N = geo[4]
    assert_plan(cid)
    pr = problem(cid, True)
    what = f"{cid} act {act}"
    check_smooth_conditions(what, pr, act)
    pk, xb, ld_in, ci = operands(cid, pr)
    out = fused_launch(pr, geo, act, False, pk, xb, ld_in, ci).cpu().double()
    assert bool((out[..., :8] == YS).all()) and bool((out[..., 8 + N:] == YS).all()), f"{what}: the sentinel outside the slice"
    check_smooth(what, out[..., 8:8 + N].permute(0, 3, 1, 2), pr, act)


# ---- the bodies behind the knobs -------------------------------------------------------------------------------------------
# KODHIP_NO_FAST=1: the register-staged kernel (conv_igemm_kernel<.., MODE_FUSED*, false>); the stem expects the "FAST" refusal.
# KODHIP_ROW3=0: 3x3 / stride 1 through the generic FAST kernel.
KNOB_RUNS = [("KODHIP_NO_FAST", "1"), ("KODHIP_ROW3", "0")]


@gpu
def test_fused_bodies_behind_the_knobs():
    """This file again in a fresh process per setting (the knobs are read once per process), one child at a time, each under
    its own timeout; a child that ends by a signal or a time limit fails the test there and no further child is started."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for knob, value in KNOB_RUNS:
        env = dict(os.environ, **{knob: value})
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                            "not test_fused_bodies_behind_the_knobs"], capture_output=True, text=True, timeout=300, env=env, cwd=root)
        assert r.returncode >= 0, f"{knob}={value}: the child ended by signal {-r.returncode}\n" + r.stdout[-3000:] + r.stderr[-1000:]
        assert r.returncode == 0, f"{knob}={value}\n" + r.stdout[-3000:] + r.stderr[-1000:]
        assert "passed" in r.stdout
