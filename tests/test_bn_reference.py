"""Pins the float64 BatchNorm reference of tests/bn_reference.py (the yardstick of tests/test_hip_bn_stats.py) to
torch.nn.BatchNorm2d and autograd in float64 - on the CPU, no GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import bn_reference as R

ACTS = [(R.SILU, 0.0), (R.RELU, 0.0), (R.LEAKY, 0.1), (R.HARDSWISH, 0.0), (R.IDENTITY, 0.0)]


def _rows(t):
    """NCHW -> [M, C] rows."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _close(a, b, what, tol=1e-12):
    a, b = a.double(), b.double()
    err = ((a - b).abs() / (1 + b.abs())).max().item()
    assert err <= tol, f"{what}: {err:.3g}"


@pytest.mark.parametrize("kind,slope", ACTS)
@pytest.mark.parametrize("res", [False, True])
def test_train_mode_reference_matches_torch(kind, slope, res):
    g = torch.Generator().manual_seed(7 + kind)
    B, C, H, W = 3, 5, 4, 3
    offs = torch.tensor([0.0, 8.0, -64.0, 1.0, 0.5], dtype=torch.float64)
    y = (torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 2 + offs.view(1, C, 1, 1) * 2)
    y[0, 3, 0, 0] = 3.0
    gamma = torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    resid = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) if res else None
    bn = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.03).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
        bn.running_mean.copy_(torch.randn(C, generator=g)); bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    yr = y.clone().requires_grad_(True)
    out = R.act(kind, bn(yr), slope)
    if res:
        out = out + resid
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dout)

    got, z, mean, var, rstd = R.bn_act_forward(_rows(y), gamma, beta, 1e-3, kind, slope, _rows(resid) if res else None)
    _close(got, _rows(out.detach()), "forward")
    m, vb, vu = R.batch_stats(_rows(y))
    _close(m, y.mean((0, 2, 3)), "mean")
    _close(vb, y.var((0, 2, 3), unbiased=False), "biased var")
    _close(vu, y.var((0, 2, 3), unbiased=True), "unbiased var")
    rm, rv = R.running_update(rm0, rv0, m, vu, 0.03)
    _close(rm, bn.running_mean, "running_mean")
    _close(rv, bn.running_var, "running_var")
    rs, sc, sh = R.affine(m, vb, gamma, beta, 1e-3)
    _close(_rows(y) * sc + sh, z, "scale / shift")
    dX, dgamma, dbeta, dz = R.bn_act_backward(_rows(y), _rows(dout), gamma, beta, 1e-3, kind, slope)
    _close(dX, _rows(yr.grad), "dX", 1e-10)
    _close(dgamma, bn.weight.grad, "dgamma", 1e-10)
    _close(dbeta, bn.bias.grad, "dbeta", 1e-10)
    _close(R.bn_act_backward(_rows(y), _rows(dout), gamma, beta, 1e-3, kind, slope, z_side=z)[0], dX, "dX at z_side = z")
    # the coefficient form rebuilds dX from (sum dz, sum dz*xhat) alone
    k1, k2, k3 = R.bwd_coeffs(dbeta, dgamma, y.numel() // C, gamma, m, rs)
    _close(k1 * dz + k2 * _rows(y) + k3, _rows(yr.grad), "k1 dz + k2 y + k3", 1e-10)


@pytest.mark.parametrize("kind,slope", ACTS)
def test_activation_gradient_at_the_kinks(kind, slope):
    z = torch.tensor([-4.0, -3.0, -1.0, 0.0, 1e-3, 1.0, 3.0, 4.0], dtype=torch.float64, requires_grad=True)
    R.act(kind, z, slope).sum().backward()
    _close(R.act_grad(kind, z.detach(), slope), z.grad, "act'")
    zz = torch.linspace(-8, 8, 4001, dtype=torch.float64)
    assert R.act_grad(kind, zz, slope).abs().max().item() <= R.act_lipschitz(kind, slope)


@pytest.mark.parametrize("kind,slope", ACTS)
def test_eval_mode_reference_matches_torch(kind, slope):
    g = torch.Generator().manual_seed(3)
    B, C, H, W = 2, 4, 3, 5
    y = torch.randn(B, C, H, W, generator=g, dtype=torch.float64) * 3 + 1
    bn = torch.nn.BatchNorm2d(C, eps=1e-3).double().eval()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5); bn.bias.copy_(torch.randn(C, generator=g))
        bn.running_mean.copy_(torch.randn(C, generator=g)); bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    yr = y.clone().requires_grad_(True)
    out = R.act(kind, bn(yr), slope)
    dout = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(dout)
    args = (bn.running_mean, bn.running_var, bn.weight.detach(), bn.bias.detach(), 1e-3, kind, slope)
    _close(R.bn_eval_forward(_rows(y), *args), _rows(out.detach()), "eval forward")
    dX, dgamma, dbeta = R.bn_eval_backward(_rows(y), _rows(dout), *args)
    _close(dX, _rows(yr.grad), "eval dX")
    _close(dgamma, bn.weight.grad, "eval dgamma")
    _close(dbeta, bn.bias.grad, "eval dbeta")


def test_error_model_bounds_fp32_sums():
    """gamma(c) * sum |x| bounds a sequential fp32 sum of c + 1 terms (data with a large common offset, the
    cancellation case), and stats_bounds / affine_bounds / running_bounds contain the fp32 results computed from
    such sums."""
    g = torch.Generator().manual_seed(0)
    n, C = 4096, 3
    y = (torch.randn(n, C, generator=g) * torch.tensor([1.0, 0.1, 0.01]) + torch.tensor([0.0, 8.0, 64.0])).float()
    s0 = torch.zeros(C, dtype=torch.float32)
    s1 = torch.zeros(C, dtype=torch.float32)
    for i in range(n):                                   # fp32 recursive sums (c = n - 1 roundings of the first term)
        s0 = s0 + y[i]
        s1 = s1 + y[i] * y[i]
    yd = y.double()
    e0 = R.gamma_n(n - 1) * yd.abs().sum(0)
    e1 = R.gamma_n(n) * (yd * yd).sum(0)
    assert ((s0.double() - yd.sum(0)).abs() <= e0).all()
    assert ((s1.double() - (yd * yd).sum(0)).abs() <= e1).all()
    mean, var, rstd, dmean, dvar, drstd = R.stats_bounds(yd.sum(0), (yd * yd).sum(0), e0, e1, n, 1e-3)
    m32 = s0.double() / n
    v32 = (s1.double() / n - m32 * m32).clamp_min(0)
    r32 = R.f32(1.0 / torch.sqrt(v32 + 1e-3))
    assert ((R.f32(m32) - mean).abs() <= dmean).all()
    assert ((v32 - var).abs() <= dvar).all()
    assert ((r32 - rstd).abs() <= drstd).all()
    _close(var, yd.var(0, unbiased=False), "var", 1e-9)
    gamma, beta = torch.tensor([1.0, 0.5, 2.0]), torch.tensor([0.1, -0.2, 0.3])
    sc, sh, dsc, dsh = R.affine_bounds(mean, rstd, dmean, drstd, gamma, beta)
    sc32 = R.f32(gamma.double() * r32)
    sh32 = R.f32(beta.double() - R.f32(R.f32(m32) * sc32))
    assert ((sc32 - sc).abs() <= dsc).all() and ((sh32 - sh).abs() <= dsh).all()
    rm0, rv0 = torch.zeros(C), torch.ones(C)
    rm, rv, drm, drv = R.running_bounds(rm0, rv0, mean, var, n, 0.03, dmean, dvar)
    unb32 = R.f32(v32 * n / (n - 1))
    rm32 = R.f32(R.f32(0.97 * rm0.double()) + R.f32(0.03 * R.f32(m32)))
    rv32 = R.f32(R.f32(0.97 * rv0.double()) + R.f32(0.03 * unb32))
    assert ((rm32 - rm).abs() <= drm).all() and ((rv32 - rv).abs() <= drv).all()


def _bf(t):
    return t.to(torch.bfloat16).float()


def test_fma32_is_one_rounding():
    """fma32 on operands built to need the exact path - sums that fp64 cannot hold, one of them landing on an fp32
    midpoint after fp64's rounding (the double-rounding case) - against expected values worked out by hand, and on
    random operands against the definition of round-to-nearest-even, checked in exact rational arithmetic without the
    rounding helper fma32 itself uses."""
    import numpy as np
    from fractions import Fraction
    e = 2.0 ** -23
    # (1 + e)^2 + 2^24 = 2^24 + 1 + 2^-22 + 2^-46: just above the midpoint 2^24 + 1 (fp32 spacing 2 there)  -> 2^24 + 2
    # (1 + e)(1 - e) + 2^30 = 2^30 + 1 - 2^-46: fp32 spacing 128 there                                       -> 2^30
    # (1 + e)(1 - e) + (2^24 + 2) = 2^24 + 3 - 2^-46: fp64 rounds it ONTO the midpoint 2^24 + 3, from which ties-to-even
    #   would go up to 2^24 + 4; the exact value lies below the midpoint                                     -> 2^24 + 2
    a = torch.tensor([1 + e, 1 + e, 1 + e]); b = torch.tensor([1 + e, 1 - e, 1 - e]); c = torch.tensor([2.0 ** 24, 2.0 ** 30, 2.0 ** 24 + 2])
    slow0 = R.FMA_SLOW[0]
    got = R.fma32(a, b, c)
    assert R.FMA_SLOW[0] == slow0 + 3                             # all three took the exact path
    assert got.tolist() == [2.0 ** 24 + 2, 2.0 ** 30, 2.0 ** 24 + 2]
    g = torch.Generator().manual_seed(1)
    a, b, c = (torch.randn(300, generator=g) * s for s in (1.0, 1.0, 1e-3))
    got = R.fma32(a, b, c)
    for i in range(a.numel()):
        v = Fraction(a[i].item()) * Fraction(b[i].item()) + Fraction(c[i].item())
        r = np.float32(got[i].item())
        d = abs(Fraction(float(r)) - v)
        for nb in (np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))):
            dn = abs(Fraction(float(nb)) - v)
            assert d < dn or (d == dn and int(r.view(np.int32)) % 2 == 0), i


@pytest.mark.parametrize("kind,slope", ACTS[1:])
@pytest.mark.parametrize("res", [False, True])
def test_fp32_restatement_within_the_fp64_reference(kind, slope, res):
    """apply32 / bwd_apply32 against this file's fp64 reference, kinks 0, -3 and 3 included: the fp32 restatement
    differs from the exact value by the activation's fp32 error (relerr_bound), one fma rounding of z carried through
    the activation's Lipschitz constant, the add and the bf16 rounding."""
    g = torch.Generator().manual_seed(11 + kind)
    M, C = 64, 8
    y = _bf(torch.randn(M, C, generator=g) * 3)
    scale = _bf(torch.rand(C, generator=g) + 0.5); shift = _bf(torch.randn(C, generator=g))
    y[0] = _bf((torch.tensor([0.0, -3.0, 3.0, 0.0, -3.0, 3.0, 1.0, -1.0]) - shift) / scale)   # near the kinks
    scale[:3] = 1.0; shift[:3] = 0.0; y[1, :3] = torch.tensor([0.0, -3.0, 3.0])              # exactly on them
    resid = _bf(torch.randn(M, C, generator=g)) if res else None
    z = y.double() * scale.double() + shift.double()
    want = R.act(kind, z, slope) + (resid.double() if res else 0.0)
    got = R.apply32(y.bfloat16(), scale, shift, kind, slope, resid.bfloat16() if res else None).double()
    L = R.act_lipschitz(kind, slope)
    pre = R.relerr_bound(kind, z) + L * R.ulp32(z) + R.ulp32(want)
    assert ((got - want).abs() <= pre + R.ulpbf16(want) / 2 + R.ulpbf16(pre)).all()
    # backward: dz exact up to the side of a kink z's rounding fell on (none here: z is exact in fp32 for these operands
    # except by one rounding, and the kink rows are exact), then two fmas
    dA = _bf(torch.randn(M, C, generator=g))
    coef = _bf(torch.randn(3 * C, generator=g))
    z32 = R.fma32(y, scale, shift)
    dz = dA.double() * R.act_grad(kind, z32.double(), slope)
    wantb = coef[:C].double() * dz + coef[C:2 * C].double() * y.double() + coef[2 * C:].double()
    gotb = R.bwd_apply32(dA.bfloat16(), y.bfloat16(), scale, shift, coef, kind, slope).double()
    mag = (coef[:C].double() * dz).abs() + (coef[C:2 * C].double() * y.double()).abs() + coef[2 * C:].double().abs()
    preb = 6 * R.U32 * mag
    assert ((gotb - wantb).abs() <= preb + R.ulpbf16(wantb) / 2 + R.ulpbf16(preb)).all()
