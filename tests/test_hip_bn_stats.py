"""Train-mode BatchNorm statistics and backward coefficients of the HIP chain against the float64 reference of
tests/bn_reference.py (itself pinned to torch.nn.BatchNorm2d by tests/test_bn_reference.py).

The chain: a producer writes per-slot fp32 partial sums (forward: the conv epilogue; backward: the fused data-gradient
epilogue or the bwd_reduce pass), a finalize kernel adds the slots in fp64 and forms the constants
(kodhip_bn_finalize_partials / kodhip_bn_bwd_coeffs_partials[2] / _eval_*), an apply pass uses them.

Tolerances come from an error model, not from observed errors.  A partial is an fp32 sum; a term that passes through
at most c fp32 roundings on its way into its slot is off by at most gamma(c) = c u / (1 - c u) of its size
(u = 2^-24), so a channel's sum is within gamma(c) * sum |terms| of the exact one, plus T u64 * sum |terms| for the
fp64 addition of the T slots.  The chain c of one term:
* forward conv epilogue (conv_igemm.hip, MODE_RAW): the thread's accumulator runs over every tile of its group,
  BM * BN / (8 * threads) rows per tile (tiles per group x rows), then log2(64 / (BN / 8)) shuffle levels, then the
  cross-wave sum over the block's threads / 64 waves; the sum of squares rounds each product once more (c + 1).
  BM, BN, the groups and the tile band of every group come from a mirror of the launch plan (make_plan: M, N, K).
  The stem kernel (N <= 32): 128 x 32 tiles, 2 rows per thread per tile, 4 shuffle levels, 4 waves, min(tiles, 768)
  blocks over the same kind of bands.
* fused data-gradient epilogue (MODE_PLAIN_BN): <= 8 rows per tile in the thread, <= 4 shuffle levels, then the block's
  running value takes <= 8 wave sums per tile of its group: c <= 12 + 8 * tiles per group, with the tiles per group
  bounded by ceil(ceil(M / 128) / groups) + 1 and the groups read from the slot count the launch reports.
* bn_*_bwd_reduce: ceil(M / (grid * rows per block)) rows in the thread, then the block's rpb row lanes in fixed order;
  the second sum's terms dz * (y - mean) * rstd are rounded three times before they are added (c + 3).
These bounds on the two sums are pushed through mean, var, rstd, scale, shift, the running update and the backward
coefficients by interval arithmetic (bn_reference.stats_bounds / affine_bounds / running_bounds and _dk_bounds /
_bwd_bounds below); the apply passes add their fp32 roundings, the activation's own error and the final bf16 rounding.
Every check asserts |kernel - reference| <= bound elementwise and prints the worst err / bound (pytest -rP shows it).
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import bn_reference as R  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from hip_helpers import bf, conv_fwd_raw, nhwc, pack, pad, stream  # noqa: E402

EPS, MOM = 1e-3, 0.03
NAN = float("nan")
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))
ACTS = [(R.SILU, 0.0), (R.RELU, 0.0), (R.LEAKY, 0.1), (R.HARDSWISH, 0.0), (R.IDENTITY, 0.0)]


def _check(got, want, bound, what):
    """|got - want| <= bound elementwise (NaN fails); returns the worst err / bound."""
    dev = want.device
    got, want, bound = got.double().to(dev), want.double(), bound.double().to(dev)
    err = (got - want).abs()
    ratio = err / bound.clamp_min(1e-300)
    bad = ~(err <= bound)
    if bad.any():
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{what}: {int(bad.sum())}/{err.numel()} outside the bound, first at {i}: got "
                             f"{got.flatten()[i].item():.9g} want {want.flatten()[i].item():.9g} bound "
                             f"{bound.flatten()[i].item():.3g}; worst err/bound {ratio.nan_to_num(math.inf).max().item():.3g}")
    return ratio.max().item() if ratio.numel() else 0.0


def _ulp_eq(got, want, what, ulps=1):
    """fp32 results within `ulps` units in the last place of the fp32 value of `want`."""
    want = want.double()
    return _check(got, want, ulps * R.ulp32(want), what)


def _report(group, worst):
    print(f"[bn-stats] {group}: worst err/bound {max(worst.values()):.3g} "
          f"({', '.join(f'{k} {v:.3g}' for k, v in worst.items())})")


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


# ---------------------------------------------------------------- a. forward finalize on synthetic slabs
def _finalize_expected(s0, s1, n, gamma, beta, rm0, rv0, mom):
    """The finalize's fp64 formula rounded to fp32; scale / shift / running update as the fp32 expressions."""
    mean = s0 / n
    var = (s1 / n - mean * mean).clamp_min(0.0)
    rstd = R.f32(1.0 / torch.sqrt(var + EPS32))
    mean_f = R.f32(mean)
    sc = R.f32(gamma.double() * rstd)
    sh = R.f32(beta.double() - R.f32(mean_f * sc))
    unb = var * n / (n - 1) if n > 1 else var
    m = float(torch.tensor(mom, dtype=torch.float32))
    rm = R.f32(R.f32(R.f32(1 - m) * rm0.double()) + R.f32(m * mean_f))
    rv = R.f32(R.f32(R.f32(1 - m) * rv0.double()) + R.f32(m * R.f32(unb)))
    return mean_f, rstd, sc, sh, rm, rv


def _run_finalize(route, slab, T, n, gamma, beta, rm, rv, mom, C_, update=1):
    lib = _lib.lib()
    aff = _nan(4 * C_)
    a = aff.data_ptr()
    if route == "fused":
        _lib.check(lib.kodhip_bn_finalize_partials(slab.data_ptr(), T, float(n), gamma.data_ptr(), beta.data_ptr(),
                                                   rm.data_ptr(), rv.data_ptr(), mom, EPS, a, a + 4 * C_, a + 8 * C_,
                                                   a + 12 * C_, C_, update, stream()), "finalize_partials")
    else:
        sums = _nan(2 * C_, dtype=torch.float64)
        _lib.check(lib.kodhip_bn_reduce_partials(slab.data_ptr(), sums.data_ptr(), C_, T, stream()), "reduce_partials")
        _lib.check(lib.kodhip_bn_finalize(sums.data_ptr(), float(n), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                                          rv.data_ptr(), mom, EPS, a, a + 4 * C_, a + 8 * C_, a + 12 * C_, C_, update,
                                          stream()), "finalize")
    torch.cuda.synchronize()
    return aff.view(4, C_).cpu()


def _synthetic_slab(C_, T, rows, g):
    """[2][C][T] fp32 partials of `rows` values per slot: integers (fp64 sums exact in any order) with channel mean
    offsets 0, 8 and 64 x the spread; sum y^2 >= (sum y)^2 / rows per slot, so var >= 0."""
    off = torch.tensor([0.0, 8.0, 64.0])[torch.arange(C_) % 3].double() * 16
    p0 = torch.randint(-64 * rows, 64 * rows + 1, (C_, T), generator=g).double() + rows * off[:, None]
    p1 = torch.ceil(p0 * p0 / rows) + torch.randint(0, 4096 * rows, (C_, T), generator=g).double()
    return torch.stack((p0, p1)).float().double()


FIN_T = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3001]


@pytest.mark.parametrize("C_", [1, 3, 8, 65])
def test_finalize_partials_synthetic(C_):
    """kodhip_bn_finalize_partials and reduce_partials + finalize on [2][C][T] slabs over the slot counts around the
    4-pass / tail / fallback boundaries of wave_sum_partials2, slab bases offset by 0..3 floats (rows alternate
    16-byte alignment): mean and rstd are the fp64 formula rounded to fp32, scale / shift / running statistics the fp32
    expressions (<= 1 ulp), and the two routes agree bit for bit."""
    g = torch.Generator().manual_seed(C_)
    worst = {}
    for T in FIN_T:
        rows = 16
        n = float(T * rows)
        parts = _synthetic_slab(C_, T, rows, g)
        gamma, beta = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
        rm0, rv0 = torch.randn(C_, generator=g), torch.rand(C_, generator=g) + 0.5
        want = _finalize_expected(parts[0].sum(1), parts[1].sum(1), n, gamma, beta, rm0, rv0, MOM)
        for off in range(4):
            buf = _nan(2 * C_ * T + 8)
            slab = buf[off:off + 2 * C_ * T]
            slab.copy_(parts.flatten().float())
            outs = {}
            for route in ("fused", "reduce"):
                rm, rv = rm0.cuda(), rv0.cuda()
                aff = _run_finalize(route, slab, T, n, gamma.cuda(), beta.cuda(), rm, rv, MOM, C_)
                outs[route] = (aff, rm.cpu(), rv.cpu())
                what = f"C={C_} T={T} off={off} {route}"
                assert torch.equal(aff[2].double(), want[0]), what + ": mean != fp32(fp64 mean)"
                assert torch.equal(aff[3].double(), want[1]), what + ": rstd != fp32(fp64 rstd)"
                for key, got, ref in (("scale", aff[0], want[2]), ("shift", aff[1], want[3]),
                                      ("running_mean", rm, want[4]), ("running_var", rv, want[5])):
                    worst[key] = max(worst.get(key, 0), _ulp_eq(got, ref, f"{what} {key}"))
            for x, y in zip(outs["fused"], outs["reduce"]):
                assert torch.equal(x, y), f"C={C_} T={T} off={off}: the two routes differ"
    _report(f"finalize synthetic C={C_}", worst)


@pytest.mark.parametrize("T", [5, 257, 1024, 3001])
def test_finalize_routes_bit_identical_on_inexact_sums(T):
    """Random fp32 partials (inexact sums): both routes add in the same order, so their constants are bit-identical,
    and within the fp64 summation bound of the exact statistics."""
    g = torch.Generator().manual_seed(T)
    C_ = 9
    parts = torch.randn(2, C_, T, generator=g) * 100
    parts[1] = parts[1].abs() * 50 + 1e4
    n = float(T * 7)
    gamma, beta = (torch.rand(C_, generator=g) + 0.5).cuda(), torch.randn(C_, generator=g).cuda()
    outs = []
    for route in ("fused", "reduce"):
        rm, rv = torch.zeros(C_, device="cuda"), torch.ones(C_, device="cuda")
        outs.append(_run_finalize(route, parts.flatten().cuda(), T, n, gamma, beta, rm, rv, 0.1, C_))
    assert torch.equal(outs[0], outs[1]), "finalize_partials and reduce_partials + finalize disagree"
    s = parts.double().sum(-1)
    e = T * R.U64 * parts.double().abs().sum(-1)
    mean, var, rstd, dmean, dvar, drstd = R.stats_bounds(s[0], s[1], e[0], e[1], n, EPS32)
    _report(f"finalize inexact T={T}", {"mean": _check(outs[0][2], mean, dmean, "mean"),
                                        "rstd": _check(outs[0][3], rstd, drstd, "rstd")})


@pytest.mark.parametrize("count", [2, 3])
@pytest.mark.parametrize("mom", [0.03, 0.1])
def test_finalize_running_update_small_counts(count, mom):
    """count 2 / 3: the unbiased factor is 2 / 1.5 - a biased running variance is far outside 1 ulp; also against
    torch.nn.BatchNorm1d's own update over the same samples."""
    g = torch.Generator().manual_seed(count)
    C_, T = 8, 3
    y = torch.randint(-8, 9, (C_, count), generator=g).double()
    parts = torch.zeros(2, C_, T, dtype=torch.float64)
    parts[0, :, 0], parts[1, :, 0] = y.sum(1), (y * y).sum(1)
    gamma, beta = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
    rm0, rv0 = torch.randn(C_, generator=g), torch.rand(C_, generator=g) + 0.5
    want = _finalize_expected(parts[0].sum(1), parts[1].sum(1), float(count), gamma, beta, rm0, rv0, mom)
    bn = torch.nn.BatchNorm1d(C_, eps=EPS, momentum=mom).double()
    with torch.no_grad():
        bn.running_mean.copy_(rm0); bn.running_var.copy_(rv0)
    bn(y.t())
    for route in ("fused", "reduce"):
        rm, rv = rm0.cuda(), rv0.cuda()
        _run_finalize(route, parts.flatten().float().cuda(), T, float(count), gamma.cuda(), beta.cuda(), rm, rv, mom, C_)
        _ulp_eq(rm, want[4], f"{route} running_mean")
        _ulp_eq(rv, want[5], f"{route} running_var")
        tol_m = 4 * (R.ulp32(bn.running_mean) + R.ulp32(rm0) + R.ulp32(mom * y.mean(1)))
        _check(rm, bn.running_mean, tol_m, f"{route} running_mean vs torch")
        _check(rv, bn.running_var, 4 * (R.ulp32(bn.running_var) + R.ulp32(rv0)), f"{route} running_var vs torch")


def test_finalize_edges_sentinels_constant_channel_and_nan():
    """update_running = 0 leaves the running buffers bit for bit; a constant channel whose fp32 square rounds down
    (var < 0 in fp64) clamps to var = 0, rstd = fp32(1/sqrt(eps)); a NaN partial poisons its own channel only."""
    C_, T, rows = 6, 65, 4
    g = torch.Generator().manual_seed(11)
    parts = _synthetic_slab(C_, T, rows, g)
    v = torch.tensor(0.3, dtype=torch.float32).double()
    assert R.f32(v * v) < v * v
    parts[0, 2], parts[1, 2] = rows * v, rows * R.f32(v * v)           # channel 2: every value is v
    slab = parts.float()
    slab[0, 4, 17] = NAN                                               # channel 4: one NaN partial
    gamma, beta = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
    n = float(T * rows)
    want = _finalize_expected(parts[0].sum(1), parts[1].sum(1), n, gamma, beta, torch.zeros(C_), torch.ones(C_), MOM)
    one_over = R.f32(torch.tensor(1.0 / math.sqrt(EPS32), dtype=torch.float64))
    ok = [c for c in range(C_) if c != 4]
    sent = torch.tensor([1.5, -2.25, 3.0e-30, 7.0, -0.0, 1e30], dtype=torch.float32)
    for route in ("fused", "reduce"):
        rm, rv = sent.clone().cuda(), (sent * 2).cuda()
        aff = _run_finalize(route, slab.flatten().cuda(), T, n, gamma.cuda(), beta.cuda(), rm, rv, MOM, C_, update=0)
        assert torch.equal(rm.cpu().view(torch.int32), sent.view(torch.int32)), route + ": update_running=0 wrote"
        assert torch.equal(rv.cpu().view(torch.int32), (sent * 2).view(torch.int32)), route + ": update_running=0 wrote"
        assert aff[3, 2].item() == one_over.item(), (route, "clamped rstd", aff[3, 2].item())
        assert aff[2, 2].item() == R.f32(v).item(), route
        assert torch.isnan(aff[:, 4]).all(), route + ": a NaN partial did not poison its channel"
        assert torch.equal(aff[2, ok].double(), want[0][ok]) and torch.equal(aff[3, ok].double(), want[1][ok]), route
        rm, rv = torch.zeros(C_, device="cuda"), torch.ones(C_, device="cuda")
        _run_finalize(route, slab.flatten().cuda(), T, n, gamma.cuda(), beta.cuda(), rm, rv, MOM, C_)
        assert torch.isnan(rm.cpu()[4]) and torch.isnan(rv.cpu()[4]), route
        _ulp_eq(rm.cpu()[ok], want[4][ok], route + " running_mean")
        _ulp_eq(rv.cpu()[ok], want[5][ok], route + " running_var")


# ---------------------------------------------------------------- b. backward coefficients on synthetic slabs
def _bwd_problem(M, C_, T, g, raw):
    """y [M, C] with mean offsets 0 / 8 / 64 x std, fp32 gamma, dz; partial slab [2][C][T] of row blocks (sum dz |
    sum dz*xhat with the fp32 mean / rstd, or sum dz*y when raw), rounded to fp32.  Everything fp64."""
    o = torch.tensor([0.0, 8.0, 64.0], dtype=torch.float64)[torch.arange(C_) % 3]
    std = torch.rand(C_, generator=g, dtype=torch.float64) + 0.5
    y = torch.randn(M, C_, generator=g, dtype=torch.float64) * std + o * std
    gamma = R.f32(torch.rand(C_, generator=g, dtype=torch.float64) + 0.5)
    dz = torch.randn(M, C_, generator=g, dtype=torch.float64) / M ** 0.5
    mean, var, _ = R.batch_stats(y)
    rstd = 1.0 / torch.sqrt(var + EPS)
    mean_f, rstd_f = R.f32(mean), R.f32(rstd)
    term1 = dz * y if raw else dz * (y - mean_f) * rstd_f
    slot = torch.arange(M) * T // M
    p = torch.zeros(2, C_, T, dtype=torch.float64)
    p[0].index_add_(1, slot, dz.t().contiguous())
    p[1].index_add_(1, slot, term1.t().contiguous())
    return dict(y=y, gamma=gamma, dz=dz, mean=mean, rstd=rstd, mean_f=mean_f, rstd_f=rstd_f, p=R.f32(p), M=M, C=C_,
                T=T, raw=raw)


def _coef_formula(s0, s1, n, g, mu, rs, raw):
    """The coefficient kernels' fp64 arithmetic on fp32 gamma / mean / rstd: (dgamma, dbeta, k1, k2, k3)."""
    if raw:
        s1 = rs * (s1 - mu * s0)
    S0, S1 = s0 / n, s1 / n
    return s1, s0, g * rs, -g * rs * rs * S1, -g * rs * S0 + g * rs * rs * mu * S1


def _dk_bounds(gm, mu, rs, muf, rsf, s0, s1, e0, e1, n):
    """|k_kernel - k_exact| from the kernel's inputs: the fp32 mean / rstd, sums within e0 / e1 of the exact ones,
    fp64 arithmetic, the rounding of k to fp32."""
    k1, k2, k3 = R.bwd_coeffs(s0, s1, n, gm, mu, rs)
    slack = 16 * R.U64 * gm * rs * (1 + (s0.abs() + rs * (mu.abs() + 1) * (s1.abs() + e1)) / n)
    dk1 = gm * (rsf - rs).abs() + R.ulp32(k1) / 2 + slack
    dk2 = gm * (rsf * rsf - rs * rs).abs() * s1.abs() / n + gm * rsf * rsf * e1 / n + R.ulp32(k2) / 2 + slack
    dk3 = (gm * (rsf - rs).abs() * s0.abs() / n + gm * rsf * e0 / n + gm * (rsf * rsf * muf - rs * rs * mu).abs() * s1.abs() / n
           + gm * rsf * rsf * muf.abs() * e1 / n + R.ulp32(k3) / 2 + slack)
    return (k1, k2, k3), (dk1, dk2, dk3)


def _rebuild_vs_autograd(P, coef, s0k, s1k, what):
    """dX = k1 dz + k2 y + k3 from the kernel's fp32 coefficients against fp64 autograd of BatchNorm2d; s0k / s1k: the
    sums the kernel worked from (their offsets from the exact sums enter the bound)."""
    y, dz, C_ = P["y"], P["dz"], P["C"]
    yr = y.t().reshape(1, C_, -1, 1).clone().requires_grad_(True)
    bn = torch.nn.BatchNorm2d(C_, eps=EPS).double()
    with torch.no_grad():
        bn.weight.copy_(P["gamma"])
    bn(yr).backward(dz.t().reshape(1, C_, -1, 1))
    want = yr.grad.reshape(C_, -1).t()
    xhat = (y - P["mean"]) * P["rstd"]
    s0, s1 = dz.sum(0), (dz * xhat).sum(0)
    _, (dk1, dk2, dk3) = _dk_bounds(P["gamma"], P["mean"], P["rstd"], P["mean_f"], P["rstd_f"], s0, s1,
                                    (s0k - s0).abs(), (s1k - s1).abs(), P["M"])
    k = coef.double().cpu().view(3, C_)
    got = k[0] * dz + k[1] * y + k[2]
    bound = dk1 * dz.abs() + dk2 * y.abs() + dk3 + 8 * R.U64 * (k[0].abs() * dz.abs() + k[1].abs() * y.abs() + k[2].abs())
    return _check(got, want, bound, what + " dX vs autograd")


def _device_job(P):
    C_ = P["C"]
    return dict(part=P["p"].flatten().float().cuda(), gamma=P["gamma"].float().cuda(), mean=P["mean_f"].float().cuda(),
                rstd=P["rstd_f"].float().cuda(), dgamma=_nan(C_), dbeta=_nan(C_), coef=_nan(3 * C_))


def _job_args(P, d):
    return (d["part"].data_ptr(), P["T"], float(P["M"]), d["gamma"].data_ptr(), d["mean"].data_ptr(), d["rstd"].data_ptr(),
            d["dgamma"].data_ptr(), d["dbeta"].data_ptr(), d["coef"].data_ptr(), P["C"], int(P["raw"]))


def _check_train_coeffs(P, d, what, worst, sums=None):
    """dgamma / dbeta / coefficients against the fp64 formula (<= 1 ulp), then dX rebuilt against autograd."""
    s0, s1 = sums if sums is not None else (P["p"][0].sum(1), P["p"][1].sum(1))
    dg, db, k1, k2, k3 = _coef_formula(s0, s1, float(P["M"]), P["gamma"], P["mean_f"], P["rstd_f"], P["raw"])
    got = [t.cpu() for t in (d["dgamma"], d["dbeta"], d["coef"])]
    worst["formula"] = max(worst.get("formula", 0), _ulp_eq(got[0], R.f32(dg), what + " dgamma"),
                           _ulp_eq(got[1], R.f32(db), what + " dbeta"),
                           _ulp_eq(got[2], R.f32(torch.cat([k1, k2, k3])), what + " coef"))
    worst["dX"] = max(worst.get("dX", 0), _rebuild_vs_autograd(P, got[2], s0, dg, what))


def _check_eval_coeffs(P, d, what, worst):
    """Eval-mode unit: dgamma / dbeta as in train mode, coefficients (gamma*rstd, 0, 0); dX = k1 dz against the
    eval-mode BatchNorm reference with mean / rstd standing for the running statistics."""
    s0, s1 = P["p"][0].sum(1), P["p"][1].sum(1)
    dg, db, _, _, _ = _coef_formula(s0, s1, float(P["M"]), P["gamma"], P["mean_f"], P["rstd_f"], P["raw"])
    got = [t.cpu() for t in (d["dgamma"], d["dbeta"], d["coef"])]
    worst["formula"] = max(worst.get("formula", 0), _ulp_eq(got[0], R.f32(dg), what + " dgamma"),
                           _ulp_eq(got[1], R.f32(db), what + " dbeta"))
    C_ = P["C"]
    k = got[2].double().view(3, C_)
    assert (k[1] == 0).all() and (k[2] == 0).all(), what + ": eval-mode k2 / k3 must be 0"
    rv = 1.0 / (P["rstd_f"] ** 2) - EPS                    # the running variance whose rstd is rstd_f
    dX, _, _ = R.bn_eval_backward(P["y"], P["dz"], P["mean_f"], rv, P["gamma"], torch.zeros(C_), EPS, R.IDENTITY)
    bound = (R.ulp32(P["gamma"] * P["rstd_f"]) / 2 + 16 * R.U64 * P["gamma"] * P["rstd_f"]) * P["dz"].abs()
    worst["dX"] = max(worst.get("dX", 0), _check(k[0] * P["dz"], dX, bound, what + " eval dX"))


@pytest.mark.parametrize("raw", [0, 1])
@pytest.mark.parametrize("C_,T", [(8, 5), (3, 257), (65, 1024), (16, 1500)])
def test_bwd_coeffs_partials_synthetic(raw, C_, T):
    g = torch.Generator().manual_seed(C_ * 7 + T + raw)
    P = _bwd_problem(4096, C_, T, g, raw)
    d = _device_job(P)
    _lib.check(_lib.lib().kodhip_bn_bwd_coeffs_partials(*_job_args(P, d), stream()), "bwd_coeffs_partials")
    torch.cuda.synchronize()
    worst = {}
    _check_train_coeffs(P, d, f"partials raw={raw} C={C_} T={T}", worst)
    _report(f"bwd_coeffs_partials raw={raw} C={C_} T={T}", worst)


@pytest.mark.parametrize("order", [0, 1])
def test_bwd_coeffs_partials2_two_units(order):
    """Two units of different (C, T, raw_moment) in one launch, the grid sized by the larger C - in both orders."""
    g = torch.Generator().manual_seed(5)
    Ps = [_bwd_problem(2048, 72, 33, g, 1), _bwd_problem(3000, 9, 700, g, 0)]
    if order:
        Ps = Ps[::-1]
    ds = [_device_job(P) for P in Ps]
    _lib.check(_lib.lib().kodhip_bn_bwd_coeffs_partials2(*_job_args(Ps[0], ds[0]), *_job_args(Ps[1], ds[1]), stream()),
               "partials2")
    torch.cuda.synchronize()
    worst = {}
    for i, (P, d) in enumerate(zip(Ps, ds)):
        _check_train_coeffs(P, d, f"partials2 job {i}", worst)
    _report(f"bwd_coeffs_partials2 order={order}", worst)


@pytest.mark.parametrize("raw", [0, 1])
def test_bwd_coeffs_eval_partials(raw):
    g = torch.Generator().manual_seed(21 + raw)
    P = _bwd_problem(2048, 24, 129, g, raw)
    d = _device_job(P)
    a = _job_args(P, d)
    _lib.check(_lib.lib().kodhip_bn_bwd_coeffs_eval_partials(a[0], a[1], *a[3:], stream()), "eval_partials")
    torch.cuda.synchronize()
    worst = {}
    _check_eval_coeffs(P, d, f"eval_partials raw={raw}", worst)
    _report(f"bwd_coeffs_eval_partials raw={raw}", worst)


@pytest.mark.parametrize("modes", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_bwd_coeffs_eval_partials2_modes(modes):
    """The two-unit launch with a mode per job (0 train, 1 eval)."""
    g = torch.Generator().manual_seed(31 + 2 * modes[0] + modes[1])
    Ps = [_bwd_problem(2048, 40, 17, g, 1), _bwd_problem(1024, 8, 1031, g, 0)]
    ds = [_device_job(P) for P in Ps]
    _lib.check(_lib.lib().kodhip_bn_bwd_coeffs_eval_partials2(*_job_args(Ps[0], ds[0]), modes[0], *_job_args(Ps[1], ds[1]),
                                                              modes[1], stream()), "eval_partials2")
    torch.cuda.synchronize()
    worst = {}
    for i, (P, d, ev) in enumerate(zip(Ps, ds, modes)):
        (_check_eval_coeffs if ev else _check_train_coeffs)(P, d, f"eval_partials2 {modes} job {i}", worst)
    _report(f"bwd_coeffs_eval_partials2 {modes}", worst)


@pytest.mark.parametrize("raw", [0, 1])
def test_bwd_coeffs_local_and_global_sums(raw):
    """kodhip_bn_bwd_coeffs (the all-reduce route): dgamma / dbeta from the LOCAL sums, the coefficients from the
    GLOBAL ones - the local sums here are those of the first half of the slots."""
    g = torch.Generator().manual_seed(41 + raw)
    P = _bwd_problem(4096, 16, 64, g, raw)
    glob, loc = P["p"].sum(-1), P["p"][:, :, :32].sum(-1)
    sl, sg = loc.flatten().cuda(), glob.flatten().cuda()
    d = _device_job(P)
    _lib.check(_lib.lib().kodhip_bn_bwd_coeffs(sl.data_ptr(), sg.data_ptr(), float(P["M"]), d["gamma"].data_ptr(),
                                               d["mean"].data_ptr(), d["rstd"].data_ptr(), d["dgamma"].data_ptr(),
                                               d["dbeta"].data_ptr(), d["coef"].data_ptr(), P["C"], raw, stream()), "bwd_coeffs")
    torch.cuda.synchronize()
    n = float(P["M"])
    ldg, ldb, _, _, _ = _coef_formula(loc[0], loc[1], n, P["gamma"], P["mean_f"], P["rstd_f"], raw)
    gdg, _, k1, k2, k3 = _coef_formula(glob[0], glob[1], n, P["gamma"], P["mean_f"], P["rstd_f"], raw)
    worst = {"formula": max(_ulp_eq(d["dgamma"], R.f32(ldg), "local dgamma"), _ulp_eq(d["dbeta"], R.f32(ldb), "local dbeta"),
                            _ulp_eq(d["coef"], R.f32(torch.cat([k1, k2, k3])), "global coef"))}
    worst["dX"] = _rebuild_vs_autograd(P, d["coef"], glob[0], gdg, "bwd_coeffs")
    _report(f"bwd_coeffs local/global raw={raw}", worst)


# ---------------------------------------------------------------- launch-plan mirror (conv_igemm.hip make_plan)
def _plan(M, N, K, row3):
    """(BM, BN, groups, tiles_m) of make_plan on the FAST path."""
    widest = 128 if N > 64 else (64 if N > 32 else 32)
    bm = 256 if (not row3 and widest >= 64 and M >= 256 * 64 and K >= 512) else 128
    best, best_cost = None, 1e30
    bn = widest
    while bn >= 32 and bn >= widest // 2:
        if not (bm == 256 and bn != widest):
            tiles_m, tiles_n = -(-M // bm), -(-N // bn)
            slots = 512 if bm == 256 else 1024
            if row3:
                slots = 512 if bn == 128 else (768 if bn == 64 else 1024)
            cost = -(-(tiles_m * tiles_n) // slots) * (bm + bn)
            if cost < best_cost * 0.97:
                best_cost = cost
                best = (bm, bn, min(tiles_m, min(max(slots // tiles_n, 8), 1024)), tiles_m)
        bn //= 2
    return best


def _tiles_per_group(tiles_m, groups):
    """Most tiles any group takes: groups sweep per-XCD bands (group q of an XCD: band begin + q, + gk, ...)."""
    worst = 0
    for xcd in range(8):
        gk = (groups - xcd + 7) >> 3
        if gk <= 0:
            continue
        gb = sum((groups - i + 7) >> 3 for i in range(xcd))
        b0, b1 = tiles_m * gb // groups, tiles_m * (gb + gk) // groups
        worst = max(worst, -(-(b1 - b0) // gk))
    return worst


def fwd_chain(M, N, Cin, k, s, stem=False):
    """Longest chain of fp32 roundings of a term of the forward conv epilogue's partial (module docstring)."""
    if stem and N <= 32:
        tiles = -(-M // 128)
        return _tiles_per_group(tiles, min(tiles, 768)) * 2 + 4 + 4
    row3 = k == 3 and s == 1 and not stem
    bm, bn, groups, tiles_m = _plan(M, N, 6 * 32 if stem else k * k * pad(Cin, 32), row3)
    threads = 512 if bm == 256 else 256
    return _tiles_per_group(tiles_m, groups) * bm * bn // (8 * threads) + int(math.log2(512 // bn)) + threads // 64


def _fwd_reference(y, chain, T, gamma, beta, rm0, rv0):
    """Exact statistics of the stored tensor y [M, C] (fp64 on the device) and the bounds of what the finalize
    writes from partials of chain length `chain` over T slots."""
    n, C_ = y.shape
    s0 = torch.zeros(C_, dtype=torch.float64, device=y.device)
    s1, a0 = s0.clone(), s0.clone()
    step = 1 << 22
    for i in range(0, n, step):
        yc = y[i:i + step].double()
        s0 += yc.sum(0); s1 += (yc * yc).sum(0); a0 += yc.abs().sum(0)
    e0 = (R.gamma_n(chain) + T * R.U64) * a0
    e1 = (R.gamma_n(chain + 1) + T * R.U64) * s1
    mean, _, _, dmean, dvar, drstd = R.stats_bounds(s0, s1, e0, e1, n, EPS32)
    m2 = torch.zeros_like(s0)                               # two-pass variance for the reference values
    for i in range(0, n, step):
        m2 += ((y[i:i + step].double() - mean) ** 2).sum(0)
    var = m2 / n
    rstd = 1.0 / torch.sqrt(var + EPS32)
    dev = y.device
    sc, sh, dsc, dsh = R.affine_bounds(mean, rstd, dmean, drstd, gamma.double().to(dev), beta.double().to(dev))
    rm, rv, drm, drv = R.running_bounds(rm0.to(dev), rv0.to(dev), mean, var, n, MOM, dmean, dvar)
    return dict(mean=mean, rstd=rstd, scale=sc, shift=sh, rm=rm, rv=rv, dmean=dmean, drstd=drstd, dscale=dsc,
                dshift=dsh, drm=drm, drv=drv)


def _check_fwd_constants(ref, aff, rm, rv, what, worst):
    C_ = ref["mean"].numel()
    a = aff.view(4, C_)
    for key, got, bnd in (("mean", a[2], "dmean"), ("rstd", a[3], "drstd"), ("scale", a[0], "dscale"),
                          ("shift", a[1], "dshift"), ("rm", rm, "drm"), ("rv", rv, "drv")):
        worst[key] = max(worst.get(key, 0), _check(got, ref[key], ref[bnd], f"{what} {key}"))


# ---------------------------------------------------------------- c. forward chain
FWD_CASES = [
    # B, Cin, H, W, N, k, s
    (2, 32, 40, 40, 64, 1, 1),          # 128-row tiles, one tile per group
    (4, 64, 128, 128, 128, 3, 2),       # 256-row tiles: 64 groups in 128 slots (the rest zeroed)
    (2, 32, 300, 300, 32, 1, 1),        # M = 180000 > 128 * 1024: several tiles per slot
    (2, 64, 128, 128, 1024, 1, 1),      # N wide: 128 groups in 256 slots
    (2, 32, 48, 40, 96, 3, 1),          # 3x3 stride 1 (ROW3 form)
]


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_chain_vs_fp64_bn(case):
    """kodhip_conv_fwd_raw (stats slab pre-filled with NaN) -> kodhip_bn_finalize_partials -> bn_silu_apply /
    bn_act_apply (every activation, with a residual), channels with |mean|/std in {0, 8, 64} (a constant input channel),
    against fp64 BatchNorm of the stored tensor."""
    B, Cin, H, W, N, k, s = case
    lib = _lib.lib()
    g = torch.Generator().manual_seed(sum(case))
    p = k // 2
    x = torch.randn(B, Cin, H, W, generator=g)
    x[:, 0] = 1.0
    w = torch.randn(N, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    w[:, 0] = 0.0
    w[:, 0, p, p] = torch.tensor([0.0, 8.0, 64.0])[torch.arange(N) % 3]
    pk = pack([bf(w)])
    yb, stats = conv_fwd_raw(nhwc(x), (0, Cin), pk, s, p)
    T = stats.shape[-1]
    assert torch.isfinite(stats).all(), "a statistics slot was left unwritten"
    M = yb.numel() // N
    y = yb.view(M, N)
    gamma, beta = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    rm0, rv0 = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5
    rm, rv, gm, bt = rm0.cuda(), rv0.cuda(), gamma.cuda(), beta.cuda()
    aff = _nan(4 * N)
    a = aff.data_ptr()
    _lib.check(lib.kodhip_bn_finalize_partials(stats.data_ptr(), T, float(M), gm.data_ptr(), bt.data_ptr(), rm.data_ptr(),
                                               rv.data_ptr(), MOM, EPS, a, a + 4 * N, a + 8 * N, a + 12 * N, N, 1, stream()),
               "finalize_partials")
    chain = fwd_chain(M, N, Cin, k, s)
    ref = _fwd_reference(y, chain, T, gamma, beta, rm0, rv0)
    worst = {}
    _check_fwd_constants(ref, aff, rm, rv, f"{case}", worst)
    res = nhwc(torch.randn(1, N, M, 1, generator=g)).view(M, N)
    yd = y.double()
    zk = yd * aff[:N].double() + aff[N:2 * N].double()
    dz = yd.abs() * ref["dscale"] + ref["dshift"] + R.ulp32(zk)          # |z_kernel - z| (fp32 constants, the fma)
    z = yd * ref["scale"] + ref["shift"]
    for kind, slope in ACTS:
        out = _nan(M, N, dtype=torch.bfloat16)
        _lib.check(lib.kodhip_bn_act_apply(yb.data_ptr(), N, a, a + 4 * N, res.data_ptr(), N, 0, out.data_ptr(), N, 0, M, N,
                                           kind, slope, stream()), "apply")
        want = R.act(kind, z, slope) + res.double()
        pre = R.act_lipschitz(kind, slope) * dz + R.relerr_bound(kind, zk)
        pre = pre + R.ulp32(want.abs() + pre)                                # the residual add's rounding
        worst[f"apply{kind}"] = _check(out, want, pre + R.ulpbf16(want.abs() + pre) / 2, f"{case} apply act={kind}")
    _report(f"forward chain {case} chain={chain} T={T}", worst)


# ---------------------------------------------------------------- d. backward chain
def _bwd_reduce_chain(M, C_, T2):
    """bn_*_bwd_reduce: rows per thread + the block's row lanes (geo() of bn_act.hip)."""
    rpb = max(256 // (C_ // 8), 1)
    q = 1
    while (q * C_ * 2) % 128:
        q *= 2
    if rpb >= q:
        rpb -= rpb % q
    rpb = max(rpb, 1)
    return -(-M // (T2 * rpb)) + rpb


def _fused_chain(M, groups):
    return 12 + 8 * (-(-(-(-M // 128)) // groups) + 1)


def _bwd_reference(y, dA, aff, gamma, kind, slope):
    """fp64 gradients of act(BN_train(y)) (beta = 0) for the stored y.  Where the exact z and the kernel's z lie on the
    two sides of a kink the activation's derivative is taken on the kernel's side."""
    C_ = y.shape[1]
    a = aff.double().view(4, C_)
    zk = R.f32(y * a[0] + a[1])
    mean, var, _ = R.batch_stats(y)
    rstd = 1.0 / torch.sqrt(var + EPS32)
    z = (y - mean) * rstd * gamma
    side = z
    for kink in {R.RELU: (0.0,), R.LEAKY: (0.0,), R.HARDSWISH: (-3.0, 3.0)}.get(kind, ()):
        side = torch.where(((z - kink).sign() != (zk - kink).sign()) | (zk == kink), zk, side)
    dX, s1, s0, dz = R.bn_act_backward(y, dA, gamma, torch.zeros_like(gamma), EPS32, kind, slope, z_side=side)
    return dict(dX=dX, dz=dz, zk=zk, mean=mean, rstd=rstd, s0=s0, s1=s1)


def _bwd_bounds(ref, y, dA, aff, gamma, chain, T2, raw, kind):
    """Bounds on dgamma, dbeta and dY (bf16) of the kernel chain against the fp64 reference."""
    C_ = y.shape[1]
    a = aff.double().view(4, C_)
    n = y.shape[0]
    mu, rs, muf, rsf = ref["mean"], ref["rstd"], a[2], a[3]
    dz, zk = ref["dz"], ref["zk"]
    # |dz_kernel - dz|: the pre-activation's offset (fp32 constants, the fma) and the kernels' own roundings
    dzz = y.abs() * (a[0] - gamma * rs).abs() + (a[1] + mu * gamma * rs).abs() + R.ulp32(zk)
    if kind == R.SILU:
        sg = torch.sigmoid(zk)
        edz = dA.abs() * (0.5 * dzz + R.sigmoid_rel_err(zk) * sg * (1 + 2 * zk.abs()) + 4 * R.U32 * sg * (1 + zk.abs()))
    elif kind == R.HARDSWISH:
        edz = dA.abs() * (dzz / 3 + 2 * R.U32 * (zk.abs() / 3 + 0.5)) + R.U32 * dz.abs()
    else:
        edz = R.U32 * dz.abs()
    w1 = y if raw else (y - muf) * rsf                     # what dz multiplies in the second partial
    t1 = dz * w1
    e0 = edz.sum(0) + (R.gamma_n(chain) + T2 * R.U64) * (dz.abs() + edz).sum(0)
    e1 = (edz * w1.abs()).sum(0) + (R.gamma_n(chain + 3) + T2 * R.U64) * (t1.abs() + edz * w1.abs()).sum(0)
    s1k = rsf * (t1.sum(0) - muf * dz.sum(0)) if raw else t1.sum(0)
    if raw:
        e1 = rsf * (e1 + muf.abs() * e0) + 8 * R.U64 * rsf * (t1.abs().sum(0) + muf.abs() * dz.abs().sum(0))
    e1 = e1 + (s1k - ref["s1"]).abs()
    (k1, k2, k3), (dk1, dk2, dk3) = _dk_bounds(gamma, mu, rs, muf, rsf, ref["s0"], ref["s1"], e0, e1, n)
    inner = (k2 * y + k3).abs() + dk2 * y.abs() + dk3
    pre = dk1 * dz.abs() + (k1 + dk1) * edz + dk2 * y.abs() + dk3
    pre = pre + R.ulp32(inner) + R.ulp32(ref["dX"].abs() + pre)
    return dict(dgamma=e1 + R.ulp32(ref["s1"].abs() + e1), dbeta=e0 + R.ulp32(ref["s0"].abs() + e0),
                dX=pre + R.ulpbf16(ref["dX"].abs() + pre) / 2)


def _bwd_finish(y_raw, dA_buf, lda, dacoff, aff, gamma, part, T2, raw, kind, slope, chain, what):
    """Coefficients from the slab, the apply pass, and the checks against fp64 gradients of act(BN_train(y)) + res."""
    lib = _lib.lib()
    M, C_ = y_raw.shape
    assert torch.isfinite(part).all(), what + ": a partial slot was left unwritten"
    gm = gamma.float().cuda()
    dg, db, coef = _nan(C_), _nan(C_), _nan(3 * C_)
    a = aff.data_ptr()
    _lib.check(lib.kodhip_bn_bwd_coeffs_partials(part.data_ptr(), T2, float(M), gm.data_ptr(), a + 8 * C_, a + 12 * C_,
                                                 dg.data_ptr(), db.data_ptr(), coef.data_ptr(), C_, raw, stream()), "coeffs")
    dA16 = dA_buf.view(M, lda)[:, dacoff:dacoff + C_]
    dA, y = dA16.double(), y_raw.double()
    gd = gamma.double().to(y.device)
    ref = _bwd_reference(y, dA, aff, gd, kind, slope)
    bnd = _bwd_bounds(ref, y, dA, aff, gd, chain, T2, raw, kind)
    ybuf = y_raw.clone()
    di = _nan(M, C_, dtype=torch.bfloat16)
    _lib.check(lib.kodhip_bn_act_bwd_apply(dA_buf.data_ptr(), lda, dacoff, ybuf.data_ptr(), C_, a, a + 4 * C_, coef.data_ptr(),
                                           di.data_ptr(), C_, 0, 0, M, C_, kind, slope, stream()), "bwd apply")
    worst = {"dgamma": _check(dg, ref["s1"], bnd["dgamma"], what + " dgamma"),
             "dbeta": _check(db, ref["s0"], bnd["dbeta"], what + " dbeta"),
             "dY": _check(ybuf, ref["dX"], bnd["dX"], what + " dY")}
    assert torch.equal(di, dA16), what + ": residual gradient"
    return worst


def _aff_for(y, gamma):
    """fp32 (scale, shift, mean, rstd) of the exact batch statistics of y (beta = 0), as a forward pass leaves them."""
    mean, var, _ = R.batch_stats(y.double())
    rstd = 1.0 / torch.sqrt(var + EPS32)
    g = gamma.double().to(y.device)
    return torch.cat([g * rstd, -mean * g * rstd, mean, rstd]).float().cuda()


def _offset_raw(M, C_, g):
    o = torch.tensor([0.0, 8.0, 64.0])[torch.arange(C_) % 3]
    return (torch.randn(M, C_, generator=g) + o).to(torch.bfloat16).cuda()


@pytest.mark.parametrize("kind,slope", ACTS)
def test_backward_chain_separate_reduce(kind, slope):
    """bn_{silu,act}_bwd_reduce (slab pre-filled with NaN) -> _bwd_coeffs_partials -> bn_{silu,act}_bwd_apply."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(50 + kind)
    M, C_ = 37 * 29 * 3, 48
    y = _offset_raw(M, C_, g)
    gamma = R.f32(torch.rand(C_, generator=g, dtype=torch.float64) + 0.5)
    aff = _aff_for(y, gamma)
    ld = C_ + 16
    dA = torch.zeros(M, ld, dtype=torch.bfloat16, device="cuda")
    dA[:, 8:8 + C_] = (torch.randn(M, C_, generator=g) * 100 / M ** 0.5).to(torch.bfloat16).cuda()
    T2 = lib.kodhip_bn_bwd_slots(M, C_)
    part = _nan(2 * C_ * T2)
    a = aff.data_ptr()
    _lib.check(lib.kodhip_bn_act_bwd_reduce(dA.data_ptr(), ld, 8, y.data_ptr(), C_, a, a + 4 * C_, a + 8 * C_, a + 12 * C_,
                                            part.data_ptr(), M, C_, kind, slope, stream()), "bwd reduce")
    worst = _bwd_finish(y, dA, ld, 8, aff, gamma, part, T2, 0, kind, slope, _bwd_reduce_chain(M, C_, T2), f"reduce act={kind}")
    _report(f"backward separate reduce act={kind}", worst)


BNRED_CASES = [
    # B, Cin (dX channels), H, W, Cout, k, s, stride-2 form
    (2, 64, 24, 20, 64, 3, 1, None),
    (3, 96, 40, 30, 64, 1, 1, None),
    (2, 64, 32, 24, 128, 3, 2, "classes"),
    (2, 64, 32, 24, 128, 3, 2, "fold"),
    (4, 128, 72, 64, 128, 3, 1, None),      # 256-pixel tiles
]


@pytest.mark.parametrize("case", BNRED_CASES)
def test_backward_chain_fused_dgrad_epilogue(case):
    """conv_dgrad_bnred / _s2_bnred / _s2f_bnred (segment slab pre-filled with NaN; sum dz, sum dz*y) ->
    _bwd_coeffs_partials(raw_moment = 1) -> bn_silu_bwd_apply, against fp64 gradients of SiLU(BN_train(y))."""
    from object_detection_cib_amd._lib import KodBnRedSeg
    lib = _lib.lib()
    B, Cin, H, W, Cout, k, s, form = case
    g = torch.Generator().manual_seed(sum(case[:7]))
    p = k // 2
    w = bf(torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = torch.randn(B, Ho, Wo, Cout, generator=g).to(torch.bfloat16).cuda()
    M = B * H * W
    pk = pack([w], s2=("fold" if form == "fold" else bool(form)))
    if form == "fold":
        slots = lib.kodhip_conv_dgrad_s2f_bnred_slots(B, H, W, Cin, Cout, Cout)
    else:
        slots = lib.kodhip_conv_dgrad_bnred_slots(B, H, W, Cin, Cout, k, k, s, s, p, p, Cout, int(bool(form)))
    assert slots > 0
    y = _offset_raw(M, Cin, g)
    gamma = R.f32(torch.rand(Cin, generator=g, dtype=torch.float64) + 0.5)
    aff = _aff_for(y, gamma)
    part = _nan(2 * Cin * slots)
    segs = (KodBnRedSeg * 1)()
    segs[0].ch_begin, segs[0].ch_count, segs[0].raw, segs[0].ldr = 0, Cin, y.data_ptr(), Cin
    segs[0].aff, segs[0].partials = aff.data_ptr(), part.data_ptr()
    sp = C.cast(segs, C.c_void_p)
    dx = _nan(B, H, W, Cin, dtype=torch.bfloat16)
    if form:
        fn = lib.kodhip_conv_dgrad_s2f_bnred if form == "fold" else lib.kodhip_conv_dgrad_s2_bnred
        _lib.check(fn(dy.data_ptr(), pk["d"].data_ptr(), dx.data_ptr(), B, H, W, Cin, 0, Cin, Cout, Cout, 0, 0, None, sp, 1,
                      slots, stream()), "dgrad_s2_bnred")
        groups = slots // 4
    else:
        _lib.check(lib.kodhip_conv_dgrad_bnred(dy.data_ptr(), pk["d"].data_ptr(), dx.data_ptr(), B, H, W, Cin, 0, Cin, Cout, k, k,
                                               s, s, p, p, pk["Kdp"], Cout, 0, 0, None, sp, 1, slots, stream()), "dgrad_bnred")
        groups = slots
    worst = _bwd_finish(y, dx.view(M, Cin), Cin, 0, aff, gamma, part, slots, 1, R.SILU, 0.0, _fused_chain(M, groups),
                        f"fused {case}")
    _report(f"backward fused {case}", worst)


def test_backward_chain_dual_source_epilogue():
    """conv_dgrad_dual_bnred: two pointwise sources into one dX, the fused reduction into two segments."""
    from object_detection_cib_amd._lib import KodBnRedSeg
    lib = _lib.lib()
    B, Cin, H, W, N = 3, 128, 20, 12, 64
    g = torch.Generator().manual_seed(77)
    M = B * H * W
    pks = [pack([bf(torch.randn(N, Cin, 1, 1, generator=g) / Cin ** 0.5)]) for _ in range(2)]
    dys = [torch.randn(B, H, W, N, generator=g).to(torch.bfloat16).cuda() for _ in range(2)]
    slots = lib.kodhip_conv_dgrad_dual_bnred_slots(B, H, W, Cin, N, N)
    assert slots > 0
    prods = []
    segs = (KodBnRedSeg * 2)()
    for i, c0 in enumerate((0, 64)):
        c = 64
        y = _offset_raw(M, c, g)
        gamma = R.f32(torch.rand(c, generator=g, dtype=torch.float64) + 0.5)
        aff = _aff_for(y, gamma)
        part = _nan(2 * c * slots)
        segs[i].ch_begin, segs[i].ch_count, segs[i].raw, segs[i].ldr = c0, c, y.data_ptr(), c
        segs[i].aff, segs[i].partials = aff.data_ptr(), part.data_ptr()
        prods.append((c0, y, gamma, aff, part))
    dx = _nan(B, H, W, Cin, dtype=torch.bfloat16)
    _lib.check(lib.kodhip_conv_dgrad_dual_bnred(dys[0].data_ptr(), pks[0]["d"].data_ptr(), dys[1].data_ptr(), pks[1]["d"].data_ptr(),
                                                dx.data_ptr(), B, H, W, Cin, 0, Cin, N, pks[0]["Kdp"], N, 0, 0, None,
                                                C.cast(segs, C.c_void_p), 2, slots, stream()), "dual_bnred")
    worst = {}
    for c0, y, gamma, aff, part in prods:
        w = _bwd_finish(y, dx.view(M, Cin), Cin, c0, aff, gamma, part, slots, 1, R.SILU, 0.0, _fused_chain(M, slots),
                        f"dual segment {c0}")
        worst.update({f"{k}@{c0}": v for k, v in w.items()})
    _report("backward fused dual", worst)


# ---------------------------------------------------------------- e. in situ, at the engine's own geometry
@pytest.mark.parametrize("B", [16, 64])
def test_in_situ_statistics_every_unit(B):
    """yv5s train-mode forward_raw at B x 640 px (B = 64: the bench geometry), the statistics slabs NaN-filled before the
    first batch, then a second, different batch (stale slots): every unit's mean, rstd, scale, shift and running
    statistics against fp64 statistics of its stored pre-BN tensor, within the error model's bound."""
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    size = 640
    torch.manual_seed(0)
    net = Yolov5Network(3, 10, widen_factor=0.5, deepen_factor=0.33).cuda().train()
    eng = net.engine()
    xs = [torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(s)).cuda() for s in (1, 2)]
    with torch.no_grad():
        net.forward_raw(xs[0])                      # allocates the engine's buffers at this geometry
    worst, where = {}, {}
    for it, x in enumerate(xs):
        if it == 0:
            for u in eng.exec_units:
                eng.cur.units[u.name].stats.fill_(NAN)
        rm0, rv0 = eng.rm_arena.clone(), eng.rv_arena.clone()
        with torch.no_grad():
            net.forward_raw(x)
        torch.cuda.synchronize()
        for u in eng.exec_units:
            st, C_ = eng.cur.units[u.name], u.cout
            chain = fwd_chain(st.M, C_, u.cin, u.k, u.s, stem=u.stem)
            o = st.lay.rs_off
            ref = _fwd_reference(st.raw.view(-1, C_), chain, st.T, eng.p_arena[st.lay.g_off:st.lay.g_off + C_],
                                 eng.p_arena[st.lay.b_off:st.lay.b_off + C_], rm0[o:o + C_], rv0[o:o + C_])
            w = {}
            _check_fwd_constants(ref, st.aff, eng.rm_arena[o:o + C_], eng.rv_arena[o:o + C_], f"B={B} batch {it} {u.name}", w)
            for key, v in w.items():
                if v > worst.get(key, -1):
                    worst[key], where[key] = v, f"{u.name} (M={st.M}, T={st.T}, chain={chain})"
    _report(f"in situ B={B}/640", worst)
    key = max(worst, key=worst.get)
    print(f"[bn-stats] in situ B={B}/640 worst unit: {where[key]} {key} err/bound {worst[key]:.3g}")
