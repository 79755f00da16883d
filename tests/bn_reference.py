"""Plain float64 reference of train-mode / eval-mode BatchNorm2d followed by an activation (and a residual add), and
the rounding-error model that the BatchNorm statistics tests (tests/test_hip_bn_stats.py) take their tolerances from.

Tensors are channels-last rows: y is [M, C] (M = batch x height x width), every per-channel vector is [C].  Everything
here is float64 torch on whatever device the inputs live on; tests/test_bn_reference.py pins it to
torch.nn.BatchNorm2d and autograd in float64, so the GPU tests compare the kernels with torch's semantics, not with a
transcription of the kernel sources.

Error model (fp32 unit roundoff u = 2^-24).  A sum formed by fp32 additions in which every term passes through at most
c roundings has |computed - exact| <= gamma(c) * sum |terms|, gamma(c) = c u / (1 - c u) (Higham, Accuracy and
Stability of Numerical Algorithms, 2nd ed., sec. 4.2); a product rounded once more adds one to c for its terms.
`stats_bounds` carries such bounds on the two per-channel sums (sum y, sum y^2) through mean = s0 / n,
var = s1 / n - mean^2 and rstd = 1 / sqrt(var + eps) by interval arithmetic, plus the final rounding to fp32.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24          # unit roundoff of fp32
U64 = 2.0 ** -53          # ... of fp64

# activation codes of the kodhip_bn_act_* entry points
SILU, RELU, LEAKY, HARDSWISH, IDENTITY = 0, 1, 2, 3, 4


# ---------------------------------------------------------------- forward statistics
def batch_stats(y: torch.Tensor):
    """y [M, C] -> (mean, biased variance, unbiased variance), fp64, two-pass."""
    y = y.double()
    n = y.shape[0]
    mean = y.mean(0)
    var = ((y - mean) ** 2).sum(0) / n
    return mean, var, var * n / (n - 1) if n > 1 else var


def affine(mean, var, gamma, beta, eps):
    """BatchNorm's per-channel constants: rstd = 1/sqrt(var + eps), scale = gamma*rstd, shift = beta - mean*scale."""
    rstd = 1.0 / torch.sqrt(var.double() + eps)
    scale = gamma.double() * rstd
    return rstd, scale, beta.double() - mean.double() * scale


def running_update(running_mean, running_var, mean, var_unbiased, momentum):
    """torch's update: r <- (1 - momentum) r + momentum * batch value (the variance unbiased)."""
    m = float(momentum)
    return ((1 - m) * running_mean.double() + m * mean.double(),
            (1 - m) * running_var.double() + m * var_unbiased.double())


# ---------------------------------------------------------------- activations (torch conventions at the kinks)
def act(kind: int, z: torch.Tensor, slope: float = 0.0) -> torch.Tensor:
    if kind == SILU:
        return F.silu(z)
    if kind == RELU:
        return F.relu(z)
    if kind == LEAKY:
        return F.leaky_relu(z, slope)
    if kind == HARDSWISH:
        return F.hardswish(z)
    return z


def act_grad(kind: int, z: torch.Tensor, slope: float = 0.0) -> torch.Tensor:
    """d act / dz: relu'(0) = 0, leaky uses z > 0, hardswish' = 0 up to -3, z/3 + 1/2 inside (-3, 3), 1 from 3 on."""
    if kind == SILU:
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    if kind == RELU:
        return (z > 0).to(z.dtype)
    if kind == LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    if kind == HARDSWISH:
        return torch.where(z <= -3, torch.zeros_like(z), torch.where(z < 3, z / 3 + 0.5, torch.ones_like(z)))
    return torch.ones_like(z)


def act_lipschitz(kind: int, slope: float = 0.0) -> float:
    """max |act'|: bounds how far an error in the pre-activation moves the output."""
    return {SILU: 1.0999, RELU: 1.0, LEAKY: max(1.0, abs(slope)), HARDSWISH: 1.5, IDENTITY: 1.0}[kind]


# ---------------------------------------------------------------- train-mode BatchNorm + activation
def bn_act_forward(y, gamma, beta, eps, kind=SILU, slope=0.0, residual=None):
    """act(BN_train(y)) (+ residual) with the batch statistics; returns (out, z, mean, var_biased, rstd)."""
    y = y.double()
    mean, var, _ = batch_stats(y)
    rstd, scale, shift = affine(mean, var, gamma, beta, eps)
    z = (y - mean) * rstd * gamma.double() + beta.double()
    out = act(kind, z, slope)
    if residual is not None:
        out = out + residual.double()
    return out, z, mean, var, rstd


def bwd_coeffs(s0, s1, count, gamma, mean, rstd):
    """From s0 = sum dz and s1 = sum dz*xhat: (k1, k2, k3) of dX = k1*dz + k2*y + k3, dgamma = s1, dbeta = s0."""
    g, rs, mu = gamma.double(), rstd.double(), mean.double()
    S0, S1 = s0.double() / count, s1.double() / count
    return g * rs, -g * rs * rs * S1, -g * rs * S0 + g * rs * rs * mu * S1


def bn_act_backward(y, dout, gamma, beta, eps, kind=SILU, slope=0.0, z_side=None):
    """Closed-form gradients of act(BN_train(y)) (+ residual): (dX, dgamma, dbeta, dz) with dz = dout * act'(z),
    dbeta = sum dz, dgamma = sum dz*xhat.  (The residual's own gradient is dout.)  z_side: where given, act' is taken
    at these pre-activations instead (the side of a kink that a rounded z fell on)."""
    y, dout = y.double(), dout.double()
    n = y.shape[0]
    mean, var, _ = batch_stats(y)
    rstd, _, _ = affine(mean, var, gamma, beta, eps)
    xhat = (y - mean) * rstd
    z = xhat * gamma.double() + beta.double()
    dz = dout * act_grad(kind, z if z_side is None else z_side, slope)
    s0, s1 = dz.sum(0), (dz * xhat).sum(0)
    k1, k2, k3 = bwd_coeffs(s0, s1, n, gamma, mean, rstd)
    return k1 * dz + k2 * y + k3, s1, s0, dz


# ---------------------------------------------------------------- eval-mode BatchNorm
def bn_eval_forward(y, running_mean, running_var, gamma, beta, eps, kind=SILU, slope=0.0):
    rstd, scale, shift = affine(running_mean, running_var, gamma, beta, eps)
    return act(kind, y.double() * scale + shift, slope)


def bn_eval_backward(y, dout, running_mean, running_var, gamma, beta, eps, kind=SILU, slope=0.0):
    """(dX, dgamma, dbeta) of act(BN_eval(y)): no terms through the batch moments, dX = gamma*rstd*dz."""
    rstd, scale, shift = affine(running_mean, running_var, gamma, beta, eps)
    y = y.double()
    dz = dout.double() * act_grad(kind, y * scale + shift, slope)
    xhat = (y - running_mean.double()) * rstd
    return dz * gamma.double() * rstd, (dz * xhat).sum(0), dz.sum(0)


# ---------------------------------------------------------------- error model
def gamma_n(c: float, u: float = U32) -> float:
    """gamma(c) = c u / (1 - c u): relative bound of c chained roundings."""
    assert c * u < 0.5, c
    return c * u / (1 - c * u)


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """Spacing of fp32 numbers at |x| (subnormal floor 2^-149)."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def ulpbf16(x: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 numbers at |x|."""
    a = x.double().abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def f32(x) -> torch.Tensor:
    """Round to fp32 (kept as fp64)."""
    return torch.as_tensor(x, dtype=torch.float64).float().double()


def stats_bounds(s0, s1, e0, e1, n, eps):
    """Exact per-channel sums s0 = sum y, s1 = sum y^2 (fp64) and bounds e0, e1 on the kernel's error in them ->
    (mean, var, rstd) of the exact data and the bounds (dmean, dvar, drstd) on the fp32 results of the finalize
    (fp64 arithmetic from the sums; the interval of var is pushed through rstd, then the rounding to fp32 added)."""
    s0, s1, e0, e1 = s0.double(), s1.double(), e0.double(), e1.double()
    mean = s0 / n
    var = (s1 / n - mean * mean).clamp_min(0.0)
    dmean = e0 / n
    dvar = e1 / n + (2 * mean.abs() + dmean) * dmean
    # fp64 rounding of the finalize itself (a few operations on values of size s1 / n)
    dvar = dvar + 8 * U64 * (s1.abs() / n + mean * mean)
    rstd = 1.0 / torch.sqrt(var + eps)
    lo = 1.0 / torch.sqrt((var + dvar) + eps)
    hi = 1.0 / torch.sqrt((var - dvar).clamp_min(0.0) + eps)
    drstd = torch.maximum(rstd - lo, hi - rstd) + ulp32(rstd) / 2
    return mean, var, rstd, dmean + ulp32(mean) / 2, dvar, drstd


def affine_bounds(mean, rstd, dmean, drstd, gamma, beta):
    """fp32 scale = gamma*rstd_f, shift = beta - mean_f*scale from rstd_f, mean_f within (drstd, dmean) of the exact
    values -> bounds on scale and shift (each product / difference rounded once)."""
    g = gamma.double()
    scale = g * rstd
    shift = beta.double() - mean * scale
    dscale = g.abs() * drstd + ulp32(scale)
    dshift = (mean.abs() + dmean) * dscale + scale.abs() * dmean + ulp32(mean * scale) + ulp32(shift)
    return scale, shift, dscale, dshift


def running_bounds(rm0, rv0, mean, var, n, momentum, dmean, dvar):
    """Exact running update from the exact batch statistics and bounds on the kernel's fp32 result
    ((1 - m) r and m x each rounded, their sum rounded; the batch values within dmean / dvar)."""
    m = float(momentum)
    unb = var * n / (n - 1) if n > 1 else var
    rm, rv = running_update(rm0, rv0, mean, unb, m)
    drm = m * dmean + ulp32((1 - m) * rm0.double()) + ulp32(m * mean) + ulp32(rm)
    dunb = (dvar * n / (n - 1) if n > 1 else dvar) + ulp32(unb)
    drv = m * dunb + ulp32((1 - m) * rv0.double()) + ulp32(m * unb) + ulp32(rv)
    return rm, rv, drm, drv


def sigmoid_rel_err(z: torch.Tensor) -> torch.Tensor:
    """Relative error bound of the kernels' sigmoid, rcp(1 + exp2(-log2(e) z)) with hardware exp2 / rcp (1 ulp each):
    the fp32 argument (|z| log2(e) rounded twice) moves exp by |z| 2u relatively, exp2 / rcp / the add add 5u."""
    s = torch.sigmoid(z.double())
    return 5 * U32 + (1 - s) * (2 * U32 * z.double().abs() + 4 * U32)


def relerr_bound(kind: int, z: torch.Tensor) -> torch.Tensor:
    """Bound on |fp32 act(z) - act(z)| of the kernels' activations (SiLU: z * sigmoid with the error above)."""
    if kind == SILU:
        return (sigmoid_rel_err(z) + U32) * torch.sigmoid(z.double()) * z.double().abs()
    return (4 if kind == HARDSWISH else 1) * U32 * z.double().abs()     # z*clamp(z+3)/6: three roundings; leaky: z*slope


# ---------------------------------------------------------------- fp32 restatement of the elementwise kernels (acts 1 - 4)
# ReLU, LeakyReLU, Hardswish and identity use only IEEE operations (the library is built without fast-math and without
# contraction), so the apply and backward-apply passes can be restated operation by operation in fp32 and compared
# bit for bit (tests/test_hip_bn_act_exact.py).  SiLU (hardware exp2 / rcp) is not restated.
def _round_fraction_f32(v) -> float:
    """Exact rational -> nearest fp32, ties to even."""
    import numpy as np
    f = np.float32(float(v))
    from fractions import Fraction
    best = None
    for c in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        d = abs(Fraction(float(c)) - v)
        even = (int(np.float32(c).view(np.int32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, float(c), even)
    return best[1]


FMA_SLOW = [0]            # elements that took the exact path (tests report it)


def fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fmaf(a, b, c) on fp32 tensors: one rounding.  a*b is exact in fp64 (48-bit product); where the fp64 sum with c is
    exact too (TwoSum residual zero) its rounding to fp32 is the fma's.  Every other element is recomputed exactly with
    fractions.Fraction - no element is left out."""
    from fractions import Fraction
    a, b, c = torch.broadcast_tensors(a.float(), b.float(), c.float())
    p, cd = a.double() * b.double(), c.double()
    s = p + cd
    bb = s - p
    resid = (p - (s - bb)) + (cd - bb)
    out = s.float()
    idx = (resid != 0).nonzero(as_tuple=False)
    if idx.numel():
        out = out.clone()
        FMA_SLOW[0] += idx.shape[0]
        for i in idx.tolist():
            i = tuple(i)
            v = Fraction(a[i].item()) * Fraction(b[i].item()) + Fraction(c[i].item())
            out[i] = _round_fraction_f32(v)
    return out


def act32(kind: int, z: torch.Tensor, slope: float = 0.0) -> torch.Tensor:
    """kod_act<> in fp32, in the kernel's operation order."""
    z = z.float()
    if kind == RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if kind == LEAKY:
        return torch.where(z > 0, z, z * torch.tensor(slope, dtype=torch.float32))
    if kind == HARDSWISH:
        return z * torch.clamp(z + 3.0, 0.0, 6.0) / 6.0
    assert kind == IDENTITY, kind
    return z


def act_bwd32(kind: int, g: torch.Tensor, z: torch.Tensor, slope: float = 0.0) -> torch.Tensor:
    """kod_act_bwd<> (g * act'(z)) in fp32, in the kernel's operation order."""
    g, z = g.float(), z.float()
    if kind == RELU:
        return torch.where(z > 0, g, torch.zeros_like(g))
    if kind == LEAKY:
        return torch.where(z > 0, g, g * torch.tensor(slope, dtype=torch.float32))
    if kind == HARDSWISH:
        return torch.where(z <= -3, torch.zeros_like(g), torch.where(z < 3, g * ((z / 3.0) + 0.5), g))
    assert kind == IDENTITY, kind
    return g


def apply32(y, scale, shift, kind, slope=0.0, residual=None) -> torch.Tensor:
    """The forward apply pass: z = fma(y, scale, shift), kod_act, + r, one rounding to bf16.  y / residual bf16 [M, C]."""
    a = act32(kind, fma32(y.float(), scale, shift), slope)
    if residual is not None:
        a = a + residual.float()
    return a.to(torch.bfloat16)


def bwd_apply32(dA, y, scale, shift, coef, kind, slope=0.0) -> torch.Tensor:
    """The backward apply pass: dY = fma(k1, dz, fma(k2, y, k3)), dz = kod_act_bwd(dA, fma(y, scale, shift)); bf16."""
    C = y.shape[1]
    yv = y.float()
    dz = act_bwd32(kind, dA.float(), fma32(yv, scale, shift), slope)
    return fma32(coef[:C], dz, fma32(coef[C:2 * C], yv, coef[2 * C:])).to(torch.bfloat16)
