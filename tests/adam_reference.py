"""Plain numpy restatement of the fused Adam / AdamW update (csrc/adam.hip): the yardstick of tests/test_adam_reference.py
(against CPU torch.optim.Adam / AdamW) and tests/test_hip_adam.py (the kernel, bit for bit).

All values are fp32 and every operation is rounded once, in the order of the kernel:

    gg = g * gscale;  [norm: gg = gg * coef | value: clamp, a NaN stays];  maximize: gg = -gg
    Adam  (wd != 0): gg = fma(p, wd, gg)            AdamW (wd != 0): p = p * c_decay
    m = fma(gg - m, omb1, m)
    v = fma(omb2 * gg, gg, v * beta2)
    den = sqrt(v) / bc2s + eps
    p = p + (nss * m) / den

`fma32` is an exact fp32 fused multiply-add.  The product of two fp32 values is exact in fp64 (24 + 24 significant bits); the
sum with the addend is then rounded ONCE to fp64 and a second time to fp32, and that double rounding is wrong in rare cases
(`float32(float64(a) * b + c)` is NOT a fused multiply-add).  The fp64 sum is therefore rounded to odd: TwoSum gives its exact
residual, and where the residual is not zero and the sum's last mantissa bit is even, the sum moves to its odd fp64
neighbour on the residual's side.  Rounding a round-to-odd fp64 value (53 >= 2 * 24 + 2 bits) to fp32 gives the correctly
rounded fp32 result.  (math.fma, where a Python has it, works on doubles and returns that same once-rounded fp64 sum: it
does not remove the second rounding, so it is not used.)

`host_constants` forms the per-group constants in Python doubles as torch's single-tensor non-capturable path forms them
(torch/optim/adam.py _single_tensor_adam) and rounds them to fp32.
"""
import numpy as np

F = np.float32


def fma32(a, b, c):
    """fp32(a * b + c) with ONE rounding, elementwise; a NaN / Inf anywhere goes the IEEE way"""
    a, b, c = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(all="ignore"):
        p = a * b                                   # exact
        s = p + c
        bb = s - p                                  # TwoSum: s + e == p + c exactly
        e = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def host_constants(lr, beta1, beta2, eps, wd, step):
    """-> dict of fp32 scalars for one group at optimizer step `step` (1-based)"""
    lr, beta1, beta2, eps, wd = float(lr), float(beta1), float(beta2), float(eps), float(wd)
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    return dict(nss=F(-step_size), beta2=F(beta2), omb1=F(1 - beta1), omb2=F(1 - beta2), bc2s=F(bias_correction2 ** 0.5),
                eps=F(eps), wd=F(wd), c_decay=F(1 - lr * wd))


def adam_ref(p, g, m, v, c, gscale=1.0, maximize=False, decoupled=False, clip_mode=None, coef=1.0, clip_value=0.0):
    """One step over fp32 arrays with one group's constants `c` (host_constants).  -> (p, m, v), new arrays."""
    p, g, m, v = (np.asarray(t, dtype=np.float32) for t in (p, g, m, v))
    with np.errstate(all="ignore"):
        gg = g * F(gscale)
        if clip_mode == "norm":
            gg = gg * F(coef)
        elif clip_mode == "value":
            cv = F(clip_value)
            gg = np.where(gg < -cv, -cv, np.where(gg > cv, cv, gg)).astype(np.float32)
        if maximize:
            gg = -gg
        if c["wd"] != 0:
            if decoupled:
                p = p * c["c_decay"]
            else:
                gg = fma32(p, c["wd"], gg)
        m2 = fma32(gg - m, c["omb1"], m)
        v2 = fma32(c["omb2"] * gg, gg, v * c["beta2"])
        den = np.sqrt(v2) / c["bc2s"] + c["eps"]
        p2 = p + (c["nss"] * m2) / den
    assert p2.dtype == m2.dtype == v2.dtype == np.float32
    return p2, m2, v2


def adam_ref_arena(p, g, m, v, gid, keep, consts, **kw):
    """The kernel's view: flat arenas, group id per 64-element granule (above 2: skipped), optional u8 keep mask per element
    (0: untouched), per-group constants consts[0..2].  -> (p, m, v), new arrays."""
    p, m, v = (np.array(t, dtype=np.float32, copy=True) for t in (p, m, v))
    ge = np.repeat(np.asarray(gid), 64)
    for grp in range(3):
        sel = ge == grp
        if keep is not None:
            sel &= np.asarray(keep) != 0
        if sel.any():
            p[sel], m[sel], v[sel] = adam_ref(p[sel], np.asarray(g, dtype=np.float32)[sel], m[sel], v[sel], consts[grp], **kw)
    return p, m, v


def hyper_block(consts, gscale, maximize, decoupled, floats=32):
    """the device block of csrc/adam.hip from three groups' constants"""
    h = np.zeros(floats, dtype=np.float32)
    for k, base in (("nss", 0), ("beta2", 3), ("omb1", 6), ("omb2", 12), ("bc2s", 15), ("eps", 18), ("wd", 21), ("c_decay", 24)):
        for grp in range(3):
            h[base + grp] = consts[grp][k]
    h[9] = gscale
    h[10] = (1 if maximize else 0) + (2 if decoupled else 0)
    return h


def ulp_distance(a, b):
    """|a - b| in units of the last place over finite fp32 arrays of equal sign pattern handling (monotone integer map)"""
    def key(x):
        i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-2 ** 31) - i, i)
    return np.abs(key(a) - key(b))
