"""Inputs and C-ABI calls of the bit pins on the BatchNorm statistics kernels and the SGD update
(tests/test_hip_stat_sgd_bits.py; tools/record_stat_sgd_bits.py stores the outputs as tests/golden/stat_sgd_bits.npz).

Every family is a function lib -> {name: int32 tensor}: inputs come from numpy generators seeded per case, outputs are
written into NaN-filled buffers with spare floats on both sides and returned whole, as their bits.  A case asserts, from
its inputs, what makes it worth running (a masked and a live element in one quad, a clamp that changes something, ...).
Nothing here starts a peer exchange."""
import numpy as np
import torch

from object_detection_cib_amd import _lib

EPS, MOM = 1e-3, 0.03
PAD = 8                      # spare floats before and after every output


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _out(n, dtype=torch.float32):
    """NaN-filled buffer of n elements with PAD spare ones on both sides; [buffer, pointer to element 0 of the payload]"""
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=dtype, device="cuda")
    return buf, buf.data_ptr() + PAD * buf.element_size()


def _bits(t):
    torch.cuda.synchronize()
    return t.view(torch.int32).cpu().clone()


def _slab(rng, C, T, off=0):
    """[2][C][T] fp32 partials at a base `off` floats past a 256-byte boundary"""
    vals = rng.standard_normal((2, C, T)).astype(np.float32) * 8
    buf = torch.zeros(2 * C * T + 64 + off, dtype=torch.float32, device="cuda")
    base = (-buf.data_ptr() // 4) % 64 + off
    slab = buf[base:base + 2 * C * T]
    slab.copy_(_dev(vals).flatten())
    return slab, vals


class _Job:
    """one coefficient job: inputs on the device, one output buffer dgamma[C] | dbeta[C] | coef[3C]"""

    def __init__(self, rng, C, T, raw, count, off=0):
        self.C, self.T, self.raw, self.count = C, T, raw, float(count)
        self.slab, self.vals = _slab(rng, C, T, off)
        self.gamma = _dev((rng.random(C) + 0.5).astype(np.float32))
        self.mean = _dev(rng.standard_normal(C).astype(np.float32))
        self.rstd = _dev((rng.random(C) + 0.5).astype(np.float32))
        self.out, self.p = _out(5 * C)

    def args(self, count=True, eval_=None):
        C = self.C
        a = [self.slab.data_ptr(), self.T] + ([self.count] if count else []) + [
            self.gamma.data_ptr(), self.mean.data_ptr(), self.rstd.data_ptr(), self.p, self.p + 4 * C, self.p + 8 * C, C, self.raw]
        return a + ([eval_] if eval_ is not None else [])

    def fresh(self):
        self.out.fill_(float("nan"))


COEF_C = [1, 3, 8, 65]
COEF_T = [1, 4, 5, 257, 1024, 1025, 3001]


def coeffs(lib):
    """kodhip_bn_bwd_coeffs_partials: one wave per channel, four per block; vector body, tail, the > 1024-slot and the
    unaligned forms of the reduction (odd T, and T = 4 / 1024 once more from a base one float off)"""
    res = {}
    for C in COEF_C:
        for T in COEF_T:
            for off in ((0, 1) if T in (4, 1024) else (0,)):
                for raw in (0, 1):
                    j = _Job(np.random.default_rng([1, C, T, off, raw]), C, T, raw, 16 * T, off)
                    assert (j.slab.data_ptr() % 16 == 4) == (off == 1)
                    _lib.check(lib.kodhip_bn_bwd_coeffs_partials(*j.args(), _stream()), "coeffs")
                    res[f"coeffs_C{C}_T{T}_o{off}_r{raw}"] = _bits(j.out)
    return res


def coeffs2(lib):
    """the two-job forms: the narrower job's surplus blocks exit; T, raw_moment and count differ between the jobs; every
    pair of modes; kodhip_bn_bwd_coeffs_partials2 is the pair (train, train)"""
    res = {}
    for C0, C1 in ((8, 65), (65, 8)):
        rng = np.random.default_rng([2, C0, C1])
        j0, j1 = _Job(rng, C0, 257, 1, 257 * 16), _Job(rng, C1, 5, 0, 5 * 3)
        m = min(C0, C1)
        assert not np.array_equal(j0.vals[:, :m, :5], j1.vals[:, :m, :5])
        _lib.check(lib.kodhip_bn_bwd_coeffs_partials2(*j0.args(), *j1.args(), _stream()), "coeffs2")
        res[f"coeffs2_{C0}_{C1}_a"], res[f"coeffs2_{C0}_{C1}_b"] = _bits(j0.out), _bits(j1.out)
        for e0, e1 in ((0, 0), (0, 1), (1, 0), (1, 1)):
            j0.fresh(), j1.fresh()
            _lib.check(lib.kodhip_bn_bwd_coeffs_eval_partials2(*j0.args(eval_=e0), *j1.args(eval_=e1), _stream()), "coeffs mode2")
            a, b = _bits(j0.out), _bits(j1.out)
            assert not torch.equal(a[PAD:PAD + m], b[PAD:PAD + m])                    # the jobs' outputs differ
            if (e0, e1) == (0, 0):
                assert torch.equal(a, res[f"coeffs2_{C0}_{C1}_a"]) and torch.equal(b, res[f"coeffs2_{C0}_{C1}_b"])
            res[f"mode2_{C0}_{C1}_{e0}{e1}_a"], res[f"mode2_{C0}_{C1}_{e0}{e1}_b"] = a, b
    return res


def coeffs_eval(lib):
    """kodhip_bn_bwd_coeffs_eval_partials (takes no count)"""
    res = {}
    for C in (3, 65):
        for T in (5, 1025):
            for raw in (0, 1):
                j = _Job(np.random.default_rng([3, C, T, raw]), C, T, raw, 0)
                _lib.check(lib.kodhip_bn_bwd_coeffs_eval_partials(*j.args(count=False), _stream()), "coeffs eval")
                res[f"eval_C{C}_T{T}_r{raw}"] = _bits(j.out)
    return res


def coeffs_sums(lib):
    """kodhip_bn_bwd_coeffs, the sums form: parameter gradients from the local sums, coefficients from the global ones"""
    res = {}
    for C in (3, 65):
        for raw in (0, 1):
            rng = np.random.default_rng([4, C, raw])
            loc, glo = rng.standard_normal(2 * C) * 50, rng.standard_normal(2 * C) * 400
            assert not np.array_equal(loc, glo)
            j, dl, dg = _Job(rng, C, 1, raw, 4096), _dev(loc), _dev(glo)
            _lib.check(lib.kodhip_bn_bwd_coeffs(dl.data_ptr(), dg.data_ptr(), j.count, *j.args()[3:], _stream()), "coeffs sums")
            res[f"sums_C{C}_r{raw}"] = _bits(j.out)
    return res


def finalize(lib):
    """both finalize routes on the same slabs: kodhip_bn_finalize_partials, and kodhip_bn_reduce_partials + kodhip_bn_finalize;
    channel 0's variance clamps to 0, the last channel of C >= 3 holds one NaN partial"""
    res = {}
    for C in (3, 65):
        for T in (5, 257, 1025):
            for count, upd in ((16.0 * T, 1), (16.0 * T, 0), (2.0, 1)):
                rng = np.random.default_rng([5, C, T, int(count), upd])
                slab, vals = _slab(rng, C, T)
                vals[1] = np.abs(vals[1]) * count                   # a plausible second moment ...
                vals[0, 0], vals[1, 0] = 3.0 * count / T, 0.0        # ... but channel 0: mean 3, E[y^2] 0
                vals[0, C - 1, T // 2] = np.nan
                slab.copy_(_dev(vals).flatten())
                s = vals.astype(np.float64).sum(2)
                assert s[1, 0] / count - (s[0, 0] / count) ** 2 < 0 and np.isnan(s[0, C - 1]) and not np.isnan(s[:, :C - 1]).any()
                gamma, beta = _dev((rng.random(C) + 0.5).astype(np.float32)), _dev(rng.standard_normal(C).astype(np.float32))
                run0 = np.concatenate([rng.standard_normal(C), rng.random(C) + 0.5]).astype(np.float32)
                for route in ("fused", "sums"):
                    aff, a = _out(4 * C)
                    run, r = _out(2 * C)
                    run[PAD:PAD + 2 * C] = _dev(run0)
                    tail = (gamma.data_ptr(), beta.data_ptr(), r, r + 4 * C, MOM, EPS, a, a + 4 * C, a + 8 * C, a + 12 * C, C, upd, _stream())
                    if route == "fused":
                        _lib.check(lib.kodhip_bn_finalize_partials(slab.data_ptr(), T, count, *tail), "finalize_partials")
                    else:
                        sums, sp = _out(2 * C, torch.float64)
                        _lib.check(lib.kodhip_bn_reduce_partials(slab.data_ptr(), sp, C, T, _stream()), "reduce_partials")
                        _lib.check(lib.kodhip_bn_finalize(sp, count, *tail), "finalize")
                        res[f"fin_C{C}_T{T}_n{int(count)}_u{upd}_sums64"] = _bits(sums)
                    res[f"fin_C{C}_T{T}_n{int(count)}_u{upd}_{route}_aff"] = _bits(aff)
                    res[f"fin_C{C}_T{T}_n{int(count)}_u{upd}_{route}_run"] = _bits(run)
                    if not upd:
                        assert torch.equal(run[PAD:PAD + 2 * C].cpu(), torch.from_numpy(run0))
    return res


def eval_constants(lib):
    """kodhip_bn_eval_constants: two descriptors in one launch, 3 channels and 300 (more than the block's 256 threads)"""
    res = {}
    assert lib.kodhip_bn_eval_desc_bytes() == 64
    for with_coef in (0, 1):
        rng = np.random.default_rng([6, with_coef])
        rows, keep, outs = [], [], []
        for C in (3, 300):
            ins = [_dev((rng.random(C) + 0.5).astype(np.float32)), _dev(rng.standard_normal(C).astype(np.float32)),
                   _dev(rng.standard_normal(C).astype(np.float32)), _dev((rng.random(C) * 4).astype(np.float32))]
            aff, a = _out(4 * C)
            coef, k = _out(3 * C)
            rows.append([t.data_ptr() for t in ins] + [a, k if with_coef else 0, C, 0])
            keep += ins
            outs += [aff, coef]
        desc = torch.tensor(rows, dtype=torch.int64, device="cuda")
        _lib.check(lib.kodhip_bn_eval_constants(desc.data_ptr(), 2, EPS, _stream()), "eval_constants")
        for i, t in enumerate(outs):
            res[f"evalconst_k{with_coef}_{i}"] = _bits(t)
    return res


# ---------------------------------------------------------------- SGD
def _hyper(nesterov=1, maximize=0, first=0, dampening=0.0):
    """lr[3] | momentum[3] | wd[3] | grad_scale | flags | dampening; group 0 has no weight decay, group 2 no momentum"""
    return _dev(np.array([0.01, 0.02, 0.03, 0.9, 0.937, 0.0, 0.0, 5e-4, 1e-3, 0.75,
                          nesterov + 2 * maximize + 4 * first, dampening], dtype=np.float32))


HYPERS = {"nest": dict(), "plain": dict(nesterov=0), "max": dict(maximize=1), "damp_first": dict(first=1, dampening=0.5),
          "damp": dict(dampening=0.5)}


class _Sgd:
    def __init__(self, n, seed, masked, nan_grad=False):
        rng = np.random.default_rng([7, n, seed])
        self.n = n
        g = n // 64
        gid = np.array([1] if g == 1 else [0, 1, 2, 255, 1, 2, 0, 1, 255, 2, 1, 0, 1, 1, 2, 0, 1][:g], dtype=np.uint8)
        assert len(gid) == g
        self.gid = _dev(gid)
        self.p0 = (rng.standard_normal(n)).astype(np.float32)
        self.b0 = (rng.standard_normal(n) * 0.1).astype(np.float32)
        grad = rng.standard_normal(n).astype(np.float32)
        keep = (rng.random(n) < 0.6).astype(np.uint8)             # partly zero quads
        keep[0:4] = 1
        keep[8:12] = 0                                            # an all-zero quad inside a live granule
        keep[12:16] = (1, 0, 1, 0)
        if g > 1:
            keep[64 * 4:64 * 5] = 0                               # whole granules frozen
            keep[64 * 6:64 * 7] = 0
            keep[64 * 5:64 * 6] = 1
        q = keep.reshape(-1, 4).sum(1)
        live = np.repeat(gid <= 2, 16)
        assert ((q > 0) & (q < 4) & live).any() and ((q == 0) & live).any() and (q == 4).any()
        if nan_grad:
            grad[13 if masked else 14] = np.nan                   # one masked and one live position in the masked form
            grad[14] = np.nan
        self.grad, self.keep_np = _dev(grad), keep
        self.keep = _dev(keep) if masked else None
        self.grad_np = grad

    def run(self, lib, hyper, clip=None, mode=0, skip=0, entry=None):
        n = self.n
        p, pp = _out(n + 2 * 56)                 # payload 64 floats in: 16-byte aligned like the arena
        b, bp = _out(n + 2 * 56)
        pp, bp = pp + 56 * 4, bp + 56 * 4
        p[64:64 + n], b[64:64 + n] = _dev(self.p0), _dev(self.b0)
        k = self.keep.data_ptr() if self.keep is not None else None
        if clip is not None:
            _lib.check(lib.kodhip_sgd_nesterov_clipped(pp, self.grad.data_ptr(), bp, self.gid.data_ptr(), k, n, hyper.data_ptr(),
                                                       clip.data_ptr(), mode, skip, _stream()), "sgd clipped")
        elif k is not None:
            _lib.check(lib.kodhip_sgd_nesterov_masked(pp, self.grad.data_ptr(), bp, self.gid.data_ptr(), k, n, hyper.data_ptr(),
                                                      _stream()), "sgd masked")
        else:
            _lib.check(lib.kodhip_sgd_nesterov(pp, self.grad.data_ptr(), bp, self.gid.data_ptr(), n, hyper.data_ptr(), _stream()), "sgd")
        return _bits(p), _bits(b)


def _clip_block(coef=1.0, value=0.0, nonfinite=0.0):
    c = np.zeros(16, dtype=np.float32)
    c[4], c[5], c[8] = coef, nonfinite, value
    return _dev(c)


SGD_N = [64, 64 * 17]


def sgd(lib):
    """kodhip_sgd_nesterov and _masked: one partly filled block and two blocks; groups 0 / 1 / 2 / 255 in mixed order"""
    res = {}
    for n in SGD_N:
        for masked in (0, 1):
            s = _Sgd(n, 0, masked)
            for name, kw in HYPERS.items():
                p, b = s.run(lib, _hyper(**kw))
                res[f"sgd_n{n}_m{masked}_{name}_p"], res[f"sgd_n{n}_m{masked}_{name}_b"] = p, b
            if masked:                            # a frozen element keeps its bits next to a live one that moved
                old, new = torch.from_numpy(s.p0).view(torch.int32), p[PAD + 56:PAD + 56 + n]
                assert new[13] == old[13] and new[12] != old[12]
    return res


def sgd_clipped(lib):
    """kodhip_sgd_nesterov_clipped in both modes: coefficient 1 (the bits of the unclipped entry points) and 0.25, a clamp
    that bites on both sides, a NaN gradient, and skip_nonfinite with the flag raised (nothing moves)"""
    res = {}
    for n in SGD_N:
        for masked in (0, 1):
            s = _Sgd(n, 1, masked)
            sn = _Sgd(n, 1, masked, nan_grad=True)
            for hname in ("nest", "damp_first"):
                h = _hyper(**HYPERS[hname])
                plain = s.run(lib, h)
                for coef in (1.0, 0.25):
                    out = s.run(lib, h, _clip_block(coef=coef, value=1e30), mode=0)
                    assert all(torch.equal(x, y) for x, y in zip(out, plain)) == (coef == 1.0)
                    res[f"clip_n{n}_m{masked}_{hname}_norm{coef}_p"], res[f"clip_n{n}_m{masked}_{hname}_norm{coef}_b"] = out
                cv = 0.5
                sg = s.grad_np * np.float32(0.75)
                live = np.repeat(s.gid.cpu().numpy() <= 2, 64) & ((s.keep_np != 0) | (not masked))
                assert (sg[live] > cv).any() and (sg[live] < -cv).any()
                out = s.run(lib, h, _clip_block(coef=0.25, value=cv), mode=1)
                assert not torch.equal(out[0], plain[0])
                res[f"clip_n{n}_m{masked}_{hname}_value_p"], res[f"clip_n{n}_m{masked}_{hname}_value_b"] = out
            h = _hyper()
            for mode in (0, 1):
                out = sn.run(lib, h, _clip_block(coef=0.25, value=0.5), mode=mode)
                res[f"clip_n{n}_m{masked}_nan_mode{mode}_p"], res[f"clip_n{n}_m{masked}_nan_mode{mode}_b"] = out
                out = s.run(lib, h, _clip_block(coef=0.25, value=0.5, nonfinite=1.0), mode=mode, skip=1)
                for t, old in zip(out, (s.p0, s.b0)):
                    assert torch.equal(t[PAD + 56:PAD + 56 + n], torch.from_numpy(old).view(torch.int32))
                    assert bool((t[:PAD + 56] == t[0]).all()) and bool((t[PAD + 56 + n:] == t[0]).all())
                res[f"clip_n{n}_m{masked}_skip_mode{mode}_p"], res[f"clip_n{n}_m{masked}_skip_mode{mode}_b"] = out
    return res


FAMILIES = [coeffs, coeffs2, coeffs_eval, coeffs_sums, finalize, eval_constants, sgd, sgd_clipped]
