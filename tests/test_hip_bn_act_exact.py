"""The BatchNorm apply / backward passes for the activations other than SiLU, bit for bit.

Since the activation became a template parameter of the tuned kernels, ReLU, LeakyReLU, Hardswish and identity run
through ten launch-shape instantiations per pass.  The library is built with -fno-fast-math -ffp-contract=off and these
four activations use only IEEE operations, so apply and backward apply are compared with torch.equal against the fp32
restatement of tests/bn_reference.py (apply32 / bwd_apply32; pinned to the fp64 reference on the CPU in
tests/test_bn_reference.py), inside NaN-filled buffers and through sliced operands.  The backward reduction is pinned
with integer operands whose sums are exact in fp32 in any order.  The instantiations behind the KODHIP_BN_* knobs run
this file again in one child process each."""
import os
import subprocess
import sys

import pytest
import torch

import bn_reference as R
from hip_helpers import stream
from object_detection_cib_amd import _lib

gpu = pytest.mark.gpu

KNOBS = ("KODHIP_BN_GRID", "KODHIP_BN_U", "KODHIP_BN_LDS", "KODHIP_BN_BLOCK")
# (C, M): constants in LDS backward + 26 chunks with a ragged last one | 40-row line-aligned chunks | ... | two rows per
# thread, constants in registers | second row of the last pair out of range | fewer rows than one block | widest tensor
SHAPES = [(32, 3219), (48, 3219), (64, 3219), (96, 2139), (128, 2139), (256, 17), (32, 5), (2048, 3)]
ACTS = [(R.RELU, 0.0), (R.LEAKY, 0.5), (R.HARDSWISH, 0.0), (R.IDENTITY, 0.0)]
_CACHE = {}


def _bf16_grid(g, shape, lim):
    """bf16-representable values in [-lim, lim]."""
    return (torch.randn(shape, generator=g) * (lim / 4)).clamp(-lim, lim).to(torch.bfloat16)


def _case(C, M):
    """Operands of one shape (host tensors), shared by the tests and never modified.  scale, shift, the coefficients and
    the slope are bf16-representable and every value is within [-32, 32]: products then carry 16 significant bits and the
    fp64 emulation of fma is exact except where the addends lie more than 53 bits apart."""
    if (C, M) not in _CACHE:
        g = torch.Generator().manual_seed(1000 * C + M)
        d = dict(y=_bf16_grid(g, (M, C), 8.0), res=_bf16_grid(g, (M, C + 8), 8.0), dA=_bf16_grid(g, (M, C + 16), 8.0),
                 dI=_bf16_grid(g, (M, C + 8), 8.0), scale=_bf16_grid(g, (C,), 2.0).float(), shift=_bf16_grid(g, (C,), 4.0).float(),
                 coef=_bf16_grid(g, (3 * C,), 4.0).float())
        # values on the kinks 0, -3, 3: channels 0..2 of the first rows get scale 1, shift 0
        d["scale"][:3] = 1.0; d["shift"][:3] = 0.0
        d["y"][: min(M, 3), :3] = torch.tensor([[0.0, -3.0, 3.0]] * min(M, 3), dtype=torch.bfloat16)
        for k, v in d.items():
            assert v.float().abs().max().item() <= 32.0, k
            assert torch.equal(v.float(), v.to(torch.bfloat16).float()), k
        _CACHE[(C, M)] = d
    return _CACHE[(C, M)]


def _nan(shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device="cuda")


def _same(got, want, what):
    """torch.equal on the payload, NaN everywhere else."""
    assert not torch.isnan(got).any(), what + ": NaN in the payload"
    assert torch.equal(got.cpu().float(), want.float()), \
        f"{what}: {(got.cpu().float() != want.float()).sum().item()} of {want.numel()} elements differ"


@gpu
@pytest.mark.parametrize("kind,slope", ACTS, ids=["relu", "leaky", "hardswish", "identity"])
@pytest.mark.parametrize("C,M", SHAPES)
def test_apply_and_backward_apply_bit_exact(C, M, kind, slope):
    lib = _lib.lib()
    d = _case(C, M)
    assert torch.equal(torch.tensor(slope).to(torch.bfloat16).float(), torch.tensor(slope))
    y, sc, sh, coef = d["y"].cuda(), d["scale"].cuda(), d["shift"].cuda(), d["coef"].cuda()
    res, dA = d["res"].cuda(), d["dA"].cuda()
    for with_res in (False, True):
        out = _nan((M, C + 16))
        _lib.check(lib.kodhip_bn_act_apply(y.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), res.data_ptr() if with_res else None,
                                           C + 8, 8, out.data_ptr(), C + 16, 8, M, C, kind, slope, stream()))
        want = R.apply32(d["y"], d["scale"], d["shift"], kind, slope, d["res"][:, 8:] if with_res else None)
        _same(out[:, 8:8 + C], want, f"apply res={with_res}")
        assert torch.isnan(out[:, :8]).all() and torch.isnan(out[:, 8 + C:]).all(), "apply wrote outside its slice"
    want = R.bwd_apply32(d["dA"][:, 8:8 + C], d["y"], d["scale"], d["shift"], d["coef"], kind, slope)
    for mode in (0, 1, 2):                       # dI absent | stored | accumulated
        yy, dI = y.clone(), d["dI"].cuda()
        _lib.check(lib.kodhip_bn_act_bwd_apply(dA.data_ptr(), C + 16, 8, yy.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), coef.data_ptr(),
                                               dI.data_ptr() if mode else None, C + 8, 8, 1 if mode == 2 else 0, M, C, kind, slope,
                                               stream()))
        _same(yy, want, f"backward apply mode={mode}")
        wi = d["dI"].clone()
        if mode == 1:
            wi[:, 8:] = d["dA"][:, 8:8 + C]
        if mode == 2:
            wi[:, 8:] = (d["dA"][:, 8:8 + C].float() + d["dI"][:, 8:].float()).to(torch.bfloat16)
        _same(dI, wi, f"dI mode={mode}")


@gpu
@pytest.mark.parametrize("kind,slope", [(R.RELU, 0.0), (R.LEAKY, 0.5), (R.IDENTITY, 0.0)], ids=["relu", "leaky", "identity"])
@pytest.mark.parametrize("C,M", SHAPES + [(32, 20011)])
def test_backward_reduce_exact_on_integers(C, M, kind, slope):
    """y, dA integers in [-8, 8], scale 1 | 2, shift / mean integers, rstd 0.5 | 1 | 2: every term is a multiple of 0.25
    and every partial sum is exact in fp32 in any order, so the fp64 sum over a channel's slots is the exact sum.
    32 x 20011: 64 blocks of 64 rows, four rows in flight per thread = 16 384 rows per trip of the kernel's outer loop - a
    second, ragged trip (on the other shapes one trip covers the tensor)."""
    lib = _lib.lib()
    g = torch.Generator().manual_seed(C + M + kind)
    y = torch.randint(-8, 9, (M, C), generator=g).float()
    dA = torch.randint(-8, 9, (M, C + 16), generator=g).float()
    scale = torch.randint(1, 3, (C,), generator=g).float(); shift = torch.randint(-4, 5, (C,), generator=g).float()
    mean = torch.randint(-4, 5, (C,), generator=g).float(); rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    for name, v, lim in (("y", y, 8), ("dA", dA, 8), ("scale", scale, 2), ("shift", shift, 4), ("mean", mean, 4), ("rstd", rstd, 2)):
        assert torch.equal(v, v.to(torch.bfloat16).float()) and v.abs().max().item() <= lim, name       # bf16-representable
        assert torch.equal(v * 2, (v * 2).round()), name                                                 # multiples of 0.5
    assert torch.equal(scale, scale.round()) and torch.equal(shift, shift.round()) and torch.equal(mean, mean.round())
    assert float(slope) in (0.0, 0.5)
    z = y.double() * scale.double() + shift.double()
    dz = dA[:, 8:8 + C].double() * R.act_grad(kind, z, slope)
    want = torch.stack([dz.sum(0), (dz * (y.double() - mean.double()) * rstd.double()).sum(0)])
    assert (dz.abs() * (y.double() - mean.double()).abs() * rstd.double()).sum(0).max().item() < 2 ** 22   # exact in fp32 at 0.25 steps
    T = lib.kodhip_bn_bwd_slots(M, C)
    part = torch.full((2, C, T), float("nan"), device="cuda")
    dev = [t.cuda() for t in (dA.to(torch.bfloat16), y.to(torch.bfloat16), scale, shift, mean, rstd)]
    _lib.check(lib.kodhip_bn_act_bwd_reduce(dev[0].data_ptr(), C + 16, 8, dev[1].data_ptr(), C, dev[2].data_ptr(), dev[3].data_ptr(),
                                            dev[4].data_ptr(), dev[5].data_ptr(), part.data_ptr(), M, C, kind, slope, stream()))
    assert not torch.isnan(part).any(), "a partial slot was left unwritten"
    assert torch.equal(part.double().sum(2).cpu(), want)


@gpu
@pytest.mark.parametrize("C,M", SHAPES)
def test_silu_entry_points_write_equal_bits(C, M):
    """kodhip_bn_silu_* and kodhip_bn_act_*(act = 0) are one implementation."""
    lib = _lib.lib()
    d = _case(C, M)
    y, sc, sh, coef, res, dA = (d[k].cuda() for k in ("y", "scale", "shift", "coef", "res", "dA"))
    mean, rstd = d["shift"].cuda(), (d["scale"].abs() + 0.5).cuda()
    o0, o1 = _nan((M, C + 16)), _nan((M, C + 16))
    _lib.check(lib.kodhip_bn_silu_apply(y.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), res.data_ptr(), C + 8, 8, o0.data_ptr(), C + 16, 8, M, C, stream()))
    _lib.check(lib.kodhip_bn_act_apply(y.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), res.data_ptr(), C + 8, 8, o1.data_ptr(), C + 16, 8, M, C, 0, 0.0, stream()))
    assert torch.equal(o0.view(torch.int16), o1.view(torch.int16)) and not torch.isnan(o0[:, 8:8 + C]).any()
    T = lib.kodhip_bn_bwd_slots(M, C)
    p0, p1 = (torch.full((2 * C * T,), float("nan"), device="cuda") for _ in range(2))
    _lib.check(lib.kodhip_bn_silu_bwd_reduce(dA.data_ptr(), C + 16, 8, y.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), rstd.data_ptr(), p0.data_ptr(), M, C, stream()))
    _lib.check(lib.kodhip_bn_act_bwd_reduce(dA.data_ptr(), C + 16, 8, y.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), mean.data_ptr(), rstd.data_ptr(), p1.data_ptr(), M, C, 0, 0.0, stream()))
    assert torch.equal(p0, p1) and not torch.isnan(p0).any()
    y0, y1, i0, i1 = y.clone(), y.clone(), d["dI"].cuda(), d["dI"].cuda()
    _lib.check(lib.kodhip_bn_silu_bwd_apply(dA.data_ptr(), C + 16, 8, y0.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), coef.data_ptr(), i0.data_ptr(), C + 8, 8, 1, M, C, stream()))
    _lib.check(lib.kodhip_bn_act_bwd_apply(dA.data_ptr(), C + 16, 8, y1.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), coef.data_ptr(), i1.data_ptr(), C + 8, 8, 1, M, C, 0, 0.0, stream()))
    assert torch.equal(y0, y1) and torch.equal(i0, i1) and not torch.isnan(y0).any()


KNOB_RUNS = [
    {"KODHIP_BN_GRID": "3"},                             # more than one trip of the grid-stride loop
    {"KODHIP_BN_U": "4"},
    {"KODHIP_BN_U": "1", "KODHIP_BN_LDS": "1"},
    {"KODHIP_BN_LDS": "-1"},
    {"KODHIP_BN_BLOCK": "1024"},
]


@gpu
@pytest.mark.parametrize("knobs", KNOB_RUNS, ids=[",".join(f"{k}={v}" for k, v in r.items()) for r in KNOB_RUNS])
def test_instantiations_behind_the_knobs(knobs):
    """This file again in a fresh process per setting (the knobs are read once per process); one child at a time."""
    if any(os.environ.get(k) for k in KNOBS):
        pytest.skip("already inside a knob run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        "not test_instantiations_behind_the_knobs"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **knobs), cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "passed" in r.stdout
