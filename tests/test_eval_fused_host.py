"""The fused eval forward's host side (no GPU): argument validation of kodhip_conv_fwd_fused, option parsing, and the
conditions on inputs and references under which tests/test_hip_conv_fused.py compares without a tolerance."""
from __future__ import annotations

import pytest

from object_detection_cib_amd import _lib
from object_detection_cib_amd.engine.options import EngineOptions
from fused_reference import (ACT_HARDSWISH, ACT_SILU, CASES, EXACT_ACTS, SMOOTH_CASES, STEM_CASES, check_exact_conditions,
                             check_smooth_conditions, problem, stem_problem)


@pytest.fixture(scope="module")
def lib():
    """The library, built if it is not there yet (this file must run on its own in a clean checkout)."""
    from object_detection_cib_amd import build
    build.build(verbose=False)
    return _lib.lib()


FAKE = 4096          # never dereferenced: every call below is refused before a launch


def call(lib, x=FAKE, w=FAKE, scale=FAKE, shift=FAKE, residual=None, ldr=0, rcoff=0, out=FAKE, B=1, H=8, W=8, ldx=32, xcoff=0,
         Cin=32, N=32, k=1, s=1, p=0, Kp=32, ldo=32, ocoff=0, act=0, slope=0.0):
    return lib.kodhip_conv_fwd_fused(x, w, scale, shift, residual, ldr, rcoff, out, B, H, W, ldx, xcoff, Cin, N, k, k, s, s, p, p,
                                     Kp, ldo, ocoff, act, slope, None)


@pytest.mark.parametrize("kw", [dict(scale=None), dict(shift=None), dict(out=None), dict(act=7), dict(act=-1),
                                dict(residual=FAKE, ldr=40, rcoff=16), dict(residual=FAKE, ldr=36, rcoff=0),
                                dict(Cin=12, ldx=12, Kp=32), dict(N=36, ldo=40), dict(x=None), dict(Kp=64)],
                         ids=["null_scale", "null_shift", "null_out", "act_7", "act_negative", "residual_slice_out_of_range",
                              "residual_ld_not_8", "cin_not_8", "n_not_8", "null_x", "bad_kp"])
def test_fused_refuses_bad_arguments(lib, kw):
    """refused before any launch, with the entry point's name in kodhip_last_error"""
    rc = call(lib, **kw)
    err = lib.kodhip_last_error().decode()
    assert rc < 0, (kw, rc)
    assert "conv_fwd_fused" in err, (kw, err)


def test_version_bumped(lib):
    assert lib.kodhip_version() >= 101


def test_option_parsing(monkeypatch):
    monkeypatch.delenv("KODHIP_EVAL_FUSED", raising=False)
    assert EngineOptions().eval_fused is False
    assert EngineOptions.from_env().eval_fused is False
    assert EngineOptions.from_env().as_dict()["eval_fused"] is False
    monkeypatch.setenv("KODHIP_EVAL_FUSED", "1")
    assert EngineOptions.from_env().eval_fused is True
    assert EngineOptions.from_env().as_dict()["eval_fused"] is True
    monkeypatch.setenv("KODHIP_EVAL_FUSED", "0")
    assert EngineOptions.from_env().eval_fused is False


@pytest.mark.parametrize("cid", list(CASES))
def test_exact_cases_are_determined_and_not_vacuous(cid):
    """Per case and activation: below 2^24 in units of 2^-5, z / act(z) / bf16(act(z)) + r are fp32 numbers, >= 10 % of act(z)
    are no bf16 numbers, and two roundings differ from one on >= 1 % of the elements."""
    pr = problem(cid)
    for act in EXACT_ACTS:
        share, differ = check_exact_conditions(f"{cid} act {act}", pr, act, True)
        print(f"INPUTS {cid} act {act}: act(z) rounds {share:.3f}, two roundings differ from one on {differ:.3f}")


@pytest.mark.parametrize("N,B,H,W,bn", STEM_CASES, ids=lambda v: str(v))
def test_stem_cases_are_determined_and_not_vacuous(N, B, H, W, bn):
    pr = stem_problem(N, B, H, W)
    for act in EXACT_ACTS:
        share, differ = check_exact_conditions(f"stem N={N} act {act}", pr, act, True)
        print(f"INPUTS stem N={N} act {act}: act(z) rounds {share:.3f}, two roundings differ from one on {differ:.3f}")


@pytest.mark.parametrize("cid", SMOOTH_CASES)
def test_smooth_cases_are_bounded(cid):
    """SiLU / Hardswish: |z| <= 128, exact in fp32, and at most 5 % of the float64 activations lie near a rounding boundary."""
    pr = problem(cid, True)
    for act in (ACT_SILU, ACT_HARDSWISH):
        near = check_smooth_conditions(f"{cid} act {act}", pr, act)
        print(f"INPUTS {cid} act {act}: near a rounding boundary {near:.4f}")


def test_public_interface_without_an_engine():
    """fuse_eval() before the engine exists only records the choice: it returns self and converts no parameter or buffer;
    the experiment's eval_fused is keyword-only and defaults to None (leave the engine's option alone)."""
    import inspect
    import torch
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
    from object_detection_cib_amd.nn.graph_module import GraphModule
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    torch.manual_seed(0)
    net = Yolov5Network(3, 4, widen_factor=0.25, deepen_factor=0.33)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    assert net.fuse_eval() is net and net._eval_fused is True
    assert net.fuse_eval(False) is net and net._eval_fused is False
    after = net.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], v) for k, v in before.items())
    assert callable(getattr(GraphModule, "fuse_eval"))
    par = inspect.signature(DefaultYolov5Experiment.__init__).parameters["eval_fused"]
    assert par.kind is inspect.Parameter.KEYWORD_ONLY and par.default is None
