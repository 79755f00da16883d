"""Gradient clipping, host side (no GPU): the new C-ABI entries refuse bad arguments before any launch, FusedSGD and the
experiment accept and forward Lightning's Trainer(gradient_clip_val, gradient_clip_algorithm), and with clipping off the
engine issues exactly the SGD launch it always did."""
import ctypes as C
from functools import partial
from types import SimpleNamespace
from unittest import mock

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from object_detection_cib_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_sizes_are_queried_not_hard_coded(lib):
    assert lib.kodhip_clip_block_bytes() == 16 * 4          # include/kodhip.h: 16 fp32, input slot at [8]
    ws = lib.kodhip_grad_norm_workspace_bytes()
    assert ws > 0 and ws % (3 * 8) == 0                     # one fp64 partial per block and group


def test_new_entries_refuse_bad_arguments_before_any_launch(lib):
    buf = (C.c_float * 256)()
    a = C.addressof(buf)                                    # a non-null pointer; validation fails before it is used
    rc = lib.kodhip_grad_norm(None, None, None, 64, None, None, None, 0, 0, None)
    assert rc < 0 and b"grad_norm" in lib.kodhip_last_error()
    rc = lib.kodhip_grad_norm(a, a, None, 65, a, a, a, 0, 0, None)
    assert rc < 0 and b"grad_norm" in lib.kodhip_last_error()
    rc = lib.kodhip_grad_norm(a, a, None, 0, a, a, a, 0, 0, None)
    assert rc < 0
    rc = lib.kodhip_sgd_nesterov_clipped(a, a, a, a, None, 64, a, None, 0, 0, None)
    assert rc < 0 and b"sgd_nesterov_clipped" in lib.kodhip_last_error()
    rc = lib.kodhip_sgd_nesterov_clipped(a, a, a, a, None, 100, a, a, 0, 0, None)
    assert rc < 0 and b"sgd_nesterov_clipped" in lib.kodhip_last_error()
    rc = lib.kodhip_sgd_nesterov_clipped(a, a, a, a, None, 64, a, a, 7, 0, None)
    assert rc < 0 and b"unknown mode 7" in lib.kodhip_last_error()
    rc = lib.kodhip_grad_clip_inplace(None, a, None, 64, a, 0, None)
    assert rc < 0 and b"grad_clip_inplace" in lib.kodhip_last_error()
    rc = lib.kodhip_grad_clip_inplace(a, a, None, 64, a, 2, None)
    assert rc < 0 and b"unknown mode 2" in lib.kodhip_last_error()
    rc = lib.kodhip_grad_clip_inplace(a, a, None, 32, a, 0, None)
    assert rc < 0


def _hip_net():
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    torch.manual_seed(0)
    return Yolov5Network(3, 4, widen_factor=0.25, deepen_factor=0.33)      # construction needs no GPU, running it does


def test_fused_sgd_keywords_and_defaults():
    from object_detection_cib_amd.nn.optim.smart import FusedSGD, SmartOptimizer
    net = _hip_net()
    opt = SmartOptimizer(partial(torch.optim.SGD, lr=0.01, momentum=0.937, nesterov=True), 5e-4)(net)
    assert isinstance(opt, FusedSGD)
    assert (opt.gradient_clip_val, opt.gradient_clip_algorithm, opt.skip_nonfinite) == (None, "norm", False)
    assert opt.clip_config() == (None, False, False)                       # today's behaviour: no clipping launches
    opt = SmartOptimizer(partial(FusedSGD, lr=0.01, momentum=0.937, nesterov=True, gradient_clip_val=2.5,
                                 gradient_clip_algorithm="value", skip_nonfinite=True), 5e-4)(net)
    assert (opt.gradient_clip_val, opt.gradient_clip_algorithm, opt.skip_nonfinite) == (2.5, "value", True)
    assert opt.clip_config() == ("value", True, False)
    assert [g["name"] for g in opt.param_groups] == ["bias_params", "decay_params", "norm_params"]
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        FusedSGD(list(net.parameters()), lr=0.01, net=net, gradient_clip_val=1.0, gradient_clip_algorithm="agc")
    opt.gradient_clip_algorithm = "inf-norm"                               # set later, as the experiment sets attributes
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        opt.clip_config()


def _experiment(net, **kw):
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
    return DefaultYolov5Experiment(net, loss=None, anchor_info=None, **kw)


def test_experiment_forwards_trainer_arguments():
    from object_detection_cib_amd.nn.optim.smart import FusedSGD, SmartOptimizer
    net = _hip_net()
    exp = _experiment(net)
    assert exp.get_metrics_to_display() == ["box", "cls", "obj"]
    (opt,), _ = exp.configure_optimizers()
    assert isinstance(opt, FusedSGD) and opt.clip_config() == (None, False, False)
    assert exp.get_metrics_to_display() == ["box", "cls", "obj"]
    exp = _experiment(net, gradient_clip_val=10.0)
    assert exp.get_metrics_to_display() == ["box", "cls", "obj", "grad_norm"]
    (opt,), _ = exp.configure_optimizers()
    assert opt.clip_config() == ("norm", False, True) and opt.gradient_clip_val == 10.0
    exp = _experiment(net, gradient_clip_val=0.5, gradient_clip_algorithm="value", graphed=True)
    (opt,), _ = exp.configure_optimizers()
    assert opt.clip_config() == ("value", False, True) and opt.gradient_clip_val == 0.5
    # a partial(FusedSGD, ...) that carries the keywords keeps them when the experiment has none
    exp = _experiment(net, smart_optimizer=SmartOptimizer(partial(FusedSGD, lr=0.01, momentum=0.9, gradient_clip_val=3.0), 5e-4))
    (opt,), _ = exp.configure_optimizers()
    assert opt.gradient_clip_val == 3.0 and exp.get_metrics_to_display()[-1] == "grad_norm"
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        _experiment(net, gradient_clip_val=1.0, gradient_clip_algorithm="agc")


class _Recorder:
    """stands in for the ctypes handle: records the entry points the engine calls, in order"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _fake_engine(frozen: bool):
    from object_detection_cib_amd.engine.arenas import ArenaMixin
    t = lambda v: SimpleNamespace(data_ptr=lambda: v)
    rec = _Recorder()
    eng = mock.MagicMock()
    eng.lib = rec
    eng.CLIP_MODES = ArenaMixin.CLIP_MODES
    eng.p_arena, eng.m_arena, eng.gid, eng.hyper, eng.clip, eng.norm_ws = t(1), t(2), t(3), t(4), t(5), t(6)
    eng.keep_mask = t(7)
    eng.current_grad_arena = lambda: t(8)
    eng._count_mask = lambda: t(9)
    eng.n_arena, eng.param_version, eng.norm_nontemporal = 640, 0, False
    eng._stream = lambda: 0
    eng.freeze_active = lambda: (object() if frozen else None)
    eng.grad_norm_device = lambda hyper=None: ArenaMixin.grad_norm_device(eng, hyper)
    eng.clip_algorithm, eng.clip_skip_nonfinite, eng.track_grad_norm = None, False, False
    return eng, rec


@pytest.mark.parametrize("frozen", [False, True])
def test_launch_order_of_the_optimizer_step(frozen):
    """clipping off: the parent's single SGD launch, entry for entry; on: norm, then the SGD form that consumes it"""
    from object_detection_cib_amd.engine.arenas import ArenaMixin
    plain = "kodhip_sgd_nesterov_masked" if frozen else "kodhip_sgd_nesterov"

    def run(algo, skip, track):
        eng, rec = _fake_engine(frozen)
        ArenaMixin.configure_clip(eng, algo, skip, track)
        ArenaMixin.sgd_step_device(eng)
        assert eng.note_sgd_step.call_count == 1 and eng.param_version == 1
        return rec.calls

    calls = run(None, False, False)
    assert [c[0] for c in calls] == [plain]
    assert calls[0][1] == ((1, 8, 2, 3, 7, 640, 4, 0) if frozen else (1, 8, 2, 3, 640, 4, 0))
    assert [c[0] for c in run(None, False, True)] == ["kodhip_grad_norm", plain]          # track only: the update stays
    calls = run("norm", False, False)
    assert [c[0] for c in calls] == ["kodhip_grad_norm", "kodhip_sgd_nesterov_clipped"]
    assert calls[0][1] == (8, 3, 9, 640, 4, 5, 6, 0, 0, 0)
    assert calls[1][1] == (1, 8, 2, 3, 7 if frozen else None, 640, 4, 5, 0, 0, 0)
    calls = run("value", False, False)                                                    # no reduction needed
    assert [c[0] for c in calls] == ["kodhip_sgd_nesterov_clipped"] and calls[0][1][8:10] == (1, 0)
    calls = run("value", True, False)
    assert [c[0] for c in calls] == ["kodhip_grad_norm", "kodhip_sgd_nesterov_clipped"]
    assert calls[0][1][7] == 1 and calls[1][1][8:10] == (1, 1)
    calls = run(None, True, False)                       # skip without a clip value: norm form, max_norm = +inf
    assert [c[0] for c in calls] == ["kodhip_grad_norm", "kodhip_sgd_nesterov_clipped"] and calls[1][1][8:10] == (0, 1)
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        ArenaMixin.configure_clip(_fake_engine(False)[0], "agc")
