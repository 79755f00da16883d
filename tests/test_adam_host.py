"""Fused Adam / AdamW, host side (no GPU): kodhip_adam_step refuses bad arguments before any launch, the hyper block's length
is queried, FusedAdam refuses what it has no form for, SmartOptimizer maps torch.optim.Adam / AdamW over a HIP network to the
fused classes, and the engine issues the norm reduction and ONE kodhip_adam_step in the order sgd_step_device() uses."""
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


def test_hyper_block_length_is_queried(lib):
    from object_detection_cib_amd.engine.arenas import ADAM_HYPER_FLOATS, adam_hyper_values
    assert lib.kodhip_adam_hyper_floats() == ADAM_HYPER_FLOATS
    assert len(adam_hyper_values([1e-3] * 3, [(0.9, 0.999)] * 3, [1e-8] * 3, [0.0] * 3, 1)) == ADAM_HYPER_FLOATS


def test_adam_step_refuses_bad_arguments_before_any_launch(lib):
    buf = (C.c_float * 256)()
    a = C.addressof(buf)                                    # a non-null pointer; validation fails before it is used
    for args in ((None, a, a, a, a), (a, None, a, a, a), (a, a, None, a, a), (a, a, a, None, a), (a, a, a, a, None)):
        rc = lib.kodhip_adam_step(*args, None, 64, a, None, -1, None)
        assert rc < 0 and b"adam_step" in lib.kodhip_last_error()
    rc = lib.kodhip_adam_step(a, a, a, a, a, None, 64, None, None, -1, None)            # no hyper block
    assert rc < 0 and b"adam_step" in lib.kodhip_last_error()
    for n in (100, 65, 0, -64):
        rc = lib.kodhip_adam_step(a, a, a, a, a, None, n, a, None, -1, None)
        assert rc < 0 and b"adam_step" in lib.kodhip_last_error() and b"64" in lib.kodhip_last_error()
    for mode in (0, 1):                                     # a clip mode without a clip block
        rc = lib.kodhip_adam_step(a, a, a, a, a, None, 64, a, None, mode, None)
        assert rc < 0 and b"adam_step" in lib.kodhip_last_error() and b"clip" in lib.kodhip_last_error()
    rc = lib.kodhip_adam_step(a, a, a, a, a, None, 64, a, a, 7, None)
    assert rc < 0 and b"adam_step" in lib.kodhip_last_error() and b"7" in lib.kodhip_last_error()
    rc = lib.kodhip_adam_step(a, a, a, a, a, None, 64, a, a, -1, None)                  # a clip block without a mode
    assert rc < 0 and b"adam_step" in lib.kodhip_last_error()


def _hip_net():
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    torch.manual_seed(0)
    return Yolov5Network(3, 4, widen_factor=0.25, deepen_factor=0.33)      # construction needs no GPU, running it does


def test_refusals():
    from object_detection_cib_amd.nn.optim.smart import FusedAdam, FusedAdamW
    net = _hip_net()
    ps = list(net.parameters())
    for kw in (dict(amsgrad=True), dict(capturable=True), dict(differentiable=True), dict(foreach=False), dict(fused=True)):
        with pytest.raises(NotImplementedError):
            FusedAdam(ps, net=net, **kw)
    for b1 in (0.0, 0.3, 0.4999, 1.0, 1.5):
        with pytest.raises(ValueError, match="beta"):
            FusedAdam(ps, betas=(b1, 0.999), net=net)
    with pytest.raises(ValueError, match="beta"):
        FusedAdamW(ps, betas=(0.9, 1.0), net=net)
    FusedAdam(ps, betas=(0.5, 0.0), net=net)                 # the edges that are accepted
    with pytest.raises(ValueError, match="skip_nonfinite"):
        FusedAdam(ps, net=net, skip_nonfinite=True)
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        FusedAdam(ps, net=net, gradient_clip_val=1.0, gradient_clip_algorithm="agc")
    with pytest.raises(ValueError, match="learning rate"):
        FusedAdam(ps, lr=-1.0, net=net)
    opt = FusedAdamW(ps, net=net)
    assert opt.defaults["weight_decay"] == 1e-2 and opt.defaults["decoupled_weight_decay"] is True
    opt.skip_nonfinite = True                                # set later, as an experiment sets attributes
    with pytest.raises(ValueError, match="skip_nonfinite"):
        opt.clip_config()


def test_smart_optimizer_maps_adam_and_adamw():
    from object_detection_cib_amd.nn.optim.smart import FusedAdam, FusedAdamW, SmartAdamW, SmartOptimizer
    net = _hip_net()
    opt = SmartOptimizer(partial(torch.optim.AdamW, lr=1e-3), 5e-4)(net)
    assert type(opt) is FusedAdamW
    assert [g["name"] for g in opt.param_groups] == ["bias_params", "decay_params", "norm_params"]
    assert [g["weight_decay"] for g in opt.param_groups] == [1e-2, 5e-4, 0.0]
    h = opt.hyper()
    assert h["decoupled"] is True and h["maximize"] is False and h["step"] == 1
    assert h["lr"] == [1e-3] * 3 and h["betas"] == [(0.9, 0.999)] * 3 and h["weight_decay"] == [1e-2, 5e-4, 0.0]
    opt = SmartOptimizer(partial(torch.optim.Adam, lr=2e-3, betas=(0.937, 0.999), maximize=True), 5e-4)(net)
    assert type(opt) is FusedAdam and opt.hyper()["decoupled"] is False and opt.hyper()["maximize"] is True
    assert [g["weight_decay"] for g in opt.param_groups] == [0, 5e-4, 0.0]
    opt.param_groups[1]["lr"] = 7e-4                           # a scheduler's write is what the next step uploads
    opt.param_groups[1]["betas"] = (0.3, 0.999)
    with pytest.raises(ValueError, match="beta"):
        opt.hyper()
    opt.param_groups[1]["betas"] = (0.9, 0.99)
    assert opt.hyper()["lr"][1] == 7e-4 and opt.hyper()["betas"][1] == (0.9, 0.99)
    opt = SmartAdamW(net, lr=3e-4, weight_decay=0.05)
    assert type(opt) is FusedAdamW and [g["weight_decay"] for g in opt.param_groups] == [0.0, 0.05, 0.0]
    assert all(g["initial_lr"] == 3e-4 for g in opt.param_groups)
    # the param-group keys of state_dict() are the installed torch's, plus name and initial_lr
    want = set(torch.optim.Adam([torch.zeros(1)]).state_dict()["param_groups"][0]) | {"name", "initial_lr"}
    sd = opt.state_dict()
    assert all(set(g) == want for g in sd["param_groups"]) and sd["state"] == {}
    # a torch network keeps torch's optimizer
    tnet = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 1), torch.nn.BatchNorm2d(4))
    assert type(SmartOptimizer(partial(torch.optim.AdamW, lr=1e-3), 5e-4)(tnet)) is torch.optim.AdamW


def test_experiment_and_captured_step_accept_and_refuse():
    from object_detection_cib_amd.engine.graphed import GraphedTrainStep
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
    from object_detection_cib_amd.nn.optim.smart import FusedAdamW, SmartOptimizer
    net = _hip_net()
    exp = DefaultYolov5Experiment(net, loss=None, anchor_info=None, world_size=4, gradient_clip_val=10.0, graphed=True,
                                  smart_optimizer=SmartOptimizer(partial(torch.optim.AdamW, lr=1e-3), 5e-4))
    (opt,), _ = exp.configure_optimizers()
    assert type(opt) is FusedAdamW and opt.world_size == 4
    assert opt.clip_config() == ("norm", False, True) and opt.gradient_clip_val == 10.0
    assert exp._graphed_optimizer() == "adam" and exp.get_metrics_to_display()[-1] == "grad_norm"
    with pytest.raises(ValueError, match="optimizer"):
        GraphedTrainStep.__init__(mock.MagicMock(), net, None, 2, 64, 64, optimizer="lion")
    with pytest.raises(ValueError, match="skip_nonfinite"):
        GraphedTrainStep.__init__(mock.MagicMock(), net, None, 2, 64, 64, optimizer="adam", skip_nonfinite=True)


class _Recorder:
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
    eng.keep_mask, eng.v_arena, eng.adam_hyper = t(7), t(10), t(11)
    eng.current_grad_arena = lambda: t(8)
    eng._count_mask = lambda: t(9)
    eng.n_arena, eng.param_version, eng.norm_nontemporal = 640, 0, False
    eng._stream = lambda: 0
    eng.freeze_active = lambda: (object() if frozen else None)
    eng.grad_norm_device = lambda hyper=None: ArenaMixin.grad_norm_device(eng, hyper)
    eng.clip_algorithm, eng.clip_skip_nonfinite, eng.track_grad_norm = None, False, False
    return eng, rec


@pytest.mark.parametrize("frozen", [False, True])
def test_launch_order_of_the_adam_step(frozen):
    from object_detection_cib_amd.engine.arenas import ArenaMixin
    keep = 7 if frozen else None

    def run(algo, track):
        eng, rec = _fake_engine(frozen)
        ArenaMixin.configure_clip(eng, algo, False, track)
        ArenaMixin.adam_step_device(eng)
        assert eng.note_adam_step.call_count == 1 and eng.check_adam_freeze.call_count == 1 and eng.param_version == 1
        return rec.calls

    calls = run(None, False)
    assert [c[0] for c in calls] == ["kodhip_adam_step"]
    assert calls[0][1] == (1, 8, 2, 10, 3, keep, 640, 11, None, -1, 0)
    calls = run(None, True)                                  # track only: the reduction (scale from the ADAM block), the plain update
    assert [c[0] for c in calls] == ["kodhip_grad_norm", "kodhip_adam_step"]
    assert calls[0][1] == (8, 3, 9, 640, 11, 5, 6, 0, 0, 0) and calls[1][1][8:10] == (None, -1)
    calls = run("norm", False)
    assert [c[0] for c in calls] == ["kodhip_grad_norm", "kodhip_adam_step"]
    assert calls[1][1] == (1, 8, 2, 10, 3, keep, 640, 11, 5, 0, 0)
    calls = run("value", False)                              # no reduction needed
    assert [c[0] for c in calls] == ["kodhip_adam_step"] and calls[0][1][8:10] == (5, 1)
    assert [c[0] for c in run("value", True)] == ["kodhip_grad_norm", "kodhip_adam_step"]
    eng, rec = _fake_engine(frozen)
    ArenaMixin.configure_clip(eng, "norm", True, False)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        ArenaMixin.adam_step_device(eng)
    assert rec.calls == []


def test_freeze_set_is_fixed_by_the_first_step():
    from object_detection_cib_amd.engine.arenas import ArenaMixin
    eng = mock.MagicMock()
    plan = SimpleNamespace(frozen=("a", "b"))
    eng.freeze_active = lambda: plan
    eng._frozen_now = lambda: ArenaMixin._frozen_now(eng)
    eng.adam_steps, eng.adam_frozen = 0, None
    ArenaMixin.check_adam_freeze(eng)                        # nothing stepped yet
    ArenaMixin.note_adam_step(eng)
    assert eng.adam_steps == 1 and eng.adam_frozen == frozenset({"a", "b"})
    ArenaMixin.check_adam_freeze(eng)                        # frozen from the start: fine
    plan = SimpleNamespace(frozen=("a",))                    # un-freezing "b" after a step
    with pytest.raises(RuntimeError, match="freeze set"):
        ArenaMixin.check_adam_freeze(eng)
    eng.freeze_active = lambda: None                         # un-freezing everything
    with pytest.raises(RuntimeError, match="freeze set"):
        ArenaMixin.check_adam_freeze(eng)
