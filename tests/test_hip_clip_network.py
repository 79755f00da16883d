"""Gradient clipping through the network, the captured step, FusedSGD and the experiment class (small geometries).
Norm yardstick and its 1-ulp bar: see tests/test_hip_clip.py."""
import random
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import synth  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402
from object_detection_cib_amd.core.bbox.iou import IoUCalculator  # noqa: E402
from object_detection_cib_amd.core.label_assignment.yv5 import Yolov5LabelAssigner, AssignmentAnchorInfo  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.data.detection import DetectionTarget  # noqa: E402
from object_detection_cib_amd.data.device_pipeline import DeviceTrainPipeline  # noqa: E402
from object_detection_cib_amd.engine.graphed import GraphedTrainStep  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.loss import Yolov5Loss, Yolov5LossParams  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.warmup import OptimizerWarmupUpdater  # noqa: E402
from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network  # noqa: E402
from object_detection_cib_amd.nn.optim.smart import SmartSGD  # noqa: E402

from test_hip_clip import ulps  # noqa: E402

NC, B, S, SEED = 10, 4, 160, 7
INFOS = (voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))


def _loss():
    return Yolov5Loss(Yolov5LabelAssigner(AssignmentAnchorInfo(*INFOS), 4.0), Yolov5LossParams.get_default(),
                      IoUCalculator("ciou", 1e-7), None)


def _net(seed=SEED):
    torch.manual_seed(seed)
    return Yolov5Network(3, NC, widen_factor=0.25, deepen_factor=0.33).to("cuda:0").train()


def _batch(seed):
    x, _ = synth.batch(B, S, NC, seed)
    tg = synth.targets(B, S, NC, seed, nmin=12, nmax=24)          # (enough boxes that every level gets matches: no NaN level)
    return x.to("cuda:0"), tuple(DetectionTarget(b, l) for b, l in tg)


def _fp64_norm(grads):
    return torch.linalg.vector_norm(torch.cat([g.double().flatten() for g in grads if g is not None]))


def _params(net):
    return torch.cat([p.detach().flatten() for p in net.parameters()]).cpu()


def _eager_step(net, loss, x, tg):
    net.zero_grad(set_to_none=True)
    total, _ = net.train_step(x, loss, FeatureShape(width=S, height=S), tg, float(B))
    return total


@pytest.mark.parametrize("frozen", [False, True])
def test_eager_clip_grad_norm(frozen):
    """train_step -> net.clip_grad_norm_(c): the returned norm is the fp64 norm of the .grad views taken before the call
    (1 ulp), .grad afterwards = before x coef; c = 0.5 x the norm clips, c = 10 x the norm leaves the step's parameters
    bit-identical to an unclipped step.  frozen: parameters without .grad do not count."""
    loss = _loss()
    x, tg = _batch(SEED)
    results = {}
    for factor in (None, 0.5, 10.0):
        net = _net()
        if frozen:
            net.backbone.requires_grad_(False)
        opt = SmartSGD(net, lr=0.05, momentum=0.9)
        _eager_step(net, loss, x, tg)
        before = [None if p.grad is None else p.grad.detach().clone() for p in net.parameters()]
        assert any(g is None for g in before) == frozen
        ref = _fp64_norm(before)
        if factor is not None:
            c = factor * float(ref)
            # arena padding (and the frozen tensors' slots) must not count: fill them with 1e30 first
            eng = net.engine()
            dead = ~eng._count_mask().bool()
            assert int(dead.sum()) > 0
            eng.current_grad_arena()[dead] = 1e30
            got = net.clip_grad_norm_(c)
            assert got.is_cuda and got.dim() == 0
            d = ulps(got, ref)
            print(f"frozen={frozen} factor={factor}: norm {float(got):.9g}, fp64 {float(ref):.9g}, {d} ulp")
            assert d <= 1
            coef = net.engine().clip[4].clone()
            want = torch.clamp(c / (got + 1e-6), max=1.0)                  # torch's own formation, in fp32
            assert abs(float(coef) - float(want)) <= 2.0 ** -22 * float(want)      # (a reciprocal and a product, 1 ulp each)
            assert (float(coef) < 0.51) == (factor < 1) and (factor < 1 or float(coef) == 1.0)
            for p, g0 in zip(net.parameters(), before):
                assert (p.grad is None) == (g0 is None)
                if g0 is not None:
                    assert torch.equal(p.grad, g0 * coef)
        opt.step()
        torch.cuda.synchronize()
        results[factor] = _params(net)
    assert torch.equal(results[10.0], results[None])
    assert not torch.equal(results[0.5], results[None])


def test_eager_clip_grad_value():
    loss = _loss()
    x, tg = _batch(SEED)
    net = _net()
    _eager_step(net, loss, x, tg)
    before = [p.grad.detach().clone() for p in net.parameters()]
    v = float(torch.cat([g.abs().flatten() for g in before]).quantile(0.9))
    net.clip_grad_value_(v)
    for p, g0 in zip(net.parameters(), before):
        assert torch.equal(p.grad, g0.clamp(-v, v))


def _schedule(step):
    """a warm-up-like schedule and a clip value that move every step"""
    lr = (0.1 - 0.01 * step, 0.002 * (step + 1), 0.002 * (step + 1))
    mom = (0.8 + 0.01 * step,) * 3
    return lr, mom, (0.0, 5e-4, 0.0)


@pytest.mark.parametrize("frozen", [False, True])
def test_graphed_clipped_step_equals_eager_loop(frozen):
    """GraphedTrainStep(gradient_clip_val=c) over several batches, schedule and c changing between replays == the eager loop
    (net.clip_grad_norm_ + FusedSGD.step) bit for bit: losses, parameters and grad_norm; frozen: the masked forms.
    Changing the algorithm (or switching clipping off) after capture raises."""
    loss = _loss()
    batches = [_batch(SEED + k) for k in range(5)]
    # the unclipped norm of the first batch sets the scale of c
    net = _net()
    if frozen:
        net.backbone.requires_grad_(False)
    _eager_step(net, loss, *batches[0])
    base = float(_fp64_norm([p.grad for p in net.parameters()]))
    cs = [0.5 * base, 0.2 * base, 100.0 * base, 0.1 * base, 0.3 * base]
    runs = {}
    for graphed in (False, True):
        net = _net()
        if frozen:
            net.backbone.requires_grad_(False)
        opt = SmartSGD(net, lr=0.01, momentum=0.9)
        eng = net.engine()
        losses, norms = [], []
        if graphed:
            gs = GraphedTrainStep(net, loss, B, S, S, max_targets=256, gradient_clip_val=cs[0]).capture(*batches[0])
            assert gs.skipped_steps.item() == 0.0
        for step, (x, tg) in enumerate(batches):
            lr, mom, wd = _schedule(step)
            if graphed:
                total, _ = gs(x, tg, lr, mom, wd, 1.0, gradient_clip_val=cs[step])
                norms.append(gs.grad_norm.clone())
            else:
                for pg, a, m in zip(opt.param_groups, lr, mom):
                    pg["lr"], pg["momentum"] = a, m
                total = _eager_step(net, loss, x, tg)
                net.clip_grad_norm_(cs[step])
                norms.append(eng.clip[0:4].clone())
                opt.step()
            losses.append(total.clone())
        torch.cuda.synchronize()
        runs[graphed] = ([float(t) for t in losses], _params(net), torch.stack(norms).cpu(), eng.m_arena.cpu().clone())
        if graphed:
            with pytest.raises(RuntimeError, match="after capture"):
                gs(x, tg, lr, mom, wd, 1.0, gradient_clip_algorithm="value")
            gs.gradient_clip_algorithm = "norm"
            with pytest.raises(RuntimeError, match="after capture"):
                gs(x, tg, lr, mom, wd, 1.0, gradient_clip_val=None)
    print("losses", runs[True][0], "total norms", runs[True][2][:, 0].tolist(), "clip values", cs)
    assert np.isfinite(runs[False][0]).all()
    assert runs[True][0] == runs[False][0], (runs[True][0], runs[False][0])
    assert torch.equal(runs[True][2].view(torch.int32), runs[False][2].view(torch.int32))
    assert torch.equal(runs[True][1], runs[False][1])
    assert torch.equal(runs[True][3], runs[False][3])
    total = runs[True][2][:, 0]
    active = [float(t) > c for t, c in zip(total, cs)]
    assert active[0] and not active[2] and sum(active) >= 3, active       # clipped and unclipped replays of ONE graph
    parts = runs[True][2][:, 1:].double()
    assert torch.allclose(parts.pow(2).sum(1).sqrt(), total.double(), rtol=1e-6)       # bias / decay / norm groups add up


def test_track_grad_norm_and_skip_nonfinite_in_the_captured_step():
    """track_grad_norm=True without a clip value: the reduction runs, the update is the unclipped one (same parameters as a
    plain captured step).  skip_nonfinite: a batch of NaN pixels leaves parameters and momentum untouched and is counted."""
    loss = _loss()
    batches = [_batch(SEED + k) for k in range(3)]
    runs = {}
    for track in (False, True):
        net = _net()
        SmartSGD(net, lr=0.01, momentum=0.9)
        gs = GraphedTrainStep(net, loss, B, S, S, max_targets=256, track_grad_norm=track).capture(*batches[0])
        norms = []
        for step, (x, tg) in enumerate(batches):
            gs(x, tg, *_schedule(step), 1.0)
            norms.append(gs.grad_norm[0].clone())
        torch.cuda.synchronize()
        runs[track] = (_params(net), [float(t) for t in norms])
    assert torch.equal(runs[True][0], runs[False][0])
    assert all(np.isfinite(t) and t > 0 for t in runs[True][1]) and runs[False][1] == [0.0] * 3
    net = _net()
    eng = net.engine()
    gs = GraphedTrainStep(net, loss, B, S, S, max_targets=256, gradient_clip_val=1.0, skip_nonfinite=True).capture(*batches[0])
    gs(*batches[0], *_schedule(0), 1.0)
    p1, m1 = eng.p_arena.clone(), eng.m_arena.clone()
    assert gs.skipped_steps.item() == 0.0
    gs(torch.full_like(batches[1][0], float("nan")), batches[1][1], *_schedule(1), 1.0)
    assert gs.skipped_steps.item() == 1.0 and not np.isfinite(gs.grad_norm[0].item())
    assert torch.equal(eng.p_arena.view(torch.int32), p1.view(torch.int32))
    assert torch.equal(eng.m_arena.view(torch.int32), m1.view(torch.int32))


def test_fused_sgd_clipping_vs_torch_clip_grad_norm_and_sgd():
    """The eager HIP loop (FusedSGD(gradient_clip_val=c).step()) against torch.nn.utils.clip_grad_norm_ + torch.optim.SGD on
    CPU clones of the same parameters and gradients, at test_frozen_backbone_vs_fp32_oracle_and_torch_sgd's torch-SGD
    tolerance (rtol 1e-6, atol 1e-7), the atol widened only by what torch's own fp32 norm is off: the coefficient's relative
    error (torch's norm vs the fp64 norm, measured here, plus the kernel's 1 ulp) times the largest update.
    Measured on MI355X (yv5n, 1.8 M gradient elements): torch's fp32 norm 3.90316319 against the fp64 norm 3.90316415, a
    relative deviation of 2.44e-7 (4 ulp), where the HIP norm is 0 ulp away; largest update 5.25e-3, so the atol is widened by
    1.9e-9 (the line printed below repeats the measurement on every run)."""
    loss = _loss()
    x, tg = _batch(SEED)
    net = _net()
    opt = SmartSGD(net, lr=0.05, momentum=0.9)
    _eager_step(net, loss, x, tg)
    before = {n: p.detach().cpu().clone() for n, p in net.named_parameters()}
    grads = {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters()}
    ref = _fp64_norm(grads.values())
    c = 0.5 * float(ref)
    cpu = {n: torch.nn.Parameter(before[n].clone()) for n in before}
    for n in cpu:
        cpu[n].grad = grads[n].clone()
    by_id = {id(p): n for n, p in net.named_parameters()}
    opt_c = torch.optim.SGD([dict(params=[cpu[by_id[id(p)]] for p in g["params"]], lr=g["lr"], momentum=g["momentum"],
                                  weight_decay=g["weight_decay"], nesterov=True) for g in opt.param_groups])
    torch_norm = torch.nn.utils.clip_grad_norm_(list(cpu.values()), c)
    opt_c.step()
    opt.gradient_clip_val = c
    opt.step()
    torch.cuda.synchronize()
    got_norm = net.engine().clip[0].cpu()
    assert ulps(got_norm, ref) <= 1
    dev = abs(float(torch_norm.double()) - float(ref)) / float(ref) + 2.0 ** -23
    step_max = max(float((cpu[n].detach() - before[n]).abs().max()) for n in cpu)
    print(f"torch fp32 norm {float(torch_norm):.9g} vs fp64 {float(ref):.9g}: relative deviation {dev - 2.0 ** -23:.3g} "
          f"({ulps(torch_norm, ref)} ulp); largest update {step_max:.3g}; atol widened by {dev * step_max:.3g}")
    for n, p in net.named_parameters():
        torch.testing.assert_close(p.detach().cpu(), cpu[n].detach(), rtol=1e-6, atol=1e-7 + dev * step_max, msg=n)
        assert not torch.equal(p.detach().cpu(), before[n]), n


def _experiment(seed, **kw):
    net = _net(seed)
    return DefaultYolov5Experiment(net, _loss(), LayerwiseAnchorInfo(*INFOS),
                                   optimizer_warmup_updater=OptimizerWarmupUpdater(3, 0.1, 0.8, 0.937), **kw)


@pytest.mark.parametrize("algorithm", ["norm", "value"])
def test_experiment_graphed_equals_eager_with_clipping(algorithm):
    """DefaultYolov5Experiment(graphed=True, gradient_clip_val=c) == graphed=False with the same value, bit for bit: losses,
    parameters and the grad_norm metric (in the style of test_graphed_training_loop_equals_eager_loop)."""
    S2, B2, steps, seed = 160, 8, 6, 4
    cache = synth.coco_zipf_like(64, S2, seed, NC)

    def loop(graphed, c):
        pipe = DeviceTrainPipeline([k[0] for k in cache], [k[1] for k in cache], [k[2] for k in cache], S2, "cuda")
        random.seed(seed); np.random.seed(seed)
        exp = _experiment(seed, graphed=graphed, max_targets=512, gradient_clip_val=c, gradient_clip_algorithm=algorithm)
        assert exp.get_metrics_to_display() == ["box", "cls", "obj", "grad_norm"]
        losses, norms = [], []
        for step in range(steps):
            idx = [(step * B2 + k) % len(cache) for k in range(B2)]
            img, _, targets = pipe.make_batch(idx)
            losses.append(exp.optimize((img, targets, None), 8).item())
            assert exp.logged["grad_norm"].is_cuda
            norms.append(exp.logged["grad_norm"].item())
        torch.cuda.synchronize()
        return losses, _params(exp.net), norms

    # a first eager run with a clip value that never bites measures the norms; c = half their smallest (norm) or 1e-4 of it
    # (value: below the gradients' root mean square, norm / sqrt(1.8 M) = 7e-4 of the norm, so the clamp bites)
    _, unclipped, norms = loop(False, 1e30)
    c = (0.5 if algorithm == "norm" else 1e-4) * min(norms)
    eager = loop(False, c)
    graph = loop(True, c)
    print(algorithm, "c =", c, "grad norms", eager[2])
    assert np.isfinite(eager[0]).all()
    assert graph[0] == eager[0], (graph[0], eager[0])
    assert graph[2] == eager[2], (graph[2], eager[2])
    assert torch.equal(graph[1], eager[1])
    assert not torch.equal(eager[1], unclipped)            # the clipping was active
