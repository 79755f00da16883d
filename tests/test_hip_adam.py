"""Fused Adam / AdamW on the GPU: the kernel against the numpy restatement bit for bit (pin a), FusedAdam.step() against CPU
torch.optim.AdamW (pins b and c, tests/test_adam_reference.py), the captured step against the eager loop, the experiment class
and checkpoint resume (small geometries)."""
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import adam_reference as ar  # noqa: E402
from oracle import synth  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402
from object_detection_cib_amd.core.bbox.iou import IoUCalculator  # noqa: E402
from object_detection_cib_amd.core.label_assignment.yv5 import Yolov5LabelAssigner, AssignmentAnchorInfo  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.data.detection import DetectionTarget  # noqa: E402
from object_detection_cib_amd.engine.arenas import ADAM_HYPER_FLOATS  # noqa: E402
from object_detection_cib_amd.engine.graphed import GraphedTrainStep  # noqa: E402
from object_detection_cib_amd.lightning.checkpoint import load_checkpoint, save_checkpoint  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.loss import Yolov5Loss, Yolov5LossParams  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.warmup import OptimizerWarmupUpdater  # noqa: E402
from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network  # noqa: E402
from object_detection_cib_amd.nn.optim.smart import FusedAdamW, SmartAdamW, SmartOptimizer  # noqa: E402

NC, B, S, SEED = 10, 4, 160, 7
INFOS = (voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
DEV = "cuda:0"


# ------------------------------------------------------------------ 1. the kernel on raw arenas, pin (a)
N = 1088                                           # 17 granules: more than one 1024-element block
GID = np.array([0, 1, 2, 255, 1, 1, 2, 0, 1, 255, 1, 2, 2, 0, 1, 1, 1], dtype=np.uint8)
LR_STEPS = ((2e-3, 1e-3, 5e-4), (1.7e-3, 1.1e-3, 4e-4), (1.3e-3, 9e-4, 3.3e-4))
WD = (0.0, 5e-4, 1e-2)
BETAS, EPS = (0.937, 0.999), 1e-8


def _keep(variant):
    if variant == "none":
        return None
    k = np.ones(N, dtype=np.uint8)
    if variant == "partial":
        k[96:128] = 0                              # granule 1: elements 64..95 kept, 96..127 frozen
        k[4 * 64:5 * 64] = 0                       # granule 4 wholly frozen
    return k


def _same_bits(a, b):
    """bit equality where neither side is a NaN, NaNs at the same places (payloads are not pinned)"""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])


@pytest.mark.parametrize("clip", [None, "norm", "value"])
@pytest.mark.parametrize("keep_variant", ["none", "ones", "partial"])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_kernel_equals_restatement_bit_for_bit(decoupled, keep_variant, clip):
    lib = _lib.lib()
    assert lib.kodhip_adam_hyper_floats() == ADAM_HYPER_FLOATS
    rng = np.random.default_rng(3)
    p = (rng.standard_normal(N) * 0.1).astype(np.float32)
    p[5:9] = 0.0
    p_init = p.copy()
    m, v = np.zeros(N, np.float32), np.zeros(N, np.float32)
    keep = _keep(keep_variant)
    gscale, maximize = 0.25, decoupled             # (maximize on in one of the two forms)
    coef, cv = 0.37, 0.05
    clip_blk = np.zeros(16, np.float32)
    clip_blk[4], clip_blk[8] = coef, cv
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    dp, dm, dv, dgid, dclip = t(p), t(m), t(v), t(GID), t(clip_blk)
    dkeep = None if keep is None else t(keep)
    touched = np.repeat(GID, 64) <= 2
    if keep is not None:
        touched &= keep != 0
    stream = torch.cuda.current_stream().cuda_stream
    for step in range(1, 4):
        # magnitudes (0.1 + |normal|) * 10 ** U(-6, 2): no fp32 denormal arises in g * gscale * coef, (1 - beta2) * g * g, ...
        g = (rng.choice([-1.0, 1.0], N) * (0.1 + np.abs(rng.standard_normal(N))) * 10.0 ** rng.uniform(-6, 2, N)).astype(np.float32)
        g[rng.choice(N, 40, replace=False)] = 0.0  # den = eps (first step)
        g[70], g[300] = np.nan, np.inf             # in kept elements of groups 1 and 1: they must stay their own
        g[20], g[21] = 0.0, -0.0
        consts = [ar.host_constants(LR_STEPS[step - 1][k], *BETAS, EPS, WD[k], step) for k in range(3)]
        hyper = ar.hyper_block(consts, gscale, maximize, decoupled, ADAM_HYPER_FLOATS)
        p0, m0, v0 = p, m, v
        p, m, v = ar.adam_ref_arena(p0, g, m0, v0, GID, keep, consts, gscale=gscale, maximize=maximize, decoupled=decoupled,
                                    clip_mode=clip, coef=coef, clip_value=cv)
        dg, dh = t(g), t(hyper)                     # (held: a temporary's memory would be handed to the next allocation)
        rc = lib.kodhip_adam_step(dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), dgid.data_ptr(),
                                  None if dkeep is None else dkeep.data_ptr(), N, dh.data_ptr(),
                                  None if clip is None else dclip.data_ptr(), {None: -1, "norm": 0, "value": 1}[clip], stream)
        assert rc == 0, lib.kodhip_last_error()
        torch.cuda.synchronize()
        for name, dev, ref, before in (("p", dp, p, p0), ("exp_avg", dm, m, m0), ("exp_avg_sq", dv, v, v0)):
            got = dev.cpu().numpy()
            assert _same_bits(got, ref), (name, step, np.nonzero(got.view(np.int32) != ref.view(np.int32))[0][:8])
            # frozen and padding elements: the bits they had
            assert np.array_equal(got.view(np.int32)[~touched], before.view(np.int32)[~touched]), (name, step)
        # the NaN and the Inf stayed in their own elements
        bad = ~np.isfinite(dp.cpu().numpy())
        assert set(np.nonzero(bad)[0]) <= {70, 300}, np.nonzero(bad)[0]
    moved = dp.cpu().numpy()[touched] != p_init[touched]
    assert moved.mean() > 0.9                      # and the update did something


# ------------------------------------------------------------------ the network
def _loss():
    return Yolov5Loss(Yolov5LabelAssigner(AssignmentAnchorInfo(*INFOS), 4.0), Yolov5LossParams.get_default(),
                      IoUCalculator("ciou", 1e-7), None)


def _net(seed=SEED):
    torch.manual_seed(seed)
    return Yolov5Network(3, NC, widen_factor=0.25, deepen_factor=0.33).to(DEV).train()


def _batch(seed):
    x, _ = synth.batch(B, S, NC, seed)
    tg = synth.targets(B, S, NC, seed, nmin=12, nmax=24)
    return x.to(DEV), tuple(DetectionTarget(b, l) for b, l in tg)


def _eager_step(net, loss, x, tg):
    net.zero_grad(set_to_none=True)
    total, _ = net.train_step(x, loss, FeatureShape(width=S, height=S), tg, float(B))
    return total


def _state(net):
    eng = net.engine()
    torch.cuda.synchronize()
    return eng.p_arena.cpu().clone(), eng.m_arena.cpu().clone(), eng.v_arena.cpu().clone()


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _lrs(step):
    return (1e-3 - 1e-4 * step, 5e-4 + 1e-4 * step, 7e-4)


# ------------------------------------------------------------------ 2. eager FusedAdam.step() against CPU torch
def test_eager_step_against_cpu_torch_adamw():
    """Three steps; before each, the fused optimizer's state_dict() is loaded into a CPU torch.optim.AdamW over clones of the
    parameters (so torch starts every step from the same bits), which is fed the published gradients.  Moments: bit for bit
    (b).  Parameters: within one ulp, at most 1e-4 of the element-steps differing (c).  The parameters are re-drawn with
    magnitudes in [0.25, 1) first, for the reason given at tests/test_adam_reference.py _inputs: an update that cancels its
    parameter would turn a one-ulp difference in torch's CPU sqrt into many ulps of a tiny result.
    The learning rates are ~3e-5: the kernel equals the restatement bit for bit (pin a), so every difference counted here is
    one between the restatement and CPU torch, and those come from torch's CPU sqrt over a large tensor, which is off by one
    ulp in a share of the elements that depends on the host (0.7 % on one, more on another).  Such a difference reaches the
    parameter with probability ~|update| / |parameter|.  Measured on an MI355X host with lr ~1e-3: 806 of 5 332 341 element-
    steps (1.5e-4, all one ulp, moments bit-equal), where the same arithmetic gave 1.4e-5 on another host; the cap is a
    condition on the inputs, so the inputs keep |update| / |parameter| near 1e-4."""
    loss = _loss()
    net = _net()
    eng = net.engine()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for p in net.parameters():
            sign = torch.randint(0, 2, p.shape, generator=g).float() * 2 - 1
            p.copy_((sign * (0.25 + 0.75 * torch.rand(p.shape, generator=g))).to(DEV))
    eng.mark_params_changed()
    opt = SmartOptimizer(partial(torch.optim.AdamW, lr=1e-3, betas=(0.937, 0.999)), 5e-4)(net)
    assert type(opt) is FusedAdamW
    names = {id(p): n for n, p in net.named_parameters()}
    differ = worst = total_elems = 0
    where = []
    for step in range(3):
        for pg, lr in zip(opt.param_groups, _lrs(step)):
            pg["lr"] = 0.03 * lr                   # (see the docstring)
        total = _eager_step(net, loss, *_batch(SEED + step))
        assert torch.isfinite(total)
        cpu = {n: torch.nn.Parameter(p.detach().cpu().clone()) for n, p in net.named_parameters()}
        for n, p in net.named_parameters():
            cpu[n].grad = p.grad.detach().cpu().clone()
            assert torch.isfinite(cpu[n].grad).all(), n
        ref = torch.optim.AdamW([dict(params=[cpu[names[id(p)]] for p in pg["params"]]) for pg in opt.param_groups], foreach=False)
        sd = opt.state_dict()
        assert len(sd["state"]) == (0 if step == 0 else len(cpu))
        ref.load_state_dict(sd)
        for pg in ref.param_groups:
            pg["foreach"] = False
        ref.step()
        opt.step()
        torch.cuda.synchronize()
        for n, p in net.named_parameters():
            o, k = eng.layout[n]
            st = ref.state[cpu[n]]
            assert float(st["step"]) == step + 1
            assert torch.equal(eng.m_arena[o:o + k].cpu().view(torch.int32), st["exp_avg"].reshape(-1).view(torch.int32)), (step, n)
            assert torch.equal(eng.v_arena[o:o + k].cpu().view(torch.int32), st["exp_avg_sq"].reshape(-1).view(torch.int32)), (step, n)
            d = ar.ulp_distance(p.detach().cpu().numpy().reshape(-1), cpu[n].detach().numpy().reshape(-1))
            differ += int((d != 0).sum())
            worst = max(worst, int(d.max()))
            total_elems += k
            if (d != 0).any():
                where.append((int((d != 0).sum()), step, n, k, float(cpu[n].grad.abs().median())))
    for row in sorted(where, reverse=True)[:6]:
        print("  differing elements, step, tensor, numel, median |grad|:", row)
    print(f"parameters: {differ} of {total_elems} element-steps differ from CPU torch, worst {worst} ulp")
    assert worst <= 1
    assert differ <= 1e-4 * total_elems


# ------------------------------------------------------------------ 3. captured against eager
def test_captured_adam_step_equals_eager_loop():
    """One eager step (so that the moments are not zero at capture), then four batches: GraphedTrainStep(optimizer="adam") with
    the lr changing between replays and clipping by norm == the eager loop (FusedAdam.step() with the same clip value) bit for
    bit: losses, parameters, both moments.  capture() leaves parameters and moments untouched; changing `optimizer` after
    capture raises."""
    loss = _loss()
    batches = [_batch(SEED + k) for k in range(5)]
    net = _net()                                   # the unclipped norm of the first batch sets the scale of the clip value
    _eager_step(net, loss, *batches[0])
    c = 0.5 * float(torch.linalg.vector_norm(torch.cat([p.grad.double().flatten() for p in net.parameters()])))
    runs = {}
    for graphed in (False, True):
        net = _net()
        opt = SmartAdamW(net, lr=1e-3, betas=(0.937, 0.999), weight_decay=5e-4)
        eng = net.engine()
        opt.gradient_clip_val = c
        losses = []
        for step, (x, tg) in enumerate(batches):
            for pg, lr in zip(opt.param_groups, _lrs(step)):
                pg["lr"] = lr
            if graphed and step == 1:
                before = _state(net)
                gs = GraphedTrainStep(net, loss, B, S, S, max_targets=256, gradient_clip_val=c, optimizer="adam").capture(x, tg)
                assert _bits_equal(_state(net), before) and eng.adam_steps == 1
            if graphed and step >= 1:
                total, _ = gs(x, tg, grad_scale=1.0, gradient_clip_val=c, adam=opt.hyper())
                opt.steps_taken += 1
            else:
                total = _eager_step(net, loss, x, tg)
                opt.step()
            losses.append(float(total))
        runs[graphed] = (losses, _state(net), eng.clip[0].item())
        if graphed:
            with pytest.raises(ValueError, match="adam="):
                gs(x, tg, (0.1,) * 3, (0.9,) * 3, (0.0,) * 3, 1.0)
            gs.optimizer = "sgd"
            with pytest.raises(RuntimeError, match="after capture"):
                gs(x, tg, (0.1,) * 3, (0.9,) * 3, (0.0,) * 3, 1.0)
    print("losses", runs[True][0], "last grad norm", runs[True][2])
    assert np.isfinite(runs[False][0]).all()
    assert runs[True][0] == runs[False][0], (runs[True][0], runs[False][0])
    assert _bits_equal(runs[True][1], runs[False][1])
    assert runs[True][2] == runs[False][2] and runs[True][2] > c            # the clipping was active on the last step


# ------------------------------------------------------------------ 4. the experiment
def _experiment(seed=SEED, **kw):
    return DefaultYolov5Experiment(_net(seed), _loss(), LayerwiseAnchorInfo(*INFOS),
                                   smart_optimizer=SmartOptimizer(partial(torch.optim.AdamW, lr=1e-3), 5e-4),
                                   optimizer_warmup_updater=OptimizerWarmupUpdater(3, 0.1, 0.8, 0.937), **kw)


def test_experiment_graphed_equals_eager_with_ema_and_warmup():
    """SmartOptimizer(partial(torch.optim.AdamW, lr=1e-3), 5e-4) with graphed=True (an AttributeError before FusedAdam) trains
    three steps and equals graphed=False bit for bit, the EMA behind the step and a warm-up updater included."""
    batches = [_batch(SEED + k) for k in range(3)]

    def loop(graphed):
        exp = _experiment(graphed=graphed, max_targets=256, ema=True)
        losses = [exp.optimize((x, tg, None), 8).item() for x, tg in batches]
        assert type(exp.optimizer) is FusedAdamW and exp.optimizer.steps_taken == 3
        torch.cuda.synchronize()
        return losses, _state(exp.net), {k: t.detach().cpu().clone() for k, t in exp.ema.state_dict().items()}

    eager, graph = loop(False), loop(True)
    assert np.isfinite(eager[0]).all()
    assert graph[0] == eager[0], (graph[0], eager[0])
    assert _bits_equal(graph[1], eager[1])
    assert all(torch.equal(graph[2][k], eager[2][k]) for k in eager[2])
    assert float(eager[1][2].abs().sum()) > 0


def test_experiment_multi_scale_runs_two_sizes():
    exp = _experiment(graphed=True, max_targets=256, multi_scale=True, multi_scale_range=(0.8, 1.0))
    sizes = set()
    for k in range(6):
        x, tg = _batch(SEED + k)
        assert np.isfinite(exp.optimize((x, tg, None), 8).item())
        sizes.add(exp._gstep.size)
        if len(sizes) >= 2 and k >= 2:
            break
    assert len(sizes) >= 2, sizes
    assert exp.optimizer.steps_taken == k + 1 and exp.net.engine().adam_steps == k + 1


# ------------------------------------------------------------------ 5. resume
def test_resume_equals_straight_run(tmp_path):
    loss = _loss()
    batches = [_batch(SEED + k) for k in range(5)]

    def steps(net, opt, ks):
        for k in ks:
            for pg, lr in zip(opt.param_groups, _lrs(k)):
                pg["lr"] = lr
            _eager_step(net, loss, *batches[k])
            opt.step()

    net = _net()
    opt = SmartAdamW(net, lr=1e-3, betas=(0.937, 0.999), weight_decay=5e-4)
    steps(net, opt, range(5))
    straight = _state(net)
    net = _net()
    opt = SmartAdamW(net, lr=1e-3, betas=(0.937, 0.999), weight_decay=5e-4)
    steps(net, opt, range(3))
    path = str(tmp_path / "adam.ckpt")
    ckpt = save_checkpoint(path, net, opt, epoch=0, global_step=3)
    st = ckpt["optimizer_states"][0]["state"]
    assert len(st) == len(list(net.parameters())) and set(st[0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert st[0]["step"].dtype == torch.float32 and float(st[0]["step"]) == 3.0
    net2 = _net(SEED + 100)                        # other weights: everything must come from the file
    opt2 = SmartAdamW(net2, lr=1e-3, betas=(0.937, 0.999), weight_decay=5e-4)
    load_checkpoint(path, net2, opt2)
    assert opt2.steps_taken == 3 and opt2.hyper()["step"] == 4
    # the running BatchNorm statistics travel in the network's state dict
    steps(net2, opt2, range(3, 5))
    assert _bits_equal(_state(net2), straight)
    # a plain torch.optim.AdamW over a torch copy of the parameters loads the same dict
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for pg in opt.param_groups for p in pg["params"]]
    sizes = [len(pg["params"]) for pg in opt.param_groups]
    ref = torch.optim.AdamW([dict(params=cpu[:sizes[0]]), dict(params=cpu[sizes[0]:sizes[0] + sizes[1]]),
                             dict(params=cpu[sizes[0] + sizes[1]:])])
    ref.load_state_dict(ckpt["optimizer_states"][0])
    assert float(ref.state[cpu[0]]["step"]) == 3.0


def test_frozen_from_the_start_and_unfreezing_after_a_step():
    loss = _loss()
    net = _net()
    net.backbone.requires_grad_(False)
    opt = SmartAdamW(net, lr=1e-3)
    frozen_before = {n: p.detach().clone() for n, p in net.named_parameters() if not p.requires_grad}
    _eager_step(net, loss, *_batch(SEED))
    opt.step()
    _eager_step(net, loss, *_batch(SEED + 1))
    opt.step()                                     # the same freeze set: fine
    torch.cuda.synchronize()
    for n, p in net.named_parameters():
        if n in frozen_before:
            assert torch.equal(p.detach(), frozen_before[n]), n
    sd = opt.state_dict()
    flat = [p for pg in opt.param_groups for p in pg["params"]]
    assert len(frozen_before) > 0
    assert set(sd["state"]) == {i for i, p in enumerate(flat) if p.requires_grad}       # no state for the frozen tensors
    eng = net.engine()
    for n in frozen_before:                        # nor moments in the arenas
        o, k = eng.layout[n]
        assert not eng.m_arena[o:o + k].any() and not eng.v_arena[o:o + k].any()
    net.backbone.requires_grad_(True)
    _eager_step(net, loss, *_batch(SEED + 2))
    before = _state(net)
    with pytest.raises(RuntimeError, match="freeze set"):
        opt.step()
    assert _bits_equal(_state(net), before)        # refused before the launch
