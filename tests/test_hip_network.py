"""GPU parity of the whole HIP train step (network fwd, loss, bwd, SGD) against the CPU oracle, which is
pinned to the reference by tests/test_oracle_golden.py.

Tolerances (north star: "to a stated fp tolerance"): the HIP path stores activations / activation
gradients in bf16 and accumulates in fp32; SURVEY.md B.7 measured the reference's own fp32-vs-bf16-autocast
sensitivity at loss 1.4e-3 and grad-norm 2.4e-2 relative.  Bars:
* B=2 cases (BASELINE configs[0] shape): losses <= 1e-2 rel at 640 px (2e-2 / 3e-2 at 160 / 64 px), global gradient
  norm <= 1e-1 rel - train-mode BatchNorm over 2 images amplifies bf16 rounding ~2x per layer;
* B=16 at 640 px, where every BatchNorm sees >= 6400 samples per channel (test_train_step_well_conditioned_batch):
  losses <= 1e-2 rel, global gradient norm <= 5e-2 rel; per-tensor gradient cosine held to the fp32 oracle's own
  sensitivity to bf16 storage (cos(HIP, fp32) >= cos(bf16-emulated oracle, fp32) - 0.15; 0.98 is measured to be out of
  reach of bf16 storage itself, see that test);
* every layer in situ (teacher-forced, no amplification): <= 4e-3 .. 2e-2 relL2, also at B=64 / 640 px.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detection as D, synth  # noqa: E402
from oracle.network import OracleYolov5  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402
from object_detection_cib_amd.core.bbox.iou import IoUCalculator  # noqa: E402
from object_detection_cib_amd.core.label_assignment.yv5 import Yolov5LabelAssigner, AssignmentAnchorInfo  # noqa: E402
from object_detection_cib_amd.data.detection import DetectionTarget  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.loss import Yolov5Loss, Yolov5LossParams  # noqa: E402
from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network  # noqa: E402


def _loss():
    asg = Yolov5LabelAssigner(AssignmentAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32)), 4.0)
    return Yolov5Loss(asg, Yolov5LossParams.get_default(), IoUCalculator("ciou", 1e-7), None)


def _step(net, x, tg, size, B):
    res = net(x)
    lr = _loss()(FeatureShape(width=size, height=size), res, tuple(DetectionTarget(b, l) for b, l in tg))
    total = B * (lr.localization + lr.classification + lr.objectness)
    total.backward()
    return res, lr, total


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("case", ["yv5n_64", "yv5s_160", "yv5s_640", "yv5s_416"])
def test_train_step_vs_oracle(case):
    """End to end against the fp32 oracle (pinned to the reference) and its bf16-storage emulation.

    A random-init network in train-mode BN at B=2 amplifies any perturbation layer by layer (measured:
    HIP vs the emulation agree to 2e-5 after the stem and drift x2 per layer, tools/debug_layers.py), so the
    end-to-end bars are the north-star ones (loss / gradient norm) and every layer is checked tightly in
    situ by test_layers_teacher_forced below.  yv5s_416 = the reference's default geometry (kod/configs/data/default.yaml:10,
    every number in BASELINE.md): 52 / 26 / 13 maps - 13 x 13 at stride 32, pixel counts that are no multiple of any tile.
    """
    from oracle import bf16_emul
    widen, deepen, nc, B, size, seed = synth.network_cases()[case]
    torch.manual_seed(seed)
    ref = OracleYolov5(3, nc, widen, deepen).train()
    torch.manual_seed(seed)
    emu = bf16_emul.emulate(OracleYolov5(3, nc, widen, deepen).train())
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen)
    assert list(net.state_dict().keys()) == list(ref.state_dict().keys())
    for (k, a), b in zip(net.state_dict().items(), ref.state_dict().values()):
        assert torch.equal(a, b), k
    net = net.cuda().train()
    x, tg = synth.batch(B, size, nc, seed)
    res = {}
    for name, m in (("ref", ref), ("emu", emu)):
        out = m(x)
        lr = D.yolo_loss(size, size, out, [D.Target(b, l) for b, l in tg])
        tot = D.train_step_total(lr, B)
        tot.backward()
        res[name] = (lr, tot, torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters())).item())
    out_h, lr_h, tot_h = _step(net, x.cuda(), tg, size, B)
    got = np.array([lr_h.localization.item(), lr_h.objectness.item(), lr_h.classification.item(), tot_h.item()])
    gn_h = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in net.parameters())).item()
    for name, ltol, gtol in (("ref", 1e-2, 1e-1), ("emu", 1e-2, 1e-1)):
        lr_r, tot_r, gn_r = res[name]
        want = np.array([lr_r.localization.item(), lr_r.objectness.item(), lr_r.classification.item(), tot_r.item()])
        if np.isfinite(want[3]):
            # north-star bar (1e-2) at the benchmark resolution; the B=2 low-resolution cases have <= 50 samples per
            # channel in the deepest BatchNorms, where bf16 rounding noise is amplified ~2x per layer
            np.testing.assert_allclose(got, want, rtol=ltol if size >= 416 else (2e-2 if size >= 160 else 3e-2), err_msg=name)
            if size >= 160:          # 64 px: the hl map is 2x2 (8 samples per BN channel), pure chaos
                # 160 px / B=2 (50 samples per channel in the deepest BatchNorms): the HIP gradient norm itself moves by
                # 8 % between summation-order variants of its own kernels (measured on yv5s_160 with tools/gn_probe.py:
                # 16.28 .. 17.56 over ten variants; fp32 oracle 16.10, its bf16 emulation 15.67) - 15 % there, the
                # north-star 10 % at the benchmark resolution
                assert abs(gn_h - gn_r) <= (gtol if size >= 416 else 1.5 * gtol) * gn_r, (name, gn_h, gn_r)
    # BN running statistics follow torch semantics (momentum .03, unbiased variance); compared network-wide
    sd_r, sd_h = ref.state_dict(), net.state_dict()
    for suffix, tol in (("running_mean", 0.15), ("running_var", 2e-2)):
        a = torch.cat([sd_h[k].cpu().flatten() for k in sd_r if k.endswith(suffix)])
        b = torch.cat([sd_r[k].flatten() for k in sd_r if k.endswith(suffix)])
        if size >= 160:
            assert _rel(a, b) <= tol, (suffix, _rel(a, b))
    assert all(int(sd_h[k]) == int(sd_r[k]) == 1 for k in sd_r if k.endswith("num_batches_tracked"))


def test_class_count_limit_80_trains_81_is_refused_at_construction():
    """The shipped 80-class head (3 * 85 = 255 -> 256 channels) sits exactly on the limit of the head kernels: a whole
    train step runs and agrees with the fp32 oracle.  81 classes would pass the forward pass and the loss and fail in
    the backward pass (kodhip_head_bwd_prep: "bad Npad"); the engine refuses them when it is built instead."""
    widen, deepen, nc, B, size, seed = 0.25, 0.33, 80, 2, 160, 2023
    torch.manual_seed(seed)
    ref = OracleYolov5(3, nc, widen, deepen).train()
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen).cuda().train()
    x, tg = synth.batch(B, size, nc, seed)
    lr_r = D.yolo_loss(size, size, ref(x), [D.Target(b, l) for b, l in tg])
    tot_r = D.train_step_total(lr_r, B)
    tot_r.backward()
    _, lr_h, tot_h = _step(net, x.cuda(), tg, size, B)
    assert np.isfinite(tot_r.item())
    np.testing.assert_allclose(tot_h.item(), tot_r.item(), rtol=2e-2)
    gn_r = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ref.parameters())).item()
    gn_h = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in net.parameters())).item()
    assert abs(gn_h - gn_r) <= 0.15 * gn_r, (gn_h, gn_r)
    # the class heads' bias gradients come out of head_bwd_prep's column sums at Npad = 256
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    bad = Yolov5Network(3, 81, widen_factor=widen, deepen_factor=deepen)
    with pytest.raises(ValueError, match="at most 80 classes with 3 anchors"):
        bad.cuda().train()(x.cuda())


@pytest.mark.parametrize("act", ["leaky", "hardswish"])
def test_train_step_with_another_activation(act):
    """Yolov5Network(activation_layer=...) other than the reference's SiLUInplace (kod/nn/networks/yolov5.py:40-50 takes any
    callable): the whole train step - stem included, whose fused SiLU backward and the data gradients' fused reduction are
    switched off for such a network - against the fp32 oracle with the same activation in every conv unit: losses to 3e-2,
    global gradient norm to 2e-1 (kinked activations are more sensitive to bf16 storage, tests/test_hip_modules.py)."""
    make = {"leaky": lambda: torch.nn.LeakyReLU(0.1), "hardswish": torch.nn.Hardswish}[act]
    widen, deepen, nc, B, size, seed = 0.25, 0.33, 10, 4, 160, 77
    torch.manual_seed(seed)
    ref = OracleYolov5(3, nc, widen, deepen).train()
    for parent in list(ref.modules()):
        for name, child in list(parent.named_children()):
            if isinstance(child, torch.nn.SiLU):
                setattr(parent, name, make())
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, activation_layer=make, widen_factor=widen, deepen_factor=deepen).cuda().train()
    eng = net.engine()
    assert eng.act_kind in (2, 3) and not eng.opt.bn_reduce_fused and not eng.opt.stem_bwd_fused
    x, tg = synth.batch(B, size, nc, seed)
    lr = D.yolo_loss(size, size, ref(x), [D.Target(b, l) for b, l in tg])
    tot = D.train_step_total(lr, B)
    tot.backward()
    _, lr_h, tot_h = _step(net, x.cuda(), tg, size, B)
    got = np.array([lr_h.localization.item(), lr_h.objectness.item(), lr_h.classification.item(), tot_h.item()])
    want = np.array([lr.localization.item(), lr.objectness.item(), lr.classification.item(), tot.item()])
    np.testing.assert_allclose(got, want, rtol=3e-2)
    gn_r = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ref.parameters())).item()
    gn_h = torch.sqrt(sum((p.grad.detach().cpu().double() ** 2).sum() for p in net.parameters())).item()
    assert abs(gn_h - gn_r) <= 2e-1 * gn_r, (gn_h, gn_r)


def test_batchnorm_eps_and_momentum_follow_norm_layer():
    """`norm_layer` may build any nn.BatchNorm2d (kod/nn/networks/yolov5.py:47, kod/nn/layers/csp.py:16-46 take a callable): eps
    and momentum reach the kernels as arguments.  torch's defaults (eps 1e-5, momentum 0.1) instead of the reference's (1e-3,
    .03), one train step at 160 px / B=4 against the fp32 oracle with its BatchNorm modules set the same: losses, gradient
    norm, running statistics (their update IS the momentum), then an eval-mode forward (the folded scale uses eps).  Other
    normalisations and activations stay refused."""
    from functools import partial
    import torch.nn as nn
    widen, deepen, nc, B, size, seed = 0.5, 0.33, 10, 4, 160, 77
    eps, mom = 1e-5, 0.1
    torch.manual_seed(seed)
    ref = OracleYolov5(3, nc, widen, deepen).train()
    for m in ref.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eps, m.momentum = eps, mom
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, norm_layer=partial(nn.BatchNorm2d, eps=eps, momentum=mom), widen_factor=widen, deepen_factor=deepen)
    for (k, a), b in zip(net.state_dict().items(), ref.state_dict().values()):
        assert torch.equal(a, b), k
    net = net.cuda().train()
    assert (net.engine().bn_eps, net.engine().bn_momentum) == (eps, mom)
    x, tg = synth.batch(B, size, nc, seed)
    lr = D.yolo_loss(size, size, ref(x), [D.Target(b, l) for b, l in tg])
    tot = D.train_step_total(lr, B)
    tot.backward()
    gn_r = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ref.parameters())).item()
    _, lr_h, tot_h = _step(net, x.cuda(), tg, size, B)
    got = np.array([lr_h.localization.item(), lr_h.objectness.item(), lr_h.classification.item(), tot_h.item()])
    want = np.array([lr.localization.item(), lr.objectness.item(), lr.classification.item(), tot.item()])
    np.testing.assert_allclose(got, want, rtol=2e-2)
    gn_h = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in net.parameters())).item()
    assert abs(gn_h - gn_r) <= 1.5e-1 * gn_r, (gn_h, gn_r)
    sd_r, sd_h = ref.state_dict(), net.state_dict()
    for suffix, tol in (("running_mean", 0.15), ("running_var", 2e-2)):
        a = torch.cat([sd_h[k].cpu().flatten() for k in sd_r if k.endswith(suffix)])
        b = torch.cat([sd_r[k].flatten() for k in sd_r if k.endswith(suffix)])
        assert _rel(a, b) <= tol, (suffix, _rel(a, b))
        # and they are NOT what momentum .03 would have left (running_var starts at 1: 0.9 + 0.1 var vs 0.97 + 0.03 var)
    rv = torch.cat([sd_h[k].cpu().flatten() for k in sd_r if k.endswith("running_var")])
    assert rv.max().item() <= 0.9 + 0.1 * 1e3 and (rv < 0.95).float().mean().item() > 0.5
    # eval mode: the oracle on the HIP path's own running statistics
    ref.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    ref.eval(); net.eval()
    with torch.no_grad():
        want_e, got_e = ref(x), net(x.cuda())
    for lvl in ("ll", "ml", "hl"):
        for part in ("box", "obj", "cls"):
            a, b = getattr(getattr(got_e, lvl), part).float().cpu(), getattr(getattr(want_e, lvl), part)
            assert _rel(a, b) <= 3e-2, (lvl, part, _rel(a, b))
    with pytest.raises(ValueError):
        Yolov5Network(3, nc, norm_layer=partial(nn.GroupNorm, 4))
    with pytest.raises(ValueError):
        Yolov5Network(3, nc, norm_layer=partial(nn.BatchNorm2d, momentum=None))
    assert Yolov5Network(3, nc, activation_layer=nn.ReLU)._act == (1, 0.0)        # (round 6: other elementwise activations are taken)
    with pytest.raises(ValueError):
        Yolov5Network(3, nc, activation_layer=nn.GELU)


def test_train_step_yv5m_640_vs_oracle():
    """BASELINE configs[4] scale (widen .75, deepen .67: 48 / 96 / 192 / 384 / 768 channels, 88 convs, 20.9 M parameters) at
    640 px, B=2, end to end against the fp32 oracle: the 48-channel layers run on the LDS-DMA path through the padded-tap
    K axis (k = tap * round_up(Cin, 32) + ci).  Same bars as the yv5s B=2 case."""
    widen, deepen, nc, B, size, seed = 0.75, 0.67, 10, 2, 640, 31
    torch.manual_seed(seed)
    ref = OracleYolov5(3, nc, widen, deepen).train()
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen)
    assert sum(p.numel() for p in net.parameters()) == 20907687
    for (k, a), b in zip(net.state_dict().items(), ref.state_dict().values()):
        assert torch.equal(a, b), k
    net = net.cuda().train()
    x, tg = synth.batch(B, size, nc, seed)
    lr = D.yolo_loss(size, size, ref(x), [D.Target(b, l) for b, l in tg])
    tot = D.train_step_total(lr, B)
    tot.backward()
    gn_r = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in ref.parameters())).item()
    _, lr_h, tot_h = _step(net, x.cuda(), tg, size, B)
    got = np.array([lr_h.localization.item(), lr_h.objectness.item(), lr_h.classification.item(), tot_h.item()])
    want = np.array([lr.localization.item(), lr.objectness.item(), lr.classification.item(), tot.item()])
    np.testing.assert_allclose(got, want, rtol=1e-2)
    gn_h = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in net.parameters())).item()
    assert abs(gn_h - gn_r) <= 1e-1 * gn_r, (gn_h, gn_r)


def test_train_step_well_conditioned_batch():
    """B=16 at 640 px: BatchNorm statistics are well conditioned (>= 6400 samples per channel in the deepest layers).
    Bars: losses <= 1e-2 and global gradient norm <= 5e-2 against the fp32 oracle (pinned to the reference).

    Per-tensor gradient cosine: a cosine of 0.98 against fp32 is NOT reachable by any implementation that stores
    activations in bf16 - measured here every run: the CPU oracle itself, with nothing changed but bf16 rounding at the
    storage points (oracle/bf16_emul.py), reaches a median cosine of ~0.81 and a minimum of ~0.67 against its own
    fp32 run at this batch (random-init network, train-mode BatchNorm: the loss gradient is that sensitive to 2^-9
    perturbations of the activations; the tensors and values are printed).  What separates a kernel bug from that
    sensitivity is whether the HIP path is any further from fp32 than the emulation is, tensor by tensor:
      cos(HIP, fp32) >= cos(bf16-emulated oracle, fp32) - 0.15 for every tensor carrying >= 0.1 % of the gradient norm,
      the medians of the two within 0.03, the mean absolute difference <= 0.05;
    the kernels themselves are held to bf16 rounding (<= 4e-3 .. 2e-2 relL2) by the teacher-forced tests below."""
    from oracle import bf16_emul
    widen, deepen, nc, B, size, seed = 0.5, 0.33, 10, 16, 640, 2023
    torch.manual_seed(seed)
    ref = OracleYolov5(3, nc, widen, deepen).train()
    torch.manual_seed(seed)
    emu = bf16_emul.emulate(OracleYolov5(3, nc, widen, deepen).train())
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen).cuda().train()
    x, tg = synth.batch(B, size, nc, seed)
    lr = D.yolo_loss(size, size, ref(x), [D.Target(b, l) for b, l in tg])
    tot = D.train_step_total(lr, B)
    tot.backward()
    D.train_step_total(D.yolo_loss(size, size, emu(x), [D.Target(b, l) for b, l in tg]), B).backward()
    _, lr_h, tot_h = _step(net, x.cuda(), tg, size, B)
    got = np.array([lr_h.localization.item(), lr_h.objectness.item(), lr_h.classification.item(), tot_h.item()])
    want = np.array([lr.localization.item(), lr.objectness.item(), lr.classification.item(), tot.item()])
    np.testing.assert_allclose(got, want, rtol=1e-2)
    gr = {k: p.grad.double() for k, p in ref.named_parameters()}
    ge = {k: p.grad.double() for k, p in emu.named_parameters()}
    gh = {k: p.grad.detach().cpu().double() for k, p in net.named_parameters()}
    gn_r = torch.sqrt(sum((g ** 2).sum() for g in gr.values())).item()
    gn_h = torch.sqrt(sum((g ** 2).sum() for g in gh.values())).item()
    assert abs(gn_h - gn_r) <= 5e-2 * gn_r, (gn_h, gn_r)
    cos = lambda a, b: (a.flatten() @ b.flatten() / (a.norm() * b.norm() + 1e-300)).item()
    rows = [(k, cos(gh[k], g), cos(ge[k], g)) for k, g in gr.items() if g.norm().item() >= 1e-3 * gn_r]
    ch, ce = np.array([r[1] for r in rows]), np.array([r[2] for r in rows])
    worst = min(rows, key=lambda r: r[1] - r[2])
    print(f"well-conditioned batch: grad norm HIP {gn_h:.4f} vs oracle {gn_r:.4f}; {len(rows)} tensors; cosine vs fp32: "
          f"HIP median {np.median(ch):.4f} min {ch.min():.4f} | bf16-emulated oracle median {np.median(ce):.4f} min {ce.min():.4f}; "
          f"largest deficit {worst[1] - worst[2]:+.4f} at {worst[0]}")
    assert len(rows) >= 100
    assert (ch >= ce - 0.15).all(), worst
    assert abs(np.median(ch) - np.median(ce)) <= 0.03 and np.abs(ch - ce).mean() <= 0.05
    # BN running statistics, network-wide
    sd_r, sd_h = ref.state_dict(), net.state_dict()
    for suffix, tol in (("running_mean", 2e-2), ("running_var", 5e-3)):
        a = torch.cat([sd_h[k].cpu().flatten() for k in sd_r if k.endswith(suffix)])
        b = torch.cat([sd_r[k].flatten() for k in sd_r if k.endswith(suffix)])
        assert _rel(a, b) <= tol, (suffix, _rel(a, b))


def _dY(eng, u):
    """dY of a conv unit after backward (device, [B, Ho, Wo, C] bf16): st.raw holds it - except for a stem that ran the
    fused backward (kodhip_stem_bwd_fused never writes dY; st.raw still holds y): there the stand-alone pass forms it from
    the same dA / y / coefficients."""
    from object_detection_cib_amd import _lib
    st = eng.cur.units[u.name]
    if not st.stem_fused:
        return st.raw
    dy = st.raw.clone()
    C_, aff, dA = u.cout, st.aff.data_ptr(), eng.cur.gact[u.dst.buf.name]
    _lib.check(_lib.lib().kodhip_bn_silu_bwd_apply(dA.data_ptr(), u.dst.buf.C, u.dst.coff, dy.data_ptr(), st.raw_ld,
                                                   aff, aff + 4 * C_, st.coef.data_ptr(), None, 0, 0, 0, st.M, C_,
                                                   torch.cuda.current_stream().cuda_stream), "bwd_apply")
    return dy


def test_bench_geometry_b64_640_deterministic_and_teacher_forced():
    """BASELINE configs[1] at its real batch: B=64, 640 px (M up to 6.55 M pixels: 256-pixel tiles, full split-K /
    statistic-slot geometry, exactly what bench.py times).  (1) two steps on the same batch give bit-identical
    gradients for every parameter; (2) the six largest-M units plus the first stride-2 stage conv are checked
    teacher-forced (fp32 torch on the HIP path's own bf16 inputs): raw conv output, BatchNorm batch statistics, dW."""
    import torch.nn.functional as F
    widen, deepen, nc, B, size, seed = 0.5, 0.33, 10, 64, 640, 2023
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen).cuda().train()
    x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(seed))
    tg = synth.targets(B, size, nc, seed, nmin=4, nmax=30)
    xg = x.cuda()
    runs = []
    for _ in range(2):
        for p in net.parameters():
            p.grad = None
        _, lr, tot = _step(net, xg, tg, size, B)
        runs.append((tot.item(), torch.cat([p.grad.flatten() for p in net.parameters()]).clone()))
    assert np.isfinite(runs[0][0]) and runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]), "gradients differ between two runs of the same step"
    eng = net.engine()
    grads = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    params = {k: p.detach().cpu() for k, p in net.named_parameters()}
    bf = lambda t: t.to(torch.bfloat16).float()
    units = sorted(eng.exec_units, key=lambda u: -eng.cur.units[u.name].M)[:6]
    units += [u for u in eng.exec_units if u.name == "backbone.stages.stage2.blocks.0"]
    worst, ref_y = {}, {}
    for u in units:
        st = eng.cur.units[u.name]
        # NOTE st.raw holds dY after backward; the forward's pre-BN tensor is recomputed by one more forward below
        X = bf(x) if u.stem else eng.cur.act[u.src.buf.name][..., u.src.coff:u.src.coff + u.src.C].float().permute(0, 3, 1, 2).cpu()
        W = bf(params[u.name + ".0.weight"]).requires_grad_(True)
        y = F.conv2d(X, W, None, u.s, u.p)
        dY = _dY(eng, u).float().permute(0, 3, 1, 2).cpu()
        y.backward(dY)
        worst.setdefault("dW", 0.0)
        e = _rel(grads[u.name + ".0.weight"], W.grad)
        worst["dW"] = max(worst["dW"], e)
        assert e <= 5e-3, ("dW", u.name, e)
        ref_y[u.name] = y.detach()
    with torch.no_grad():
        net.forward_raw(xg)             # train-mode forward again: st.raw = pre-BN output, st.aff = batch statistics
    for u in units:
        st = eng.cur.units[u.name]
        raw = st.raw.float().permute(0, 3, 1, 2).cpu()
        e = _rel(raw, ref_y.pop(u.name))
        worst["conv_raw"] = max(worst.get("conv_raw", 0.0), e)
        assert e <= 4e-3, ("conv_raw", u.name, e)
        C_ = u.cout
        aff = st.aff.cpu().double()
        r64 = raw.double()
        mean = r64.mean((0, 2, 3))
        var = r64.var((0, 2, 3), unbiased=False)
        e_m = ((aff[2 * C_:3 * C_] - mean).abs().max() / (var.sqrt().max() + 1e-30)).item()
        e_r = _rel(aff[3 * C_:4 * C_], 1.0 / torch.sqrt(var + 1e-3))
        worst["bn_mean"], worst["bn_rstd"] = max(worst.get("bn_mean", 0.0), e_m), max(worst.get("bn_rstd", 0.0), e_r)
        assert e_m <= 1e-4 and e_r <= 1e-4, ("bn stats", u.name, e_m, e_r)
    print("B=64/640 teacher-forced worst:", {k: round(v, 6) for k, v in worst.items()}, [u.name for u in units])


def test_eval_mode_forward_vs_oracle_through_decode():
    """Validation path net.eval() -> decode: after a few HIP training steps (non-trivial running statistics) the same
    state_dict is loaded into the fp32 oracle; eval-mode head outputs and the decoded [B, 25200-like, 5+nc] tensor
    must agree (no train-mode BN amplification in eval => a tight bar for bf16 storage)."""
    from object_detection_cib_amd.core.anchors.info import voc_anchor_info as vai
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.layers import get_detections
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo
    widen, deepen, nc, B, size, seed = 0.5, 0.33, 10, 4, 320, 17
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen).cuda().train()
    for step in range(4):
        x, tg = synth.batch(B, size, nc, seed + step)
        for p in net.parameters():
            p.grad = None
        _step(net, x.cuda(), tg, size, B)
        net.engine().sgd_step((0.05, 0.01, 0.01), (0.8, 0.8, 0.8), (0.0, 5e-4, 0.0))
    ref = OracleYolov5(3, nc, widen, deepen)
    ref.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    ref.eval(); net.eval()
    x, _ = synth.batch(B, size, nc, seed + 100)
    with torch.no_grad():
        out_r = ref(x)
        out_h = net(x.cuda())
        det_r = D.decode(out_r, size, size)
        det_h = get_detections(FeatureShape(width=size, height=size), out_h, LayerwiseAnchorInfo(vai(8), vai(16), vai(32))).cpu()
    worst = 0.0
    for hr, hh in zip(out_r, out_h):
        for tr, th in zip(hr, hh):
            worst = max(worst, _rel(th.cpu(), tr))
    print("eval-mode head logits worst relL2:", worst, "decoded max|dprob|", (det_h[..., 4:] - det_r[..., 4:]).abs().max().item())
    assert worst <= 2e-2, worst
    assert det_h.shape == det_r.shape
    assert (det_h[..., 4:] - det_r[..., 4:]).abs().max() <= 2e-2
    assert _rel(det_h[..., :4], det_r[..., :4]) <= 1e-2
    # an eval forward must not touch the BatchNorm buffers
    sd = net.state_dict()
    assert all(torch.equal(sd[k].cpu(), v) for k, v in ref.state_dict().items() if "running" in k or "num_batches" in k)


@pytest.mark.parametrize("case", ["yv5s_160", "yv5s_640", "yv5s_416", "yv5m_96", "yv5s_rect160x224", "yv5n_rect192x96"])
def test_layers_teacher_forced(case):
    """Every conv+BN+SiLU unit, in situ: feed the HIP path's own bf16 input activation / output gradient to
    plain torch fp32 and compare that unit's output, dY, dgamma, dbeta, dW and the accumulated dX of every
    tensor (all consumers: convs, residual adds, upsamples).  No error amplification => tight bars."""
    import torch.nn.functional as F
    cases = dict(synth.network_cases())
    cases["yv5m_96"] = (0.75, 0.67, 10, 3, 96, 5)
    cases["yv5s_rect160x224"] = (0.5, 0.33, 10, 2, (160, 224), 6)      # H != W: nothing may assume square maps
    cases["yv5n_rect192x96"] = (0.25, 0.33, 10, 3, (192, 96), 8)
    widen, deepen, nc, B, size, seed = cases[case]
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen).cuda().train()
    if isinstance(size, tuple):
        img_h, img_w = size
        x = torch.rand(B, 3, img_h, img_w, generator=torch.Generator().manual_seed(seed))
        tg = synth.targets(B, min(size), nc, seed)
    else:
        img_h = img_w = size
        x, tg = synth.batch(B, size, nc, seed)
    eng = net.engine()
    raws = net.forward_raw(x.cuda())
    for r in raws:
        r.retain_grad()
    fwd_raw = {u.name: eng.cur.units[u.name].raw.float().cpu() for u in eng.exec_units}
    lr = _loss()(FeatureShape(width=img_w, height=img_h),
                 tuple((r[..., :4], r[..., 4:5], r[..., 5:]) for r in raws), tuple(DetectionTarget(b, l) for b, l in tg))
    (B * (lr.localization + lr.classification + lr.objectness)).backward()
    grads = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    params = {k: p.detach().cpu() for k, p in net.named_parameters()}

    def view(v, grad=False):
        t = (eng.cur.gact if grad else eng.cur.act)[v.buf.name]
        return t[..., v.coff:v.coff + v.C].float().permute(0, 3, 1, 2).cpu()

    bf = lambda t: t.to(torch.bfloat16).float()
    expect = {}                                   # buf name -> expected accumulated gradient [B, Ctot, H, W]

    def add_expect(v, g):
        if v.buf.name not in expect:
            t = eng.cur.gact[v.buf.name]
            expect[v.buf.name] = torch.zeros((t.shape[0], t.shape[3], t.shape[1], t.shape[2]), dtype=torch.float64)
        expect[v.buf.name][:, v.coff:v.coff + v.C] += g.double()

    worst = {}

    def note(kind, name, val, tol):
        worst[kind] = max(worst.get(kind, 0.0), val)
        assert val <= tol, (kind, name, val)

    for op in eng.g.ops:
        if op.kind == "up":
            add_expect(op.src, F.avg_pool2d(view(op.dst, True), 2) * 4)
            continue
        if op.kind != "conv":
            continue
        u = op.unit
        st = eng.cur.units[u.name]
        X = bf(x) if u.stem else view(u.src)
        W = bf(params[u.name + ".0.weight"]).requires_grad_(True)
        Xr = X.clone().requires_grad_(not u.stem)
        y = F.conv2d(Xr, W, None, u.s, u.p)
        note("conv_raw", u.name, _rel(fwd_raw[u.name].permute(0, 3, 1, 2), y.detach()), 4e-3)
        yb = fwd_raw[u.name].permute(0, 3, 1, 2).clone().requires_grad_(True)     # HIP's own bf16 pre-BN tensor
        gamma = params[u.name + ".1.weight"].clone().requires_grad_(True)
        beta = params[u.name + ".1.bias"].clone().requires_grad_(True)
        out = F.silu(F.batch_norm(yb, None, None, gamma, beta, True, 0.03, 1e-3))
        if u.residual is not None:
            out = out + view(u.residual)
        note("act", u.name, _rel(view(u.dst), out.detach()), 4e-3)
        dA = view(u.dst, True)
        out.backward(dA)
        dY_hip = _dY(eng, u).float().permute(0, 3, 1, 2).cpu()
        note("dY", u.name, _rel(dY_hip, yb.grad), 1.5e-2)
        note("dgamma", u.name, _rel(grads[u.name + ".1.weight"], gamma.grad), 2e-2)
        note("dbeta", u.name, _rel(grads[u.name + ".1.bias"], beta.grad), 2e-2)
        y.backward(dY_hip)
        note("dW", u.name, _rel(grads[u.name + ".0.weight"], W.grad), 5e-3)
        if not u.stem:
            add_expect(u.src, Xr.grad)
        if u.residual is not None:
            add_expect(u.residual, dA)
    # heads: weight / bias gradients and their dX contributions from the autograd-delivered head gradients
    A = 3
    for hu, raw in zip(eng.g.heads, raws):
        X = view(hu.src).requires_grad_(True)
        outs = []
        for key, p in (("box", 4), ("obj", 1), ("cls", nc)):
            w = bf(params[f"{hu.name}.{key}_head.conv.weight"]).requires_grad_(True)
            b = params[f"{hu.name}.{key}_head.conv.bias"].clone().requires_grad_(True)
            yk = F.conv2d(X, w, b)
            outs.append((yk.view(B, A, p, *yk.shape[2:]).permute(0, 1, 3, 4, 2), w, b, key))
        full = torch.cat([o[0] for o in outs], -1)
        note("head_fwd", hu.name, _rel(raw.detach().cpu(), full.detach()), 2e-3)
        full.backward(bf(raw.grad.cpu()))
        add_expect(hu.src, X.grad)
        for _, w, b, key in outs:
            note("head_dW", f"{hu.name}.{key}", _rel(grads[f"{hu.name}.{key}_head.conv.weight"], w.grad), 1e-2)
            note("head_db", f"{hu.name}.{key}", _rel(grads[f"{hu.name}.{key}_head.conv.bias"], b.grad), 1e-2)
    # accumulated activation gradients of every buffer (all consumers: convs, residual adds, upsamples, heads);
    # the SPPF concat also receives pool-backward terms, covered by test_hip_ops
    checked = 0
    for name, g in expect.items():
        if ".2.cat" in name:
            continue
        got = eng.cur.gact[name].float().permute(0, 3, 1, 2).cpu()
        note("dX_accum", name, _rel(got, g), 2e-2)
        checked += 1
    assert checked >= 20
    print("teacher-forced worst relL2:", {k: round(v, 5) for k, v in worst.items()})


def test_sgd_trajectory_vs_oracle():
    """3 optimizer steps with warm-up hyper-parameters: parameters track the oracle's torch.optim.SGD."""
    from oracle import optim as O
    widen, deepen, nc, B, size, seed = 0.25, 0.33, 10, 2, 128, 3
    torch.manual_seed(seed)
    ref = OracleYolov5(3, nc, widen, deepen).train()
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen).cuda().train()
    bias, decay, norm = O.param_groups(ref)
    opt = torch.optim.SGD([dict(params=bias, weight_decay=0.0), dict(params=decay, weight_decay=5e-4),
                           dict(params=norm, weight_decay=0.0)], lr=0.01, momentum=0.937, nesterov=True)
    for step in range(3):
        x, tg = synth.batch(B, size, nc, seed + step)
        w = O.warmup_values(step, 0, 100)
        for pg, name in zip(opt.param_groups, O.GROUP_NAMES):
            pg["lr"], pg["momentum"] = w[name]
        opt.zero_grad()
        D.train_step_total(D.yolo_loss(size, size, ref(x), [D.Target(b, l) for b, l in tg]), B).backward()
        opt.step()
        for p in net.parameters():
            p.grad = None
        _step(net, x.cuda(), tg, size, B)
        net.engine().sgd_step([w[n][0] for n in O.GROUP_NAMES], [w[n][1] for n in O.GROUP_NAMES], (0.0, 5e-4, 0.0))
    num = den = 0.0
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        num += (p.detach().cpu().double() - q.detach().double()).pow(2).sum().item()
        den += q.detach().double().pow(2).sum().item()
    assert (num / den) ** 0.5 <= 2e-3, (num / den) ** 0.5


def test_forward_is_deterministic_and_eval_mode_runs():
    torch.manual_seed(0)
    net = Yolov5Network(3, 10, widen_factor=0.25, deepen_factor=0.33).cuda().train()
    x, tg = synth.batch(2, 96, 10, 1)
    a = [t.clone() for t in net.forward_raw(x.cuda())]
    net2_state = {k: v.clone() for k, v in net.state_dict().items()}
    b = net.forward_raw(x.cuda())
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    net.eval()
    with torch.no_grad():
        e = net(x.cuda())
    assert all(torch.isfinite(t).all() for h in e for t in h)
    assert set(net2_state) == set(net.state_dict())


@pytest.mark.parametrize("pos_weight", [False, True])
def test_train_step_without_autograd_equals_autograd_route(pos_weight):
    """Yolov5Network.train_step (engine forward -> Yolov5Loss.value_and_grad: ONE pass of the loss kernels -> engine
    backward; what the captured step and bench.py run) against the reference's call sequence through torch autograd
    (net(x) -> loss(...) -> (B * sum).backward(): the loss kernels run once per direction): every loss value and every
    parameter gradient bit for bit, BatchNorm buffers included."""
    size, B, nc = 160, 4, 10
    x, _ = synth.batch(B, size, nc, 11)
    tg = synth.targets(B, size, nc, 11, nmin=1, nmax=9)
    targets = tuple(DetectionTarget(b, l) for b, l in tg)
    shape = FeatureShape(width=size, height=size)
    got = []
    for route in ("autograd", "direct"):
        torch.manual_seed(3)
        net = Yolov5Network(3, nc, widen_factor=0.25, deepen_factor=0.33).cuda().train()
        loss = _loss()
        if pos_weight:
            loss.weights = torch.linspace(0.5, 2.0, nc)
        if route == "autograd":
            lr = loss(shape, net(x.cuda()), targets)
            total = B * (lr.localization + lr.classification + lr.objectness)
            total.backward()
        else:
            total, lr = net.train_step(x.cuda(), loss, shape, targets, float(B))
        net.engine().wait_grads()
        torch.cuda.synchronize()
        got.append(dict(total=total.detach().cpu(), parts=torch.stack([lr.localization, lr.objectness, lr.classification]).detach().cpu(),
                        grads=torch.cat([p.grad.flatten() for p in net.parameters()]).cpu(),
                        rm=net.engine().rm_arena.cpu(), rv=net.engine().rv_arena.cpu()))
    a, d = got
    assert torch.equal(a["parts"], d["parts"]) and torch.equal(a["total"], d["total"]), (a["parts"], d["parts"])
    assert torch.isfinite(d["grads"]).all() and d["grads"].abs().max() > 0
    assert torch.equal(a["grads"], d["grads"])
    assert torch.equal(a["rm"], d["rm"]) and torch.equal(a["rv"], d["rv"])


@pytest.mark.parametrize("size,B", [(160, 4), (640, 16)])
def test_side_stream_scheduling_does_not_change_results(size, B):
    """Where a kernel runs must not matter: the default schedule (weight gradients forked by event at bn_silu_bwd_apply,
    CSP short branches / P3-P4 heads / label assignment on side streams, head chains of the backward pass aside) against
    everything on one stream - eagerly and as a replayed hipGraph: losses and every
    parameter gradient bit for bit (a missing dependency shows up as a difference, at least some of the time)."""
    nc = 10
    x, _ = synth.batch(B, size, nc, 21)
    tg = synth.targets(B, size, nc, 21, nmin=2, nmax=9)
    targets = tuple(DetectionTarget(b, l) for b, l in tg)
    shape = FeatureShape(width=size, height=size)
    xc = x.cuda()
    results = {}
    for name, cfg in (("default", {}), ("one stream", dict(wgrad_overlap=False, branch_overlap=False)), ("default, graph", {})):
        torch.manual_seed(3)
        net = Yolov5Network(3, nc, widen_factor=0.5, deepen_factor=0.33).cuda().train()
        loss = _loss()
        eng = net.engine()
        for k, v in cfg.items():
            setattr(eng, k, v)
        from object_detection_cib_amd.core.label_assignment.yv5 import BatchedTargets
        bt = BatchedTargets.from_targets(targets, torch.device("cuda", 0))

        params = list(net.parameters())

        def step():
            for p in params:
                p.grad = None
            total, lr = net.train_step(xc, loss, shape, bt, float(B))
            eng.wait_grads()
            return total
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                total = step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if name.endswith("graph"):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                total = step()
            for _ in range(3):
                g.replay()
        torch.cuda.synchronize()
        results[name] = (total.detach().cpu().clone(), torch.cat([p.grad.flatten() for p in net.parameters()]).cpu().clone(),
                         eng.rm_arena.cpu().clone())
    ref = results["default"]
    for name, (t, g_, rm) in results.items():
        assert torch.equal(t, ref[0]), (name, t, ref[0])
        assert torch.equal(g_, ref[1]), name
        if not name.endswith("graph"):          # (the replayed run took more steps: running statistics moved further)
            assert torch.equal(rm, ref[2]), name


def test_multi_producer_dx_b64_640_vs_fp32_torch():
    """B=64 / 640 px, teacher-forced: the accumulated gradient of EVERY activation tensor with several producers
    (residual inputs, P3 / P4, the pyramid's concat halves, T3 / O4, the SPPF concat) against fp32 torch fed the HIP
    path's own bf16 operands, in both accumulation modes: default (each producer read-modify-writes the bf16 buffer) and
    EngineOptions.dx_accum_fp32 (fp32 partial sums, one rounding - what autograd does).  Bars: bf16 accumulation <= 5e-3
    relL2, fp32 accumulation <= 2.5e-3 (a single bf16 rounding of the stored result) and never worse than bf16."""
    import torch.nn.functional as F
    from object_detection_cib_amd.engine.options import EngineOptions
    from object_detection_cib_amd.engine.plan import backward_writes, plan_f32_accumulation
    widen, deepen, nc, B, size, seed = 0.5, 0.33, 10, 64, 640, 2023
    x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(seed)).cuda()
    tg = synth.targets(B, size, nc, seed, nmin=4, nmax=30)
    bf = lambda t: t.to(torch.bfloat16).float()
    errs = {}
    for mode in ("bf16", "fp32"):
        torch.manual_seed(seed)
        net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen)
        opts = EngineOptions.from_env()
        opts.dx_accum_fp32 = mode == "fp32"
        net.engine_options = opts
        net = net.cuda().train()
        eng = net.engine()
        raws = net.forward_raw(x)
        for r in raws:
            r.retain_grad()
        lr = _loss()(FeatureShape(width=size, height=size), tuple((r[..., :4], r[..., 4:5], r[..., 5:]) for r in raws),
                     tuple(DetectionTarget(b, l) for b, l in tg))
        (B * (lr.localization + lr.classification + lr.objectness)).backward()
        torch.cuda.synchronize()
        assert (eng._f32plan is not None) == (mode == "fp32")
        params = {k: p.detach().cpu() for k, p in net.named_parameters()}
        units = {u.name: u for u in eng.exec_units}
        duals = [v.name for v in eng._dual.values()]
        ws, _ = backward_writes(eng.g, duals)
        plan = plan_f32_accumulation(ws, {b.name: b.C for b in eng.g.bufs})
        multi = set(plan.shadow_bufs) | {w.buf for w in ws if plan.modes[w.key] == 4}
        assert len(multi) == 13

        def gview(v):                 # gradient of a view, NCHW fp32 on the host
            return eng.cur.gact[v.buf.name][..., v.coff:v.coff + v.C].float().permute(0, 3, 1, 2).cpu()

        def aview(v):
            return eng.cur.act[v.buf.name][..., v.coff:v.coff + v.C].float().permute(0, 3, 1, 2).cpu()

        def conv_dx(u):               # fp32 torch data gradient of one conv unit from the HIP path's bf16 dY and weights
            st = eng.cur.units[u.name]
            dY = _dY(eng, u).float().permute(0, 3, 1, 2).cpu()
            W = bf(params[u.name + ".0.weight"])
            shape = (B, u.cin, st.H, st.W)
            return torch.nn.grad.conv2d_input(shape, W, dY, u.s, u.p)

        expect = {}

        def add(buf, lo, g):
            t = eng.cur.gact[buf]
            e = expect.setdefault(buf, torch.zeros((t.shape[0], t.shape[3], t.shape[1], t.shape[2]), dtype=torch.float32))
            e[:, lo:lo + g.shape[1]] += g

        pool_terms = {}
        for w in ws:
            if w.buf not in multi:
                continue
            if w.kind == "dgrad":
                u = units[w.unit]
                g = conv_dx(u)
                if u.name in eng._dual:
                    g = g + conv_dx(eng._dual[u.name])
                add(w.buf, w.lo, g)
            elif w.kind == "res":
                u = units[w.key[1]]
                add(w.buf, w.lo, gview(u.dst))
            elif w.kind == "up":
                op = eng.g.ops[w.key[1]]
                add(w.buf, w.lo, F.avg_pool2d(gview(op.dst), 2) * 4)
            elif w.kind == "head":
                hu = [h for h in eng.g.heads if h.name == w.key[1]][0]
                raw = raws[[h.name for h in eng.g.heads].index(hu.name)]
                X = aview(hu.src).requires_grad_(True)
                outs = []
                for key, p_ in (("box", 4), ("obj", 1), ("cls", nc)):
                    yk = F.conv2d(X, bf(params[f"{hu.name}.{key}_head.conv.weight"]), None)
                    outs.append(yk.view(B, 3, p_, *yk.shape[2:]).permute(0, 1, 3, 4, 2))
                torch.cat(outs, -1).backward(bf(raw.grad.cpu()))
                add(w.buf, w.lo, X.grad)
            elif w.kind == "pool":    # SPPF: gradient of pool(slice q) w.r.t. slice q from the FINAL gradient of slice q + 1
                op = eng.g.ops[w.key[1]]
                xs = aview(op.src).requires_grad_(True)
                F.max_pool2d(xs, 5, 1, 2).backward(gview(op.dst))
                add(w.buf, w.lo, xs.grad)
        for buf, e in sorted(expect.items()):
            got = eng.cur.gact[buf].float().permute(0, 3, 1, 2).cpu()
            # compare only channel ranges with several producers (single-producer slices are covered elsewhere)
            C = got.shape[1]
            cover = torch.zeros(C, dtype=torch.int32)
            for w in ws:
                if w.buf == buf:
                    cover[w.lo:w.hi] += 1
            sel = cover > 1
            errs.setdefault(buf, {})[mode] = _rel(got[:, sel], e[:, sel])
        del net, eng
        torch.cuda.empty_cache()
    print("multi-producer dX at B=64/640, relL2 vs fp32 torch (bf16 accumulation | fp32 accumulation):")
    for buf, d in sorted(errs.items()):
        print(f"  {buf:45s} {d['bf16']:.5f} | {d['fp32']:.5f}")
    assert len(errs) == 13
    for buf, d in errs.items():
        assert d["bf16"] <= 5e-3, (buf, d)
        assert d["fp32"] <= 2.5e-3, (buf, d)
        assert d["fp32"] <= 1.02 * d["bf16"], (buf, d)


def test_schedule_switches_keep_the_gradients():
    """Launch-schedule switches of the backward program against the default, one training step at 320 px:
    * EngineOptions.stem_bwd_fused = False (the stem's BatchNorm/SiLU backward as its own pass + the generic weight gradient
      instead of kodhip_stem_bwd_fused) and the fused kernel on the weight-gradient stream instead of the main stream: only
      the stem's weight gradient may differ, by fp32 summation order (same bf16 dY);
    * EngineOptions.dual_wgrad = False: see the end of the test."""
    from object_detection_cib_amd.engine.options import EngineOptions
    widen, deepen, nc, B, size, seed = 0.5, 0.33, 10, 4, 320, 11
    x, tg = synth.batch(B, size, nc, seed)
    got = {}
    for tag in ("default", "unfused", "fused_wg", "single_wgrads"):
        torch.manual_seed(seed)
        net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen)
        opts = EngineOptions.from_env()
        if tag == "unfused":
            opts.stem_bwd_fused = False
        if tag == "fused_wg":
            opts.native = dict(opts.native, KODHIP_STEM_BWD_STREAM="wg")
        if tag == "single_wgrads":
            opts.dual_wgrad = False
        net.engine_options = opts
        net = net.cuda().train()
        _step(net, x.cuda(), tg, size, B)
        eng = net.engine()
        assert eng.cur.units["backbone.stem"].stem_fused == (tag != "unfused")
        n_dual = sum(1 for st in eng.cur.units.values() if st.wg_dual > 0)
        assert n_dual == (0 if tag == "single_wgrads" else 8), n_dual
        got[tag] = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    for k, g in got["default"].items():
        assert torch.isfinite(g).all()
        assert torch.equal(got["fused_wg"][k], g), k
        if k == "backbone.stem.0.weight":
            top = g.abs().max().item()
            assert top > 0 and (got["unfused"][k] - g).abs().max().item() <= 1e-4 * top, k
        else:
            assert torch.equal(got["unfused"][k], g), k
        # EngineOptions.dual_wgrad = False: a CSP layer's main_conv / short_conv weight gradients as two launches instead
        # of kodhip_conv_wgrad_dual - other split-K boundaries for those sixteen tensors, everything else untouched
        if k.endswith(("main_conv.0.weight", "short_conv.0.weight")):
            top = g.abs().max().item()
            assert (got["single_wgrads"][k] - g).abs().max().item() <= 1e-4 * top + 1e-7, k
        else:
            assert torch.equal(got["single_wgrads"][k], g), k


def test_yv5m_bench_geometry_b64_640_deterministic_and_teacher_forced():
    """BASELINE configs[4] at its per-GPU batch: yv5m (widen .75, deepen .67: 48 / 96 / 192 / 384 / 768 channels, 88 convs),
    B=64, 640 px - the 256-pixel-tile / split-K / padded-tap geometry of those widths.  (1) two steps on the same batch give
    bit-identical gradients; (2) the largest-M units of every width class plus a stride-2 stage conv and a 3x3 block conv
    are checked teacher-forced (fp32 torch on the HIP path's own bf16 operands): raw conv output, BatchNorm batch
    statistics, dW."""
    import torch.nn.functional as F
    widen, deepen, nc, B, size, seed = 0.75, 0.67, 10, 64, 640, 77
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen).cuda().train()
    x = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(seed))
    tg = synth.targets(B, size, nc, seed, nmin=4, nmax=30)
    xg = x.cuda()
    runs = []
    for _ in range(2):
        for p in net.parameters():
            p.grad = None
        _, lr, tot = _step(net, xg, tg, size, B)
        runs.append((tot.item(), torch.cat([p.grad.flatten() for p in net.parameters()]).clone()))
    assert np.isfinite(runs[0][0]) and runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]), "gradients differ between two runs of the same step"
    eng = net.engine()
    grads = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    params = {k: p.detach().cpu() for k, p in net.named_parameters()}
    bf = lambda t: t.to(torch.bfloat16).float()
    by_m = sorted(eng.exec_units, key=lambda u: -eng.cur.units[u.name].M)
    units, seen = [], set()
    for u in by_m:                                    # the largest-M unit of every (cin, cout, k, s) class, first five classes
        key = (u.cin, u.cout, u.k, u.s)
        if key not in seen and not u.stem:
            seen.add(key)
            units.append(u)
        if len(units) == 5:
            break
    units += [u for u in eng.exec_units if u.name in ("backbone.stages.stage3.blocks.0", "backbone.stages.stage2.blocks.1.blocks.0.conv2")]
    assert {u.cin for u in units} & {48, 96, 192}
    worst, ref_y = {}, {}
    for u in units:
        st = eng.cur.units[u.name]
        X = eng.cur.act[u.src.buf.name][..., u.src.coff:u.src.coff + u.src.C].float().permute(0, 3, 1, 2).cpu()
        W = bf(params[u.name + ".0.weight"]).requires_grad_(True)
        y = F.conv2d(X, W, None, u.s, u.p)
        y.backward(_dY(eng, u).float().permute(0, 3, 1, 2).cpu())     # (st.raw holds dY after backward; fused stem: _dY)
        e = _rel(grads[u.name + ".0.weight"], W.grad)
        worst["dW"] = max(worst.get("dW", 0.0), e)
        assert e <= 5e-3, ("dW", u.name, e)
        ref_y[u.name] = y.detach()
    with torch.no_grad():
        net.forward_raw(xg)             # train-mode forward again: st.raw = pre-BN output, st.aff = batch statistics
    for u in units:
        st = eng.cur.units[u.name]
        raw = st.raw.float().permute(0, 3, 1, 2).cpu()
        e = _rel(raw, ref_y.pop(u.name))
        worst["conv_raw"] = max(worst.get("conv_raw", 0.0), e)
        assert e <= 4e-3, ("conv_raw", u.name, e)
        C_ = u.cout
        aff = st.aff.cpu().double()
        r64 = raw.double()
        mean, var = r64.mean((0, 2, 3)), r64.var((0, 2, 3), unbiased=False)
        e_m = ((aff[2 * C_:3 * C_] - mean).abs().max() / (var.sqrt().max() + 1e-30)).item()
        e_r = _rel(aff[3 * C_:4 * C_], 1.0 / torch.sqrt(var + 1e-3))
        assert e_m <= 1e-4 and e_r <= 1e-4, ("bn stats", u.name, e_m, e_r)
    print("yv5m B=64/640 teacher-forced worst:", {k: round(v, 6) for k, v in worst.items()}, [u.name for u in units])
