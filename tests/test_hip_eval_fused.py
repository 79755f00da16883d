"""The fused eval forward through the engine and the public interface: `net.eval().fuse_eval()` runs every conv + BatchNorm +
activation (+ residual) unit as one launch of kodhip_conv_fwd_fused (EngineOptions.eval_fused).

Against the fp32 oracle under the bars of test_hip_network.py::test_eval_mode_forward_vs_oracle_through_decode (head logits
worst relL2 <= 2e-2, decoded scores <= 2e-2 absolute, boxes relL2 <= 1e-2), the launch program through `eng.profile`, the
training step after a fused eval forward, GraphedEvalForward, and a sub-module front end.
"""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detection as D, network as N, synth  # noqa: E402
from oracle.network import OracleYolov5  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info as vai  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.data.detection import DetectionTarget  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.layers import get_detections  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo  # noqa: E402
from object_detection_cib_amd.nn.networks.yolov5 import Yolov5BatchNorm2d, Yolov5Network  # noqa: E402
from test_hip_network import _loss, _rel, _step  # noqa: E402

ANCHORS = LayerwiseAnchorInfo(vai(8), vai(16), vai(32))
BN_KEYS = ("running_mean", "running_var", "num_batches_tracked")


def trained(widen, deepen, nc, B, size, seed, steps=4):
    """a network after `steps` HIP training steps (non-trivial running statistics), as
    test_eval_mode_forward_vs_oracle_through_decode prepares it; size: int or (H, W)"""
    torch.manual_seed(seed)
    net = Yolov5Network(3, nc, widen_factor=widen, deepen_factor=deepen).cuda().train()
    H, W = size if isinstance(size, tuple) else (size, size)
    for step in range(steps):
        if H == W:
            x, tg = synth.batch(B, H, nc, seed + step)
        else:
            x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed + step))
            tg = synth.targets(B, min(H, W), nc, seed + step)
        for p in net.parameters():
            p.grad = None
        res = net(x.cuda())
        lr = _loss()(FeatureShape(width=W, height=H), res, tuple(DetectionTarget(b, l) for b, l in tg))
        (B * (lr.localization + lr.classification + lr.objectness)).backward()
        net.engine().sgd_step((0.05, 0.01, 0.01), (0.8, 0.8, 0.8), (0.0, 5e-4, 0.0))
    return net


def eval_errors(net, ref, x, H, W):
    """(worst head relL2, decoded score max abs, box relL2, raw head tensors) of net(x) against the oracle"""
    with torch.no_grad():
        out_r = ref(x)
        out_h = net(x.cuda())
        det_r = D.decode(out_r, W, H)
        det_h = get_detections(FeatureShape(width=W, height=H), out_h, ANCHORS).cpu()
    worst = max(_rel(th.cpu(), tr) for hr, hh in zip(out_r, out_h) for tr, th in zip(hr, hh))
    assert det_h.shape == det_r.shape
    return (worst, (det_h[..., 4:] - det_r[..., 4:]).abs().max().item(), _rel(det_h[..., :4], det_r[..., :4]),
            [t.clone() for h in out_h for t in h])


def oracle_of(net, widen, deepen, nc):
    ref = OracleYolov5(3, nc, widen, deepen)
    ref.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    return ref.eval()


def assert_bars(what, errs):
    worst, dprob, box = errs[:3]
    assert worst <= 2e-2 and dprob <= 2e-2 and box <= 1e-2, (what, worst, dprob, box)


def test_yv5s_fused_vs_oracle_and_two_pass():
    widen, deepen, nc, B, size, seed = 0.5, 0.33, 10, 4, 320, 17
    net = trained(widen, deepen, nc, B, size, seed)
    ref = oracle_of(net, widen, deepen, nc)
    x, _ = synth.batch(B, size, nc, seed + 100)
    net.eval()
    bn_before = {k: v.clone() for k, v in net.state_dict().items() if k.endswith(BN_KEYS)}
    two = eval_errors(net, ref, x, size, size)
    assert net.fuse_eval() is net and net.engine().opt.eval_fused is True
    fused = eval_errors(net, ref, x, size, size)
    print(f"yv5s eval vs fp32 oracle (head logits worst relL2, decoded score max abs, box relL2): two-pass "
          f"{two[0]:.3e} {two[1]:.3e} {two[2]:.3e} | fused {fused[0]:.3e} {fused[1]:.3e} {fused[2]:.3e}")
    assert_bars("two-pass", two)
    assert_bars("fused", fused)
    sd = net.state_dict()
    assert all(torch.equal(sd[k], v) for k, v in bn_before.items()), "an eval forward must not touch the BatchNorm buffers"
    assert set(sd) == set(ref.state_dict())                        # no parameter, no buffer converted
    net.fuse_eval(False)
    again = eval_errors(net, ref, x, size, size)
    assert all(torch.equal(a, b) for a, b in zip(again[3], two[3])), "fuse_eval(False) must return to the two-pass bits"


@pytest.mark.parametrize("case", ["yv5m_96", "yv5n_rect192x96"])
def test_other_widths_and_rectangular_input(case):
    """yv5m: 48 / 96-channel K tails; 192 x 96: H != W"""
    widen, deepen, nc, B, size, seed = {"yv5m_96": (0.75, 0.67, 10, 2, 96, 5), "yv5n_rect192x96": (0.25, 0.33, 10, 3, (192, 96), 8)}[case]
    H, W = size if isinstance(size, tuple) else (size, size)
    net = trained(widen, deepen, nc, B, size, seed)
    ref = oracle_of(net, widen, deepen, nc)
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(seed + 100))
    net.eval()
    two = eval_errors(net, ref, x, H, W)
    fused = eval_errors(net.fuse_eval(), ref, x, H, W)
    print(f"{case} eval vs fp32 oracle: two-pass {two[0]:.3e} {two[1]:.3e} {two[2]:.3e} | fused {fused[0]:.3e} {fused[1]:.3e} {fused[2]:.3e}")
    assert_bars(case, fused)


def profile_counts(net, x):
    eng = net.engine()
    eng.profile = []
    with torch.no_grad():
        net(x)
    torch.cuda.synchronize()
    prof, eng.profile = eng.profile, None
    return collections.Counter(p[0] for p in prof), prof


def test_launch_program():
    torch.manual_seed(2)
    net = Yolov5Network(3, 10, widen_factor=0.25, deepen_factor=0.33).cuda().eval()
    x = torch.rand(2, 3, 96, 96, generator=torch.Generator().manual_seed(3)).cuda()
    eng = net.engine()
    n_units, with_res = len(eng.exec_units), sum(1 for u in eng.exec_units if u.residual)
    assert with_res > 0
    off, _ = profile_counts(net, x)
    assert dict(off) == {"conv_fwd": n_units, "bn_silu_apply": n_units}, off      # the two-pass program, as before
    on, prof = profile_counts(net.fuse_eval(), x)
    assert dict(on) == {"conv_fwd_fused": n_units}, on
    assert sorted(p[4] for p in prof) == sorted(u.name for u in eng.exec_units)
    # algorithmic bytes: 2 (in + out), + 2 out with a residual
    by_name = {p[4]: p[3] for p in prof}
    for u in eng.exec_units:
        st = eng.cur.units[u.name]
        in_elems = 2 * 96 * 96 * 3 if u.stem else 2 * st.H * st.W * u.cin
        assert by_name[u.name] == 2 * (in_elems + st.M * u.cout) + (2 * st.M * u.cout if u.residual else 0), u.name
    assert dict(profile_counts(net.fuse_eval(False), x)[0]) == dict(off)
    # a training forward never fuses, whatever the option says
    net.fuse_eval().train()
    eng.profile = []
    net.forward_raw(x)
    torch.cuda.synchronize()
    prof, eng.profile = eng.profile, None
    fams = collections.Counter(p[0] for p in prof)
    assert "conv_fwd_fused" not in fams and fams["conv_fwd"] == n_units, fams


def test_train_step_after_fused_eval_is_bit_equal():
    size, B, nc = 160, 4, 10
    x, _ = synth.batch(B, size, nc, 11)
    tg = synth.targets(B, size, nc, 11, nmin=1, nmax=9)
    targets = tuple(DetectionTarget(b, l) for b, l in tg)
    shape = FeatureShape(width=size, height=size)
    xe = torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(12)).cuda()
    got = []
    for fused in (False, True):
        torch.manual_seed(3)
        net = Yolov5Network(3, nc, widen_factor=0.25, deepen_factor=0.33).cuda()
        net.eval().fuse_eval(fused)
        with torch.no_grad():
            net(xe)
        net.train()
        total, lr = net.train_step(x.cuda(), _loss(), shape, targets, float(B))
        net.engine().wait_grads()
        torch.cuda.synchronize()
        got.append((total.detach().cpu(), torch.stack([lr.localization, lr.objectness, lr.classification]).detach().cpu(),
                    torch.cat([p.grad.flatten() for p in net.parameters()]).cpu(), net.engine().rm_arena.cpu(), net.engine().rv_arena.cpu()))
    assert torch.isfinite(got[1][2]).all() and got[1][2].abs().max() > 0
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_graphed_eval_forward():
    from object_detection_cib_amd.engine.graphed import GraphedEvalForward
    B, size, nc = 2, 160, 10
    net = trained(0.25, 0.33, nc, B, size, 21, steps=2)
    net.eval().fuse_eval()
    xs = [torch.rand(B, 3, size, size, generator=torch.Generator().manual_seed(30 + i)).cuda() for i in range(3)]
    shape = FeatureShape(width=size, height=size)

    def eager(x):
        with torch.no_grad():
            return get_detections(shape, net(x), ANCHORS).clone()

    gf = GraphedEvalForward(net, ANCHORS, B, size, size).capture(xs[0])
    for x in xs[:2]:
        assert torch.equal(gf(x), eager(x))
    # a parameter update between replays is picked up
    before = gf(xs[2]).clone()
    net.train()
    for p in net.parameters():
        p.grad = None
    x, tg = synth.batch(B, size, nc, 77)
    _step(net, x.cuda(), tg, size, B)
    net.engine().sgd_step((0.05, 0.01, 0.01), (0.8, 0.8, 0.8), (0.0, 5e-4, 0.0))
    net.eval()
    after = gf(xs[2]).clone()
    assert not torch.equal(after, before)
    assert torch.equal(after, eager(xs[2]))
    # the graph holds the launches of the form it was captured with
    net.fuse_eval(False)
    with pytest.raises(RuntimeError, match="eval_fused"):
        gf(xs[0])
    net.fuse_eval()
    assert torch.equal(gf(xs[0]), eager(xs[0]))


def test_submodule_front_end_csp_relu_residual():
    """A CSP layer with add_identity and ReLU (residual adds, the run-time activation switch) in eval mode against torch fp32,
    under the forward bar of tests/test_hip_modules.py::_compare (relL2 <= 1e-2 per output)."""
    from object_detection_cib_amd.nn.layers.csp import CSPLayer
    from test_hip_modules import _flat, _swap_activation
    x = torch.randn(4, 64, 24, 40, generator=torch.Generator().manual_seed(31))
    torch.manual_seed(32); hip = CSPLayer(64, 128, 0.5, True, 2, Yolov5BatchNorm2d, torch.nn.ReLU)
    torch.manual_seed(32); ref = _swap_activation(N.CSP(64, 128, 2, True), torch.nn.ReLU)
    g = torch.Generator().manual_seed(33)
    sd = ref.state_dict()
    for k, v in sd.items():                      # non-trivial running statistics and affine parameters
        if k.endswith("running_mean"):
            sd[k] = 0.5 * torch.randn(v.shape, generator=g)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith(".1.weight"):
            sd[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith(".1.bias"):
            sd[k] = 0.2 * torch.randn(v.shape, generator=g)
    assert list(hip.state_dict().keys()) == list(sd.keys())
    ref.load_state_dict(sd); hip.load_state_dict(sd)
    assert any(k.endswith("running_var") for k in sd) and hip._act[0] == 1
    ref.eval()
    hip = hip.cuda().eval()
    assert hip.fuse_eval() is hip
    with torch.no_grad():
        want = _flat(ref(x))[0]
        two = _flat(hip.fuse_eval(False)(x.cuda()))[0].cpu()
        eng = hip.engine()
        eng.profile = []
        got = _flat(hip.fuse_eval()(x.cuda()))[0].cpu()
        torch.cuda.synchronize()
        prof, eng.profile = eng.profile, None
    assert {p[0] for p in prof} == {"conv_fwd_fused"} and any(u.residual for u in eng.exec_units)
    print(f"CSP layer (ReLU, residual) eval vs torch fp32: two-pass {_rel(two, want):.3e} | fused {_rel(got, want):.3e}")
    assert got.shape == want.shape and _rel(got, want) <= 1e-2, _rel(got, want)
