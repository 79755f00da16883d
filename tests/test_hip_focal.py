"""The fused loss with YOLOv5's remaining hyper-parameters - Yolov5Loss(fl_gamma=, fl_alpha=, label_smoothing=,
obj_pos_weight=), the extended instantiations of loss_rows_kernel / loss_cells_kernel behind kodhip_yolo_loss_ex - against
the fp64 reference of tests/focal_reference.py, with the comparison scheme and the constructed cases of
tests/loss_reference.py (as tests/test_hip_loss_edges.py uses them for the default path).

Comparison: per level, per group (box / obj / cls), on matched and on unmatched cells, |kernel - fp64| <= K * E + floor with
E the fp32 CPU restatement's own max error on that group (`FR.oracle_fp32`: the yardstick is never the kernel) and floor =
FLOOR_ULPS fp32 ulps of the group's max |reference|; the three losses and the nine per-level means the same way.  Groups
whose reference is identically zero must be exactly zero.  K = 4, the project's constant.  Every figure is printed
before it is asserted (`pytest -s`).

What is new in the extended path and where it can go wrong: under focal modulation d loss / d target depends on the
cell's SURVIVING objectness target, so a row that is not its cell's last must evaluate it at the LAST row's clamp(iou, 0)
- which another thread of the same launch writes; the kernel recomputes it.  `crowded` (up to 17 rows per cell, IoU
differing per row) is that case: the box-slot gradients of its crowded cells are compared with fp64 like every other
group, and test_target_gradient_is_taken_at_the_last_rows_target recovers d loss / d t from them and shows that only the
last row's target explains it.

Option sets (gamma, alpha, smoothing, obj_pw): (1.5, .25, 0, 1), (2, .25, .1, .7), (1, .5, .1, 2), (0, .25, .1, 1) smoothing
alone, (0, .25, 0, 2) obj_pw alone - on all six constructed cases and both routes with ciou / 1e-7; `crowded` and `ties`
again with giou (the dual-number row); `crowded` and `saturated_nc80` with per-class pos_weight; four sweep cases.

Measured on an MI355X with K = 4 and the 4-ulp floor (the project's constants, nothing raised), max over levels, groups,
routes, option sets, IoU kinds and weightings of  kernel error / E  and  kernel error / (K E + floor):

    ties             3.34  0.42      nc1_b1_96x96       5.92  0.43
    crowded         10.97  0.92      nc7_b3_160x160     9.76  0.47
    saturated nc 3  27.28  0.69      nc59_b2_160x96     1.82  0.29
    saturated nc 80 11.86  0.32      nc123_b3_160x160   1.89  0.30
    empty level      3.14  0.32
    empty batch      2.24  0.25

As on the default path the ratios above 4 belong to scalars and to groups of a few elements whose E is far below one fp32
ulp of the value (the floor's purpose): the largest share of a tolerance is 0.92 (crowded, smoothing alone, giou: the 5 x 5
level's objectness slots on matched cells).  The guard-band share was 0 in every case.  The last-row recovery agrees to
1.8e-11 where another row's target would be off by 1.7e-6 (tolerance 3.7e-9, first cell).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import focal_reference as FR  # noqa: E402
import loss_reference as R  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402
from object_detection_cib_amd.core.bbox.iou import IoUCalculator  # noqa: E402
from object_detection_cib_amd.core.label_assignment.yv5 import Yolov5LabelAssigner, AssignmentAnchorInfo  # noqa: E402
from object_detection_cib_amd.data.detection import DetectionTarget  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline import loss as loss_mod  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.loss import Yolov5Loss, Yolov5LossParams  # noqa: E402

K = 4
OPTS = FR.OPTION_SETS
OPT_IDS = ["g1.5", "g2_s.1_opw.7", "g1_a.5_s.1_opw2", "s.1", "opw2"]


def _loss(opt=None, kind="ciou", eps=1e-7, pw=None, **kw):
    asg = Yolov5LabelAssigner(AssignmentAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32)), 4.0)
    if opt is not None:
        kw = dict(fl_gamma=opt.gamma, fl_alpha=opt.alpha, label_smoothing=opt.smoothing, obj_pos_weight=opt.obj_pw)
    return Yolov5Loss(asg, Yolov5LossParams.get_default(), IoUCalculator(kind, eps), pw, **kw)


def _targets(case):
    return tuple(DetectionTarget(b, l) for b, l in case.targets)


def _autograd(case, mod):
    """forward + autograd backward of B * (loc + cls + obj): (losses [3], grads)"""
    B = case.raws[0].shape[0]
    raws = [r.cuda().requires_grad_(True) for r in case.raws]
    res = mod(FeatureShape(width=case.width, height=case.height),
              tuple((r[..., :4], r[..., 4:5], r[..., 5:]) for r in raws), _targets(case))
    (B * (res.localization + res.classification + res.objectness)).backward()
    return torch.stack([res.localization, res.objectness, res.classification]).detach().cpu(), [r.grad.cpu() for r in raws]


def _single_pass(case, mod):
    """the training step's route: values and gradients in one pass, upstream = (B, B, B)"""
    B = case.raws[0].shape[0]
    res, grads = mod.value_and_grad(FeatureShape(width=case.width, height=case.height), [r.cuda() for r in case.raws],
                                    _targets(case), upstream=(float(B),) * 3)
    return torch.stack([res.localization, res.objectness, res.classification]).cpu(), [g.cpu() for g in grads]


ROUTES = {"autograd": _autograd, "single_pass": _single_pass}


def _scalar_ok(tag, got, ref, yard):
    got, ref, yard = float(got), float(ref), float(yard)
    if ref != ref:
        print(f"FOCAL {tag} got {got} ref nan")
        return got != got
    E = abs(yard - ref)
    floor = R.FLOOR_ULPS * R.ulp32(ref) if ref != 0 else 0.0
    err = abs(got - ref)
    print(f"FOCAL {tag} err {err:.3e} E {E:.3e} ref {ref:.6e} err/E {err / E if E else float('inf'):.2f} "
          f"err/tol {err / (K * E + floor) if K * E + floor else 0.0:.3f}")
    return err <= K * E + floor


def _compare(tag, case, ref, yard, losses, grads):
    """every figure printed, then asserted together"""
    l32, _, g32, _ = yard
    drop, share = R.band_cells(ref, R.constructed_rows(case, ref) if case.constructed else None)
    print(f"FOCAL {tag} guard-band share {share:.5f}")
    assert share <= R.BAND_SHARE
    bad = []
    for i, nm in enumerate(("localization", "objectness", "classification")):
        if not _scalar_ok(f"{tag} {nm}", losses[i], ref.losses[i], l32[i]):
            bad.append(nm)
    for g in grads:
        assert bool(torch.isfinite(g).all()), tag
    worst = 0.0
    for lvl, nm, where, err, E, mx, floor in R.group_report(grads, ref, g32, drop):
        tol = K * E + floor
        worst = max(worst, err / E if E else 0.0)
        print(f"FOCAL {tag} {lvl} {nm} {where} err {err:.3e} E {E:.3e} max {mx:.3e} err/E {err / E if E else 0.0:.2f} "
              f"err/tol {err / tol if tol else 0.0:.3f}")
        if not err <= tol:
            bad.append((lvl, nm, where, err, E, mx))
    print(f"FOCAL {tag} worst err/E {worst:.2f}")
    assert not bad, (tag, bad)


_refs = {}


def _reference(name, iopt, weighted, kind):
    """fp64 reference and fp32 yardstick of one (case, options, weighting, IoU kind): computed once, shared, not modified"""
    key = (name, iopt, weighted, kind)
    if key not in _refs:
        case = R.cases()[name]()
        pw = R.pos_weight_for(case.nc) if weighted else None
        ref = FR.reference(case, OPTS[iopt], pw, kind, 1e-7)
        ev = R.events(case, ref)
        for e in R.expected_events(case, kind, 1e-7):            # a fixture that stops producing its event must fail
            assert ev[e] > 0, (name, kind, e, ev)
        _refs[key] = (case, pw, ref, FR.oracle_fp32(case, OPTS[iopt], pw, kind, 1e-7))
    return _refs[key]


def _run_case(name, iopt, route, weighted=False, kind="ciou"):
    case, pw, ref, yard = _reference(name, iopt, weighted, kind)
    mod = _loss(OPTS[iopt], kind, 1e-7, pw)
    tag = f"{name} {OPT_IDS[iopt]} {kind} {'pw' if weighted else 'nopw'} {route}"
    losses, grads = ROUTES[route](case, mod)
    _compare(tag, case, ref, yard, losses, grads)
    losses2, grads2 = ROUTES[route](case, mod)                   # bit-for-bit repeatable
    assert torch.equal(losses.view(torch.int32), losses2.view(torch.int32)), tag
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(grads, grads2)), tag


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("iopt", range(len(OPTS)), ids=OPT_IDS)
@pytest.mark.parametrize("name", FR.CONSTRUCTED)
def test_constructed_cases_vs_fp64(name, iopt, route):
    _run_case(name, iopt, route)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("iopt", range(len(OPTS)), ids=OPT_IDS)
@pytest.mark.parametrize("name", ["crowded", "ties"])
def test_dual_number_route_vs_fp64(name, iopt, route):
    """giou: value and box derivatives from the dual-number row, the target gradient through the recomputed last-row value"""
    _run_case(name, iopt, route, kind="giou")


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("iopt", [0, 1], ids=OPT_IDS[:2])
@pytest.mark.parametrize("name", ["crowded", "saturated_nc80"])
def test_per_class_pos_weight_vs_fp64(name, iopt, route):
    _run_case(name, iopt, route, weighted=True)


@pytest.mark.parametrize("name,iopt", [(n, i) for n, s in FR.SWEEP.items() for i in s])
def test_class_counts_and_ragged_chunks_vs_fp64(name, iopt):
    for route in ROUTES:
        _run_case(name, iopt, route, weighted=iopt % 2 == 1)


def test_target_gradient_is_taken_at_the_last_rows_target():
    """Crowded cells whose rows have different IoU, options (1.5, .25, 0, 1).  Every row r of a cell
    adds  [iou_r >= 0] * (k_box + k_obj * dL/dt(x_obj, t_last)) * d iou_r / d logits  to the cell's box slots, with ONE
    cell-wide dL/dt.  From the fp64 reference rows: the kernel's box-slot gradient agrees with the sum that uses the last
    row's target and disagrees, by far more than the agreement, with the sum that uses any other row's."""
    import numpy as np
    opt = OPTS[0]
    case = R.crowded_case()
    B = case.raws[0].shape[0]
    ref = FR.reference(case, opt)
    _, grads = _single_pass(case, _loss(opt))
    checked = 0
    for li, (rd, raw, g, a) in enumerate(zip(ref.rows, case.raws, grads, ref.asg)):
        if li != 0:
            continue
        ncells = raw[..., 0].numel()
        m = rd.cell.numel()
        k_obj = B * (case.width / 640) ** 2 * (4.0, 1.0, 0.4)[li] / ncells
        k_box = -B * 0.05 / m
        x4 = raw.reshape(-1, raw.shape[-1])[:, :5].double()
        gbox = g.reshape(-1, g.shape[-1])[:, :4].double()
        for cell in torch.unique(rd.cell[rd.rows_per_cell > 8]).tolist():
            rows = (rd.cell == cell).nonzero().reshape(-1)
            t_rows = rd.iou[rows].clamp(0)
            if (t_rows[-1] - t_rows[:-1]).abs().min() < 1e-3:
                continue
            # d iou_r / d box logits of every row of the cell, by autograd on the reference's own functions
            p = x4[cell, :4].clone().requires_grad_(True)
            pxy = p[:2].sigmoid() * 2 - 0.5
            pwh = (p[2:4].sigmoid() * 2) ** 2 * a.anchors[rows].double()
            pred = R.D._to_xyxy(torch.cat((pxy.expand(rows.numel(), 2), pwh), 1))
            iou = R.D.iou_family(pred, R.D._to_xyxy(a.gt_boxes[rows].double()), "ciou", 1e-7).reshape(-1)
            J = torch.stack([torch.autograd.grad(iou[i], p, retain_graph=True)[0] for i in range(rows.numel())])
            gate = (iou.detach() >= 0).double()
            xo = np.array([x4[cell, 4].item()])

            def predicted(t):
                dt = FR.closed_forms(xo, np.array([float(t)]), opt.obj_pw, opt.gamma, opt.alpha)[2][0]
                up = k_box + gate * k_obj * dt
                return (up[:, None] * J).sum(0), (up.abs()[:, None] * J.abs()).sum(0).max().item()
            want, scale = predicted(t_rows[-1])
            # fp32 kernel against an fp64 sum of up to 17 terms of ~30 rounded operations each: 1e-5 of the terms' magnitude
            tol = 1e-5 * scale
            e_last = (gbox[cell] - want).abs().max().item()
            e_other = min((gbox[cell] - predicted(t)[0]).abs().max().item() for t in t_rows[:-1])
            print(f"FOCAL last-row cell {cell}: |g - sum(t_last)| {e_last:.3e}  min over other rows {e_other:.3e}  tol {tol:.3e}")
            assert e_last <= tol, (cell, e_last, tol)
            assert e_other > 10 * tol, (cell, e_other, tol)         # another row's target would be visible
            checked += 1
    assert checked >= 3


# ---------------------------------------------------------------- direct runs
def _direct(case, mod, G=4096):
    """One pass of the kernels as the wrapper runs them (loss._run), with the logits and the gradients inside larger
    poisoned buffers and the kernel's own output block visible: (out [16], grads, guards intact?, error)"""
    dev = torch.device("cuda")
    shape = FeatureShape(width=case.width, height=case.height)
    asg, cap = mod.assigner.assign_device(shape, _targets(case), dev)
    B, A, _, _, P = case.raws[0].shape
    raws, grads, gbufs = [], [], []
    for r in case.raws:
        n = r.numel()
        lb = torch.full((n + 2 * G,), float("nan"), device=dev)
        lb[G:G + n] = r.reshape(-1).cuda()
        raws.append(lb[G:G + n].view(r.shape))
        gb = torch.full((n + 2 * G,), -7.0, device=dev)
        gbufs.append(gb)
        grads.append(gb[G:G + n].view(r.shape))
    nslots = max((cap + 255) // 256, 1024)
    work = dict(maps=[torch.empty(3 * t[..., 0].numel(), dtype=torch.int32, device=dev) for t in raws],
                prev=[torch.empty(cap, dtype=torch.int32, device=dev) for _ in raws],
                rowgrad=[torch.empty(cap * (P - 1), dtype=torch.float32, device=dev) for _ in raws],
                tobj=[torch.empty(cap, dtype=torch.float32, device=dev) for _ in raws],
                partials=torch.empty(9 * nslots, dtype=torch.float32, device=dev), nslots=nslots,
                out=torch.full((16,), -7.0, dtype=torch.float32, device=dev))
    up = torch.full((3,), float(B), device=dev)
    err = None
    try:
        loss_mod._run(mod, shape, raws, asg, cap, grads, up, work)
    except RuntimeError as e:
        err = str(e)
    torch.cuda.synchronize()
    intact = all(bool((gb[:G] == -7.0).all()) and bool((gb[-G:] == -7.0).all()) for gb in gbufs)
    return work["out"].cpu(), [g.cpu() for g in grads], intact, err


@pytest.mark.parametrize("name,iopt", [("nc1_b1_96x96", 0), ("nc123_b3_160x160", 0), ("empty_level", 1), ("empty_batch", 1),
                                       ("crowded", 1)])
def test_guard_bands_and_level_means(name, iopt):
    """The extended path writes nothing before or after the gradient tensors (4096 poisoned floats either side), writes
    every element inside, its nine per-level means agree with fp64 (NaN box / class mean on a level without rows), and
    a second run gives the same bits."""
    case, pw, ref, yard = _reference(name, iopt, False, "ciou")
    out, grads, intact, err = _direct(case, _loss(OPTS[iopt]))
    assert err is None, err
    assert intact, "the loss kernels wrote outside a gradient tensor"
    for g in grads:
        assert not bool((g == -7.0).any()), "a gradient element was left unwritten"
    _compare(f"{name} {OPT_IDS[iopt]} direct", case, ref, yard, out[:3], grads)
    bad = []
    for li, lvl in enumerate(R.LEVELS):
        for j, nm in enumerate(("box", "obj", "cls")):
            if not _scalar_ok(f"{name} mean {lvl} {nm}", out[3 + 3 * li + j], ref.means[li, j], yard[3][li, j]):
                bad.append((lvl, nm))
    assert not bad, bad
    out2, grads2, _, _ = _direct(case, _loss(OPTS[iopt]))
    assert torch.equal(out[:13].view(torch.int32), out2[:13].view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(grads, grads2))


@pytest.mark.parametrize("vals,word", [((-1.0, .25, 1, 0, 1), "fl_gamma"), ((0.5, .25, 1, 0, 1), "fl_gamma"),
                                       ((1.5, 1.0, 1, 0, 1), "fl_alpha"), ((0, .25, 0.5, 0, 1), "cls_pos"),
                                       ((0, .25, 1, 0.5, 1), "cls_neg"), ((1.5, .25, 1, 0, 0.0), "obj_pos_weight")])
def test_bad_options_refused_without_a_launch(vals, word):
    """kodhip_yolo_loss_ex validates the options itself (a caller may bypass the constructor): a status and a message,
    and nothing ran - the gradient buffers and the output block keep their poison."""
    case = R.random_case(1, 96, 96, 3, seed=3)
    mod = _loss(OPTS[0])
    mod._options = _lib.KodLossOptions(*vals)
    out, grads, intact, err = _direct(case, mod)
    assert err is not None and word in err, err
    assert intact and all(bool((g == -7.0).all()) for g in grads) and bool((out == -7.0).all())


# ---------------------------------------------------------------- equalities with the default path
@pytest.mark.parametrize("name", ["crowded", "nc7_b3_160x160"])
def test_neutral_keywords_are_the_default_path(name):
    """Yolov5Loss(..., fl_gamma=0, fl_alpha=<any>, label_smoothing=0, obj_pos_weight=1) makes the default call: losses and
    gradients equal those of a loss built without keywords bit for bit, on both routes; and the raw entry point with
    opt = NULL, or with a neutral options block, equals kodhip_yolo_loss_iou."""
    case = R.cases()[name]()
    pw = R.pos_weight_for(case.nc)
    plain = Yolov5Loss(_loss().assigner, Yolov5LossParams.get_default(), IoUCalculator("ciou", 1e-7), pw)
    neutral = _loss(None, pw=pw, fl_gamma=0.0, fl_alpha=0.6, label_smoothing=0.0, obj_pos_weight=1.0)
    for fn in ROUTES.values():
        (l0, g0), (l1, g1) = fn(case, plain), fn(case, neutral)
        assert torch.equal(l0.view(torch.int32), l1.view(torch.int32))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(g0, g1))
    base = _direct(case, plain)
    # a null options pointer / a neutral block through kodhip_yolo_loss_ex itself
    for o in (C.POINTER(_lib.KodLossOptions)(), _lib.KodLossOptions(0.0, 0.6, 1.0, 0.0, 1.0)):
        plain._options = o
        got = _direct(case, plain)
        assert got[3] is None and got[2]
        assert torch.equal(base[0][:13].view(torch.int32), got[0][:13].view(torch.int32))
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(base[1], got[1]))
    plain._options = None


def test_options_change_the_result():
    """(the equalities above are not vacuous: a non-neutral option moves every loss it touches)"""
    case = R.cases()["nc7_b3_160x160"]()
    l0, _ = _single_pass(case, _loss())
    for opt, moved in ((OPTS[0], (1, 2)), (OPTS[3], (2,)), (OPTS[4], (1,))):
        l1, _ = _single_pass(case, _loss(opt))
        for i in moved:
            assert l0[i] != l1[i], (opt, i, l0, l1)


# ---------------------------------------------------------------- training routes
def _net_setup(opt):
    from oracle import synth
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    S, B, nc = 160, 4, 10
    torch.manual_seed(3)
    net = Yolov5Network(3, nc, widen_factor=0.25, deepen_factor=0.33).cuda().train()
    x, _ = synth.batch(B, S, nc, 11)
    tg = tuple(DetectionTarget(b, l) for b, l in synth.targets(B, S, nc, 11, nmin=1, nmax=9))
    return net, _loss(opt), x.cuda(), tg, S, B


def test_train_step_equals_autograd_route():
    """net.train_step with a focal loss (one pass of the extended kernels through value_and_grad) equals net(x) ->
    loss(...) -> backward() (two passes): every loss value and every parameter gradient bit for bit."""
    got = []
    for route in ("autograd", "direct"):
        net, loss, x, tg, S, B = _net_setup(OPTS[1])
        shape = FeatureShape(width=S, height=S)
        if route == "autograd":
            lr = loss(shape, net(x), tg)
            total = B * (lr.localization + lr.classification + lr.objectness)
            total.backward()
        else:
            total, lr = net.train_step(x, loss, shape, tg, float(B))
        net.engine().wait_grads()
        torch.cuda.synchronize()
        got.append((total.detach().cpu(), torch.stack([lr.localization, lr.objectness, lr.classification]).detach().cpu(),
                    torch.cat([p.grad.flatten() for p in net.parameters()]).cpu()))
    a, d = got
    assert torch.equal(a[0], d[0]) and torch.equal(a[1], d[1]), (a[:2], d[:2])
    assert bool(torch.isfinite(d[2]).all()) and d[2].abs().max() > 0
    assert torch.equal(a[2], d[2])
    # ... and it is the focal loss that ran: the default loss on the same network state gives other values
    net, _, x, tg, S, B = _net_setup(OPTS[1])
    total0, _ = net.train_step(x, _loss(), FeatureShape(width=S, height=S), tg, float(B))
    assert total0.item() != d[0].item()


def test_graphed_step_equals_eager_steps():
    """GraphedTrainStep capture + two replays equals two eager train_step + SGD steps with the same focal loss: the
    options are baked into the captured kernel arguments.  Parameters, momentum and losses bit for bit."""
    from object_detection_cib_amd.engine.graphed import GraphedTrainStep
    lr, mom, wd = (0.02, 0.02, 0.02), (0.9,) * 3, (0.0, 5e-4, 0.0)
    runs = []
    for graphed in (False, True):
        net, loss, x, tg, S, B = _net_setup(OPTS[1])
        eng = net.engine()
        totals = []
        if graphed:
            step = GraphedTrainStep(net, loss, B, S, S, max_targets=256)
            eng.set_hyper(lr, mom, wd)
            step.capture(x, tg)
            for _ in range(2):
                t, _parts = step(x, tg, lr, mom, wd)
                totals.append(t.item())
        else:
            for _ in range(2):
                for p in net.parameters():
                    p.grad = None
                t, _parts = net.train_step(x, loss, FeatureShape(width=S, height=S), tg, float(B))
                eng.sgd_step(lr, mom, wd)
                totals.append(t.item())
        torch.cuda.synchronize()
        runs.append((totals, eng.p_arena.clone(), eng.m_arena.clone()))
    assert all(t == t for t in runs[0][0]) and runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
