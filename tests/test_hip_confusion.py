"""kodhip_confusion_match (csrc/confusion.hip), DeviceConfusionMatrix and DefaultYolov5Experiment(val_confusion=True)
against the plain reference of tests/confusion_reference.py.  Every comparison is integer equality of whole matrices: the
inputs sit on a 1/4-pixel lattice (see the reference's docstring), so there is nothing to tolerate.  That the inputs reach
ties, lost detections, off-diagonal matches and both sides of the kernel's on-chip / direct-atomic switch-over is asserted on
the CPU (tests/test_confusion_reference.py)."""
import inspect

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import confusion_reference as R  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.label_assignment.yv5 import BatchedTargets  # noqa: E402
from object_detection_cib_amd.data.detection import DetectionTarget  # noqa: E402
from object_detection_cib_amd.lightning.callbacks.confusion import DeviceConfusionMatrix  # noqa: E402

GUARD = 64
POISON = 0x5A5A5A5A5A5A5A5A
HAND = R.hand_cases()
RANDOM = R.random_cases()
_WANT = {}


def _want(name):
    """the reference matrix of a case, computed once"""
    if name not in _WANT:
        c = {**HAND, **RANDOM}[name]
        _WANT[name] = R.confusion_ref(c.dets, c.gts, c.nc, c.conf, c.iou)
    return _WANT[name]


def _preload(nc):
    return (np.arange((nc + 1) ** 2, dtype=np.int64) % 7 + 1) * 1000


def _launch(det, nd, gt, lab, start, nc, conf, iou, matrix=None):
    """kodhip_confusion_match with the test's own buffers.  The matrix sits between two guards of 64 poisoned int64 words and
    is pre-loaded with a non-zero pattern -> (what the launch added [nc+1, nc+1], guards intact)"""
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()           # noqa: E731
    d, n_, s_ = dv(det), dv(nd), dv(start)
    g, l = (dv(gt), dv(lab)) if len(lab) else (None, None)
    cells = (nc + 1) ** 2
    buf = torch.full((cells + 2 * GUARD,), POISON, dtype=torch.int64, device="cuda")
    pre = _preload(nc)
    buf[GUARD:GUARD + cells] = torch.from_numpy(pre).cuda()
    B, max_det, _ = det.shape
    _lib.check(_lib.lib().kodhip_confusion_match(d.data_ptr(), n_.data_ptr(), g.data_ptr() if g is not None else None,
                                                 l.data_ptr() if l is not None else None, s_.data_ptr(),
                                                 buf[GUARD:].data_ptr(), B, max_det, nc, conf, iou, stream()), "confusion_match")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    intact = bool((host[:GUARD] == POISON).all() and (host[-GUARD:] == POISON).all())
    return (host[GUARD:GUARD + cells] - pre).reshape(nc + 1, nc + 1), intact


def _padded(det, nd, max_det=1024):
    """the same batch in a [B, 1024, 6] buffer whose rows beyond ndet hold boxes that WOULD count if they were read"""
    B = det.shape[0]
    out = np.empty((B, max_det, 6), np.float32)
    out[:] = np.array([0, 0, 1000, 1000, 0.99, 0], np.float32)
    for b in range(B):
        out[b, :nd[b]] = det[b, :nd[b]]
    return out


def _check(name, case, want):
    det, nd, gt, lab, start = R.pack(case.dets, case.gts)
    for tag, dd in (("tight", det), ("padded to 1024", _padded(det, nd))):
        got, intact = _launch(dd, nd, gt, lab, start, case.nc, case.conf, case.iou)
        assert intact, f"{name} {tag}: written outside the matrix"
        np.testing.assert_array_equal(got, want, err_msg=f"{name} {tag}")


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases_single_image(name):
    case = HAND[name]
    want = R.expected_matrix(case)
    np.testing.assert_array_equal(_want(name), want)
    assert len(case.dets) == 1
    _check(name, case, want)


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_random_scenes_sixteen_images(name):
    case = RANDOM[name]
    assert len(case.dets) == 16
    _check(name, case, _want(name))


def test_detection_count_beyond_the_buffer_is_clamped():
    """ndet announces all eight detections of case E, the buffer holds the first four"""
    case = HAND["E_300_ground_truths"]
    det, nd, gt, lab, start = R.pack(case.dets, case.gts)
    assert int(nd[0]) == 8
    want = R.confusion_ref([case.dets[0][:4]], case.gts, case.nc, case.conf, case.iou)
    got, intact = _launch(np.ascontiguousarray(det[:, :4]), nd, gt, lab, start, case.nc, case.conf, case.iou)
    assert intact
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", ["nc5", "nc200"])
def test_two_half_launches_equal_one(name):
    case = RANDOM[name]
    halves = []
    for sl in (slice(0, 8), slice(8, 16)):
        got, intact = _launch(*R.pack(case.dets[sl], case.gts[sl]), case.nc, case.conf, case.iou)
        assert intact
        halves.append(got)
    np.testing.assert_array_equal(halves[0] + halves[1], _want(name))


@pytest.mark.parametrize("name", ["lattice8", "nc81"])
def test_ten_repeats_are_identical(name):
    case = RANDOM[name]
    packed = R.pack(case.dets, case.gts)
    runs = [_launch(*packed, case.nc, case.conf, case.iou)[0] for _ in range(10)]
    for r in runs:
        np.testing.assert_array_equal(r, _want(name))


def _targets(gts):
    return tuple(DetectionTarget(torch.from_numpy(np.asarray(g, dtype=np.float64).reshape(-1, 4)), torch.from_numpy(l)) for g, l in gts)


@pytest.mark.parametrize("batched", [False, True], ids=["DetectionTarget", "BatchedTargets"])
def test_device_confusion_matrix_accumulates_batches(batched):
    nc = 5
    batches = R.evaluator_cases(nc)
    want = sum(R.confusion_ref(d, g, nc) for d, g in batches)
    assert want[:nc, :nc].sum() > 0 and want[nc].sum() > 0 and want[:, nc].sum() > 0
    cm = DeviceConfusionMatrix(nc)
    for dets, gts in batches:
        tg = _targets(gts)
        if batched:
            tg = BatchedTargets.from_targets(tg, torch.device("cuda"))
        cm.add_batch(tg, [torch.from_numpy(d).cuda() for d in dets])
    got = cm.matrix()
    assert got.dtype == np.int64 and got.shape == (nc + 1, nc + 1)
    np.testing.assert_array_equal(got, want)
    pc = cm.per_class()
    np.testing.assert_array_equal(pc["missed"], want[nc, :nc])
    np.testing.assert_array_equal(pc["background_fp"], want[:nc, nc])
    cm.reset()
    assert not cm.matrix().any()
    cm.add_batch(_targets(batches[0][1]), [torch.from_numpy(d).cuda() for d in batches[0][0]])
    np.testing.assert_array_equal(cm.matrix(), R.confusion_ref(*batches[0], nc))


def test_packed_nms_output_is_used_in_place():
    """non_max_suppression hands out views of one [B, 300, 6] buffer together with that buffer and the device-side counts:
    add_batch passes them on, rows beyond each image's count (here: boxes that would count) are never read"""
    from object_detection_cib_amd.core.nms import PackedDetections
    case = RANDOM["nc5"]
    det, nd, *_ = R.pack(case.dets, case.gts)
    packed = torch.from_numpy(_padded(det, nd, 300)).cuda()
    views = PackedDetections([packed[b, :int(n)] for b, n in enumerate(nd)], packed, torch.from_numpy(nd).cuda())
    assert isinstance(views, list) and len(views) == 16 and views[3].shape == (int(nd[3]), 6)
    cm = DeviceConfusionMatrix(case.nc)
    cm.add_batch(_targets(case.gts), views)
    np.testing.assert_array_equal(cm.matrix(), _want("nc5"))
    cm.reset()
    cm.add_batch(_targets(case.gts), list(views))                  # a plain list of the same tensors: packed by add_batch
    np.testing.assert_array_equal(cm.matrix(), _want("nc5"))


def _experiment(graphed):
    from object_detection_cib_amd.core.anchors.info import voc_anchor_info
    from object_detection_cib_amd.core.bbox.iou import IoUCalculator
    from object_detection_cib_amd.core.label_assignment.yv5 import Yolov5LabelAssigner, AssignmentAnchorInfo
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.loss import Yolov5Loss, Yolov5LossParams
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    sig = inspect.signature(DefaultYolov5Experiment.__init__).parameters
    assert sig["val_confusion"].default is False and sig["val_confusion"].kind is inspect.Parameter.KEYWORD_ONLY
    assert (sig["val_confusion_conf"].default, sig["val_confusion_iou"].default) == (0.25, 0.45)
    nc = 4
    torch.manual_seed(3)
    net = Yolov5Network(3, nc, widen_factor=0.25, deepen_factor=0.33)
    with torch.no_grad():                                  # raised head biases: scores around 0.5 x 0.5, on both sides of 0.25
        for name, p in net.named_parameters():
            if name.endswith("obj_head.conv.bias"):
                p.fill_(0.0)
            elif name.endswith("cls_head.conv.bias"):
                p.fill_(0.0)
    net = net.cuda().eval()
    infos = (voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
    loss = Yolov5Loss(Yolov5LabelAssigner(AssignmentAnchorInfo(*infos), 4.0), Yolov5LossParams.get_default(),
                      IoUCalculator("ciou", 1e-7), None)
    exp = DefaultYolov5Experiment(net, loss, LayerwiseAnchorInfo(*infos), graphed=graphed, val_confusion=True)
    rng = np.random.default_rng(5)
    batches = []
    for _ in range(2):
        x = torch.from_numpy(rng.uniform(0, 1, (2, 3, 64, 64)).astype(np.float32)).cuda()
        tg = []
        for _ in range(2):
            n = int(rng.integers(1, 5))
            c = rng.integers(8, 56, (n, 2)).astype(np.float64); wh = rng.integers(4, 24, (n, 2)).astype(np.float64)
            tg.append(DetectionTarget(torch.from_numpy(np.concatenate((c - wh / 2, c + wh / 2), 1)),
                                      torch.from_numpy(rng.integers(0, nc, n).astype(np.int64))))
        batches.append((x, tuple(tg), None))
    return exp, batches, nc


@pytest.mark.parametrize("graphed", [True, False], ids=["graphed", "eager"])
def test_experiment_reports_confusion_next_to_unchanged_map(graphed):
    exp, batches, nc = _experiment(graphed)
    names = ["a", "b", "c", "d"]
    with_cm = exp.validate(batches, nc, names)
    cm = exp.confusion
    assert isinstance(cm, DeviceConfusionMatrix) and (cm.conf_thres, cm.iou_thres) == (0.25, 0.45)
    got = cm.matrix()
    exp.val_confusion = False
    plain = exp.validate(batches, nc, names)
    assert exp.confusion is cm                                     # a run without the feature leaves the last matrix readable
    extra = {f"{k}_{n}" for k in ("precision", "recall") for n in names}
    assert set(with_cm) == set(plain) | extra and not set(plain) & extra
    for k in plain:
        assert with_cm[k] == plain[k] or (np.isnan(with_cm[k]) and np.isnan(plain[k])), k
    pairs = [exp.validation_step(b) for b in batches]
    from object_detection_cib_amd.core.nms import PackedDetections
    assert all(isinstance(d, PackedDetections) and d.packed.shape == (2, 300, 6) for _, d in pairs)
    ev = {}
    want = np.zeros((nc + 1, nc + 1), np.int64)
    for targets, dets in pairs:
        want += R.confusion_ref([d.cpu().numpy() for d in dets], [(t.boxes.numpy(), t.labels.numpy()) for t in targets], nc, events=ev)
    print(f"CONFUSION experiment graphed={graphed} events {ev}")
    assert ev["matched"] + ev["bg_fp"] > 0, "no detection above 0.25: the input does not reach the kernel's counting"
    np.testing.assert_array_equal(got, want)
    pc = cm.per_class()
    for c, n in enumerate(names):
        for k in ("precision", "recall"):
            assert with_cm[f"{k}_{n}"] == pc[k][c] or (np.isnan(with_cm[f"{k}_{n}"]) and np.isnan(pc[k][c]))
