"""kodhip_val_match / kodhip_val_append / kodhip_val_curves (csrc/val_metrics.hip), DeviceDetectionMetrics and
DefaultYolov5Experiment(val_metrics=True) against the plain reference of tests/val_metrics_reference.py.
The matcher is compared for equality - masks, record order, scores, nt: the inputs sit on a 1/4-pixel lattice (see the
reference's docstring).  The curves are compared at 1e-12 absolute: values in [0, 1] out of under ten correctly rounded fp64
operations and a 101-term sum, so the true error is a few 1e-16 and the margin only covers the order of that sum; n_p and nt
are exact, and since the tail is shared code the reported index must then be the same.  That the inputs reach ties, holes,
lost detections and the sizes they were built for is asserted on the CPU (tests/test_val_metrics_reference.py)."""
import inspect

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import val_metrics_reference as R  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.label_assignment.yv5 import BatchedTargets  # noqa: E402
from object_detection_cib_amd.data.detection import DetectionTarget  # noqa: E402
from object_detection_cib_amd.lightning.callbacks.val_metrics import DeviceDetectionMetrics, summarize  # noqa: E402

GUARD = 64
POISON = 0x5A5A5A5A
TOL = 1e-12
HAND = R.hand_cases()
SHAPES = R.shape_cases()
CURVES = R.curve_cases()
_CACHE = {}


def _batch(nc, seed, thrs_name="IOUS10"):
    """a 16-image random batch and its reference records, computed once"""
    key = (nc, seed, thrs_name)
    if key not in _CACHE:
        case = R.random_batch(nc, seed, thrs=getattr(R, thrs_name))
        _CACHE[key] = (case, R.process(case.dets, case.gts, case.nc, case.thrs))
    return _CACHE[key]


class _Store:
    """a record store of the test's own: `cap` records between two guards of poisoned words, count and nt on the device"""

    def __init__(self, nc, cap):
        self.nc, self.cap = nc, cap
        self.buf = torch.full((cap + 2 * GUARD, 2), POISON, dtype=torch.int32, device="cuda")
        self.count = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.nt = torch.zeros(nc, dtype=torch.int64, device="cuda")

    def match(self, case, sl=slice(None), max_det=None, padded=False):
        sub = R.MatchCase(case.nc, case.thrs, case.dets[sl], case.gts[sl])
        det, nd, gt, lab, start = R.pack(sub, max_det)
        if padded:                      # rows beyond ndet hold boxes that WOULD count if they were read
            full = np.empty((det.shape[0], 1024, 6), np.float32)
            full[:] = np.array([0, 0, 1000, 1000, 0.99, 0], np.float32)
            for b in range(det.shape[0]):
                full[b, :nd[b]] = det[b, :nd[b]]
            det = full
        dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()           # noqa: E731
        d, n_, s_ = dv(det), dv(nd), dv(start)
        g, l = (dv(gt), dv(lab)) if len(lab) else (None, None)
        B, md, _ = det.shape
        offsets = torch.empty(B, dtype=torch.int32, device="cuda")
        thr = np.ascontiguousarray(case.thrs, dtype=np.float64)
        import ctypes as C
        _lib.check(_lib.lib().kodhip_val_match(d.data_ptr(), n_.data_ptr(), g.data_ptr() if g is not None else None,
                                               l.data_ptr() if l is not None else None, s_.data_ptr(),
                                               thr.ctypes.data_as(C.POINTER(C.c_double)), len(thr), self.buf[GUARD:].data_ptr(),
                                               self.count.data_ptr(), self.cap, self.nt.data_ptr(), offsets.data_ptr(), B, md,
                                               case.nc, stream()), "val_match")
        torch.cuda.synchronize()

    def read(self):
        """-> (scores, classes, masks, nt); asserts that nothing outside the first `count` records was written"""
        host = self.buf.cpu().numpy().view(np.uint32)
        n = int(self.count.item())
        assert 0 <= n <= self.cap
        assert (host[:GUARD] == POISON).all() and (host[GUARD + n:] == POISON).all(), "written outside the records"
        rec = host[GUARD:GUARD + n]
        return (rec[:, 0].copy().view(np.float32), (rec[:, 1] & 0xFFFF).astype(np.int64), (rec[:, 1] >> 16).astype(np.int64),
                self.nt.cpu().numpy())


def _same_records(got, want, msg=""):
    for g, w, what in zip(got, want, ("scores", "classes", "masks", "nt")):
        np.testing.assert_array_equal(g, w, err_msg=f"{msg} {what}")


def _check(case, want, msg):
    for padded in (False, True):
        st = _Store(case.nc, max(len(want[0]), 1) + 5)
        st.match(case, padded=padded)
        _same_records(st.read(), want, f"{msg} padded={padded}")


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    case, masks, nt = HAND[name]
    want = R.process(case.dets, case.gts, case.nc, case.thrs)
    assert list(want[2]) == masks and list(want[3]) == nt
    _check(case, want, name)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_shapes_beyond_the_block(name):
    case = SHAPES[name]
    _check(case, R.process(case.dets, case.gts, case.nc, case.thrs), name)


@pytest.mark.parametrize("nc,seed,thrs", [(5, 51, "IOUS1"), (5, 51, "IOUS10"), (5, 51, "IOUS16"), (80, 52, "IOUS10")],
                         ids=["nc5-T1", "nc5-T10", "nc5-T16", "nc80-T10"])
def test_sixteen_image_random_batch(nc, seed, thrs):
    case, want = _batch(nc, seed, thrs)
    assert len(case.dets) == 16 and len(case.thrs) == {"IOUS1": 1, "IOUS10": 10, "IOUS16": 16}[thrs]
    _check(case, want, f"nc {nc} {thrs}")


def test_two_half_batches_equal_the_whole():
    case, want = _batch(5, 51)
    st = _Store(5, len(want[0]) + 5)
    st.match(case, slice(0, 8))
    st.match(case, slice(8, 16), max_det=300)            # another buffer width: the records do not depend on it
    _same_records(st.read(), want)


def test_ten_repeats_are_identical():
    case, want = _batch(80, 52)
    for i in range(10):
        st = _Store(80, len(want[0]) + 5)
        st.match(case)
        _same_records(st.read(), want, f"repeat {i}")


def test_detection_count_beyond_the_buffer_is_clamped():
    """ndet announces all five detections, the buffer holds the first three"""
    case = SHAPES["det5_gt300"]
    want = R.process([case.dets[0][:3]], case.gts, case.nc, case.thrs)
    det, nd, gt, lab, start = R.pack(case)
    st = _Store(case.nc, 8)
    import ctypes as C
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()           # noqa: E731
    d, n_, s_, g, l = dv(det[:, :3]), dv(nd), dv(start), dv(gt), dv(lab)
    assert int(nd[0]) == 5 and len(want[0]) == 3
    offsets = torch.empty(1, dtype=torch.int32, device="cuda")
    thr = np.ascontiguousarray(case.thrs, dtype=np.float64)
    _lib.check(_lib.lib().kodhip_val_match(d.data_ptr(), n_.data_ptr(), g.data_ptr(), l.data_ptr(), s_.data_ptr(),
                                           thr.ctypes.data_as(C.POINTER(C.c_double)), len(thr), st.buf[GUARD:].data_ptr(),
                                           st.count.data_ptr(), st.cap, st.nt.data_ptr(), offsets.data_ptr(), 1, 3, case.nc,
                                           stream()), "val_match")
    torch.cuda.synchronize()
    _same_records(st.read(), want)


# ---- DeviceDetectionMetrics ------------------------------------------------------------------------------------------------

def _targets(gts):
    return tuple(DetectionTarget(torch.from_numpy(np.asarray(g, dtype=np.float64).reshape(-1, 4)), torch.from_numpy(np.asarray(l, np.int64)))
                 for g, l in gts)


def _feed(vm, case, sl=slice(None), batched=False):
    tg = _targets(case.gts[sl])
    if batched:
        tg = BatchedTargets.from_targets(tg, torch.device("cuda"))
    vm.add_batch(tg, [torch.from_numpy(d).cuda() for d in case.dets[sl]])


def _state(vm):
    return (*vm.records(), vm.ground_truths())


def _close(got, want, msg=""):
    np.testing.assert_array_equal(got["n_p"], want["n_p"], err_msg=msg)
    np.testing.assert_array_equal(got["nt"], want["nt"], err_msg=msg)
    for k in ("p", "r", "ap"):
        err = np.abs(got[k] - want[k]).max() if got[k].size else 0.0
        print(f"VALMETRICS {msg} {k}: max |device - reference| = {err:.3e}, bit-equal {np.array_equal(got[k], want[k])}")
        assert got[k].shape == want[k].shape and err <= TOL, (msg, k, err)
    a, b = summarize(got["p"], got["r"], got["ap"], got["nt"]), summarize(want["p"], want["r"], want["ap"], want["nt"])
    assert a["best_index"] == b["best_index"], msg


@pytest.mark.parametrize("batched", [False, True], ids=["DetectionTarget", "BatchedTargets"])
def test_evaluator_accumulates_batches(batched):
    case, want = _batch(5, 51)
    vm = DeviceDetectionMetrics(5)
    for sl in (slice(0, 4), slice(4, 5), slice(5, 16)):
        _feed(vm, case, sl, batched)
    _same_records(_state(vm), want)
    res = vm.compute()
    ref = R.curves_ref(*want, 5, 10)
    _close({**res["curves"], "nt": res["nt"], "n_p": res["n_p"]}, ref, "evaluator nc5")
    tail = summarize(ref["p"], ref["r"], ref["ap"], ref["nt"])
    assert res["best_conf"] == tail["best_conf"] and res["map"] == pytest.approx(tail["map"], abs=TOL)
    assert res["map50"] == pytest.approx(tail["map50"], abs=TOL) and res["map"] > 0
    vm.reset()
    assert len(vm.records()[0]) == 0 and not vm.ground_truths().any() and vm.compute()["map"] == 0.0
    _feed(vm, case, slice(0, 4), batched)
    _same_records(_state(vm), R.process(case.dets[:4], case.gts[:4], 5, case.thrs))


def test_packed_nms_output_is_used_in_place():
    """non_max_suppression hands out views of one [B, 300, 6] buffer with the device-side counts: add_batch passes them on,
    rows beyond each image's count (here: boxes that would count) are never read"""
    from object_detection_cib_amd.core.nms import PackedDetections
    case, want = _batch(5, 51)
    det, nd, *_ = R.pack(case)
    full = np.empty((16, 300, 6), np.float32)
    full[:] = np.array([0, 0, 1000, 1000, 0.99, 0], np.float32)
    for b in range(16):
        full[b, :nd[b]] = det[b, :nd[b]]
    packed = torch.from_numpy(full).cuda()
    views = PackedDetections([packed[b, :int(n)] for b, n in enumerate(nd)], packed, torch.from_numpy(nd).cuda())
    vm = DeviceDetectionMetrics(5)
    vm.add_batch(_targets(case.gts), views)
    _same_records(_state(vm), want)
    vm.reset()
    vm.add_batch(_targets(case.gts), list(views))                  # a plain list of the same tensors: packed by add_batch
    _same_records(_state(vm), want)


@pytest.mark.parametrize("name", sorted(CURVES))
def test_curves_of_injected_records(name):
    case = CURVES[name]
    thrs = {1: R.IOUS1, 10: R.IOUS10, 16: R.IOUS16}[case.T]
    vm = DeviceDetectionMetrics(case.nc, iou_thresholds=thrs, initial_capacity=256)
    for f in case.feeds:
        vm.add_records(*f)
    s, c, m, nt = case.merged()
    _same_records(_state(vm), (s, c, m, nt), name)
    _close(vm.curves(), R.curves_ref(s, c, m, nt, case.nc, case.T), name)


def test_curves_repeat_bit_for_bit():
    case = CURVES["nc80_9000_in_two_feeds"]
    vm = DeviceDetectionMetrics(case.nc)
    for f in case.feeds:
        vm.add_records(*f)
    first = vm.curves()
    for _ in range(3):
        again = vm.curves()
        for k in first:
            np.testing.assert_array_equal(first[k], again[k])


def _identical(a, b):
    _same_records(_state(a), _state(b))
    ca, cb = a.curves(), b.curves()
    for k in ca:
        np.testing.assert_array_equal(ca[k], cb[k], err_msg=k)


def test_merge_of_two_halves_is_the_whole():
    case, want = _batch(5, 51)
    whole, first, second = (DeviceDetectionMetrics(5) for _ in range(3))
    _feed(whole, case)
    _feed(first, case, slice(0, 8))
    _feed(second, case, slice(8, 16))
    kept = _state(second)
    assert first.merge(second) is first
    _same_records(_state(first), want)
    _identical(first, whole)
    _same_records(_state(second), kept)                             # the other evaluator is left as it was
    empty = DeviceDetectionMetrics(5)
    _identical(DeviceDetectionMetrics(5).merge(whole).merge(empty), whole)
    with pytest.raises(ValueError):
        first.merge(DeviceDetectionMetrics(4))


def test_store_growth_changes_nothing():
    """from 64 records the store doubles at least twice while the batches arrive; same records, same curves"""
    case, want = _batch(5, 51)
    small, large = DeviceDetectionMetrics(5, initial_capacity=64), DeviceDetectionMetrics(5, initial_capacity=1 << 16)
    caps = []
    for vm in (small, large):
        for i in range(0, 16, 2):
            _feed(vm, case, slice(i, i + 2))
            if vm is small:
                caps.append(vm.capacity)
    grown = [b for a, b in zip(caps, caps[1:]) if b != a]
    assert caps[0] >= 64 and len(grown) >= 2 and all(b % 64 == 0 and (b // 64) & (b // 64 - 1) == 0 for b in caps), caps
    assert large.capacity == 1 << 16
    _same_records(_state(small), want)
    _identical(small, large)


def _targets_from_detections(exp, batches):
    """A random-init network finds none of the random boxes.  The forward does not depend on the targets, so the ground truths
    are cut from its own detections: rows 0, 3, 10, 40, 41 among those with some area, their height scaled to IoU 1, 0.9, 0.75,
    0.6, 0.52 with the row they came from - true positives at every threshold, at some, and holes where a later row fits better."""
    out = []
    for x, _, extra in batches:
        _, dets = exp.validation_step((x, None, extra))
        tg = []
        for d in dets:
            rows = d.cpu().numpy().astype(np.float64)
            ok = np.flatnonzero((rows[:, 2] - rows[:, 0] > 4) & (rows[:, 3] - rows[:, 1] > 4))
            ok = ok[[i for i in (0, 3, 10, 40, 41) if i < len(ok)]]
            boxes = rows[ok, :4].copy()
            boxes[:, 3] = boxes[:, 1] + (boxes[:, 3] - boxes[:, 1]) * np.array([1.0, 0.9, 0.75, 0.6, 0.52])[:len(ok)]
            tg.append(DetectionTarget(torch.from_numpy(boxes), torch.from_numpy(rows[ok, 5].astype(np.int64))))
        out.append((x, tuple(tg), extra))
    return out


@pytest.mark.parametrize("graphed", [True, False], ids=["graphed", "eager"])
def test_experiment_reports_the_table_next_to_unchanged_keys(graphed):
    from test_hip_confusion import _experiment
    from object_detection_cib_amd.core.nms import PackedDetections
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
    sig = inspect.signature(DefaultYolov5Experiment.__init__).parameters
    assert sig["val_metrics"].default is False and sig["val_metrics"].kind is inspect.Parameter.KEYWORD_ONLY
    exp, batches, nc = _experiment(graphed)
    batches = _targets_from_detections(exp, batches)
    names = ["a", "b", "c", "d"]
    assert exp.val_metrics is False and exp.metrics is None
    exp.val_confusion = False
    plain = exp.validate(batches, nc, names)
    assert exp.metrics is None
    exp.val_metrics = True
    with_vm = exp.validate(batches, nc, names)
    vm = exp.metrics
    assert isinstance(vm, DeviceDetectionMetrics) and np.array_equal(vm.iou_thresholds, R.IOUS10)
    new = {"metrics/precision", "metrics/recall", "metrics/f1", "metrics/best_conf", "metrics/mAP_0.5", "metrics/mAP_0.5:0.95"}
    assert set(with_vm) == set(plain) | new and not set(plain) & new
    for k in plain:
        assert with_vm[k] == plain[k] or (np.isnan(with_vm[k]) and np.isnan(plain[k])), k
    exp.val_confusion = True                                       # all three consumers on the same uploads
    both = exp.validate(batches, nc, names)
    for k in with_vm:
        assert both[k] == with_vm[k] or (np.isnan(both[k]) and np.isnan(with_vm[k])), k
    pairs = [exp.validation_step(b) for b in batches]
    assert all(isinstance(d, PackedDetections) for _, d in pairs)
    parts = [R.process([d.cpu().numpy() for d in dets], [(t.boxes.numpy(), t.labels.numpy()) for t in targets], nc, R.IOUS10)
             for targets, dets in pairs]
    want = tuple(np.concatenate([p[i] for p in parts]) for i in range(3)) + (sum(p[3] for p in parts),)
    print(f"VALMETRICS experiment: {len(want[0])} records, {int((want[2] > 0).sum())} with a true positive, nt {want[3]}")
    assert (want[2] == R.FULL).sum() >= 4 and ((want[2] > 0) & (want[2] < R.FULL)).sum() >= 4 and want[3].sum() >= 16
    assert with_vm["metrics/mAP_0.5"] > with_vm["metrics/mAP_0.5:0.95"] > 0
    _same_records(_state(vm), want)
    ref = R.curves_ref(*want, nc, 10)
    _close(vm.curves(), ref, "experiment")
    tail = summarize(ref["p"], ref["r"], ref["ap"], ref["nt"])
    assert with_vm["metrics/best_conf"] == tail["best_conf"]
    for key, k in (("metrics/precision", "mp"), ("metrics/recall", "mr"), ("metrics/f1", "mf1"), ("metrics/mAP_0.5", "map50"),
                   ("metrics/mAP_0.5:0.95", "map")):
        assert with_vm[key] == pytest.approx(tail[k], abs=TOL), key
