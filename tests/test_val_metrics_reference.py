"""CPU checks of the validation metrics: the closed-form matcher of tests/val_metrics_reference.py (what csrc/val_metrics.hip
implements) equals the per-threshold procedure of YOLOv5's process_batch on random scenes without ties and gives the
hand-worked masks; the curve reference gives hand-worked AP values; the host tail (`summarize`: F1, smoothing, argmax, means)
on synthetic curves; the inputs of the GPU test reach what they were built for; the C entry points' argument checks (no
launch, no GPU)."""
import inspect

import numpy as np
import pytest

import val_metrics_reference as R
from confusion_reference import ConfCase, on_lattice
from object_detection_cib_amd.lightning.callbacks import val_metrics as VM

HAND = R.hand_cases()
SHAPES = R.shape_cases()
CURVES = R.curve_cases()


def test_grids_and_thresholds_are_the_package_s():
    for a, b in ((R.PX, VM.PX), (R.X101, VM.X101), (R.IOUS10, VM.DEFAULT_IOUS)):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    assert R.IOUS10[0] == 0.5 and len(R.IOUS16) == 16 and (np.diff(R.IOUS16) > 0).all()


@pytest.mark.parametrize("seed", [101, 102, 103, 104])
def test_closed_form_equals_the_per_threshold_procedure(seed):
    """750 continuous random images per seed (3 000 in all): IoUs do not tie, so the two forms must agree everywhere"""
    case = R.continuous_batch(5, seed, 750)
    ev = {}
    a = R.process(case.dets, case.gts, case.nc, case.thrs, R.match_closed, ev)
    b = R.process(case.dets, case.gts, case.nc, case.thrs, R.match_literal)
    print(f"VALMETRICS closed vs literal seed {seed}: records {len(a[0])} events {ev}")
    assert ev.get("tie_det", 0) == 0
    assert ev["holes"] >= 20 and ev["lost"] >= 200 and len(a[0]) > 20000
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", sorted(HAND))
@pytest.mark.parametrize("matcher", [R.match_closed, R.match_literal], ids=["closed", "literal"])
def test_matchers_give_the_hand_masks(name, matcher):
    case, masks, nt = HAND[name]
    s, c, m, n = R.process(case.dets, case.gts, case.nc, case.thrs, matcher)
    assert list(m) == masks
    assert list(n) == nt


def test_hand_cases_reach_their_events():
    ev = {n: {} for n in HAND}
    for n, (case, _, _) in HAND.items():
        R.process(case.dets, case.gts, case.nc, case.thrs, events=ev[n])
    assert ev["B_hole_at_the_bottom"]["holes"] == 1 and ev["B_hole_at_the_bottom"]["lost"] == 0
    assert ev["C_exactly_on_a_threshold"]["exact_thr"] == 1
    assert ev["D_duplicates"]["tie_gt"] == 2 and ev["D_duplicates"]["tie_det"] == 1
    assert ev["F_loser_not_rematched"]["lost"] == 1


def test_gpu_shapes_are_what_the_kernel_test_needs():
    assert len(SHAPES["det300_gt3"].dets[0]) == 300 and len(SHAPES["det300_gt3"].gts[0][1]) == 3
    assert len(SHAPES["det5_gt300"].dets[0]) == 5 and len(SHAPES["det5_gt300"].gts[0][1]) == 300
    ev = {}
    s, c, m, nt = R.process(*SHAPES["det300_gt3"][2:], 2, R.IOUS10, events=ev)
    assert ev["holes"] >= 10 and ev["lost"] >= 100 and len(set(m.tolist())) >= 8
    s, c, m, nt = R.process(*SHAPES["det5_gt300"][2:], 3, R.IOUS10)
    assert list(m) == [R.FULL] * 4 + [0] and list(nt) == [100, 100, 100]
    for nc, seed in ((5, 51), (80, 52)):
        case, ev = R.random_batch(nc, seed), {}
        s, c, m, nt = R.process(case.dets, case.gts, nc, case.thrs, events=ev)
        print(f"VALMETRICS random batch nc {nc}: records {len(s)} events {ev}")
        assert len(case.dets) == 16 and ev["holes"] >= 1 and ev["lost"] >= 5 and (m > 0).sum() >= 20
        assert on_lattice(ConfCase(nc, 0, 0, case.dets, case.gts, None))
    for name, case in SHAPES.items():
        assert on_lattice(ConfCase(case.nc, 0, 0, case.dets, case.gts, None)), name


def test_curves_of_the_tp_fp_tp_hand_case():
    """Hand case A: records (0.9, TP), (0.8, FP), (0.7, TP at bits 0 - 5), two ground truths.
    Threshold 0: recall 1/2, 1/2, 1 and precision 1, 1/2, 2/3; mrec = 0, .5, .5, 1, 1, envelope = 1, 1, 2/3, 2/3, 0.  interp gives
    1 below recall 0.5, 2/3 from 0.5 (the LAST of the duplicate 0.5s) up to but not including 1, and 0 at 1:
    AP = 0.49 + 0.01 (1 + 2/3) / 2 + 0.49 * 2/3 + 0.01 (2/3) / 2.
    Threshold 6 (0.8): the third record is a false positive: recall 1/2 throughout, precision 1, 1/2, 1/3; mrec = 0, .5, .5, .5, 1,
    envelope = 1, 1, 1/2, 1/3, 0: 1 below 0.5, then the line from (0.5, 1/3) to (1, 0):
    AP = 0.49 + 0.01 (1 + 1/3) / 2 + (1/3) / 4."""
    case, _, _ = HAND["A_tp_fp_tp"]
    s, c, m, nt = R.process(case.dets, case.gts, 1, case.thrs)
    cur = R.curves_ref(s, c, m, nt, 1, 10)
    assert cur["ap"][0, 0] == pytest.approx(0.49 + 0.01 * (1 + 2 / 3) / 2 + 0.49 * 2 / 3 + 0.01 / 3, abs=1e-12)
    assert cur["ap"][0, 6] == pytest.approx(0.49 + 0.01 * (1 + 1 / 3) / 2 + 1 / 12, abs=1e-12)
    # confidence curves: above 0.9 nothing is kept (recall 0, precision 1 = `left`); at or below 0.7 everything is
    hi, lo = R.PX > np.float64(np.float32(0.9)), R.PX <= np.float64(np.float32(0.7))
    assert (cur["r"][0, hi] == 0).all() and (cur["p"][0, hi] == 1).all()
    assert (cur["r"][0, lo] == 1).all() and (cur["p"][0, lo] == 2 / 3).all()
    assert list(cur["n_p"]) == [3]


def test_curve_cases_cover_what_they_claim():
    s, c, m, nt = CURVES["one_class_5000"].merged()
    assert len(s) == 5000 and len(np.unique(s)) < 600 and set(c) == {1}                # ties, more than one 4096-key chunk
    s, c, m, nt = CURVES["nc80_9000_in_two_feeds"].merged()
    assert len(s) == 9000 and len(set(c)) == 7 and len(nt) == 80
    s, c, m, nt = CURVES["grid_ends"].merged()
    assert s.max() == 1.0 and s.min() == np.float32(0.001)
    for name, case in CURVES.items():
        s, c, m, nt = case.merged()
        for j in range(case.T):
            for k in range(case.nc):
                assert ((m[c == k] >> j) & 1).sum() <= max(nt[k], 0) or nt[k] == 0, (name, j, k)
        cur = R.curves_ref(s, c, m, nt, case.nc, case.T)
        assert np.isfinite(cur["p"]).all() and np.isfinite(cur["r"]).all() and np.isfinite(cur["ap"]).all()
        assert cur["ap"].min() >= 0 and cur["ap"].max() <= 1 + 1e-12
    # arrival order decides inside a tie: swapping the two feeds changes the curves
    case = CURVES["ties_across_two_feeds"]
    a = R.curves_ref(*case.merged(), 1, 10)
    b = R.curves_ref(*R.CurveCase(1, 10, case.feeds[::-1]).merged(), 1, 10)
    assert not np.array_equal(a["ap"], b["ap"])
    cur = R.curves_ref(*CURVES["gt_only_and_records_only"].merged(), 3, 10)
    assert not cur["p"][:2].any() and not cur["ap"][:2].any() and cur["ap"][2].any() and list(cur["n_p"]) == [0, 2, 2]


def test_smooth_is_a_101_tap_box_filter_with_padded_ends():
    y = np.zeros(1000)
    y[500] = 101.0
    z = VM.smooth(y, 0.1)
    assert z.shape == (1000,)
    np.testing.assert_allclose(z[450:551], 1.0, rtol=0, atol=1e-12)
    assert not z[:450].any() and not z[551:].any()
    ramp = np.arange(1000, dtype=np.float64)
    z = VM.smooth(ramp, 0.1)
    np.testing.assert_allclose(z[50:950], ramp[50:950], atol=1e-9)              # a box filter keeps a line, away from the ends
    assert z[0] == pytest.approx(sum(range(51)) / 101, abs=1e-9)               # 50 padded zeros + 0 .. 50


def test_summarize_on_a_synthetic_curve():
    """Three classes; class 1 has no ground truth and must not count.  Classes 0 and 2 have p = r = 1 on px[300:700], 0
    elsewhere, so f1 is that plateau; its 101-tap mean is 1 exactly where the window lies inside it: indices 350 .. 649, every
    such window summing the same 101 terms, and smaller elsewhere.  The FIRST maximum is 350."""
    p = np.zeros((3, 1000)); r = np.zeros((3, 1000))
    p[[0, 2], 300:700] = 1.0; r[[0, 2], 300:700] = 1.0
    p[1] = 0.9; r[1] = 0.9                                  # would move nothing even if it were counted; it is not
    ap = np.array([[0.8, 0.4], [0.99, 0.99], [0.6, 0.2]])
    res = VM.summarize(p, r, ap, np.array([4, 0, 1]), np.array([5, 5, 5]))
    assert res["best_index"] == 350 and res["best_conf"] == R.PX[350]
    assert list(res["classes"]) == [0, 2]
    assert res["mp"] == 1.0 and res["mr"] == 1.0 and res["mf1"] == 1.0
    assert res["map50"] == pytest.approx(0.7) and res["map"] == pytest.approx((0.6 + 0.4) / 2)
    assert list(res["per_class"]["ap50"]) == [0.8, 0.0, 0.6] and res["per_class"]["precision"][1] == 0.0
    # a class whose F1 peaks elsewhere pulls the mean: class 2's plateau at [100:200) only
    p[2] = 0; r[2] = 0; p[2, 100:200] = 1.0; r[2, 100:200] = 1.0
    res = VM.summarize(p, r, ap, np.array([4, 0, 1]))
    assert res["best_index"] == 350 and res["per_class"]["f1"][2] == 0.0 and res["mf1"] == 0.5
    none = VM.summarize(p, r, ap, np.zeros(3, np.int64))
    assert (none["mp"], none["mr"], none["mf1"], none["map50"], none["map"], none["best_conf"]) == (0.0,) * 6
    assert not any(v.any() for v in none["per_class"].values())


def test_evaluator_without_a_batch_reports_zeros():
    vm = VM.DeviceDetectionMetrics(4, list("abcd"))
    res = vm.compute()
    assert (res["mp"], res["mr"], res["mf1"], res["map50"], res["map"], res["best_conf"]) == (0.0,) * 6
    assert res["curves"]["p"].shape == (4, 1000) and res["curves"]["ap"].shape == (4, 10)
    assert len(vm.records()[0]) == 0 and not vm.ground_truths().any()
    with pytest.raises(ValueError):
        VM.DeviceDetectionMetrics(4, iou_thresholds=np.linspace(0.1, 0.9, 17))
    sig = inspect.signature(VM.DeviceDetectionMetrics.__init__).parameters
    assert list(sig)[1:4] == ["num_classes", "class_names", "iou_thresholds"]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes as C
    from object_detection_cib_amd import _lib
    h = _lib.lib()
    assert h.kodhip_version() >= 108 and h.kodhip_val_record_bytes() == 8
    assert h.kodhip_val_max_det() >= 300 and h.kodhip_val_max_thresholds() == 16
    thr = (C.c_double * 17)(*np.linspace(0.1, 0.9, 17))
    one = C.c_void_p(64)                                    # never dereferenced: every call below is refused first
    big = h.kodhip_val_max_det() + 1
    assert h.kodhip_val_match(one, one, one, one, one, thr, 10, one, one, 100, one, one, 1, big, 3, None) < 0
    assert b"max_det" in h.kodhip_last_error()
    assert h.kodhip_val_match(one, one, one, one, one, thr, 17, one, one, 100, one, one, 1, 300, 3, None) < 0
    assert b"thresholds" in h.kodhip_last_error()
    assert h.kodhip_val_match(one, one, one, one, one, thr, 10, one, one, 0, one, one, 1, 300, 3, None) < 0
    assert h.kodhip_val_match(one, one, one, one, one, thr, 10, None, one, 100, one, one, 1, 300, 3, None) < 0
    assert h.kodhip_val_match(one, one, one, one, one, thr, 10, one, one, 100, one, one, 1, 300, 65537, None) < 0
    assert h.kodhip_val_append(one, one, 100, one, one, 10, None) < 0                   # dst == src
    assert h.kodhip_val_append(one, one, 0, C.c_void_p(128), one, 10, None) < 0
    assert h.kodhip_val_curves_workspace_bytes(0, 3, 10) == -1 and h.kodhip_val_curves_workspace_bytes(100, 3, 17) == -1
    small, large = h.kodhip_val_curves_workspace_bytes(100, 3, 10), h.kodhip_val_curves_workspace_bytes(10000, 80, 10)
    assert 0 < small < large and small % 16 == 0
    assert h.kodhip_val_curves(one, one, 100, one, one, 1000, one, 101, 3, 10, C.c_void_p(72), one, one, one, one, None) < 0
    assert b"aligned" in h.kodhip_last_error()
    assert h.kodhip_val_curves(one, one, 100, one, one, 1000, one, 2000, 3, 10, one, one, one, one, one, None) < 0
    assert h.kodhip_val_curves(one, one, 100, one, one, 1000, one, 101, 3, 10, None, one, one, one, one, None) < 0
