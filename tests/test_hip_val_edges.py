"""The validation path's device stages - kodhip_decode, kodhip_nms, kodhip_map_match (csrc/postproc.hip, csrc/map_match.hip)
and DeviceMAPEvaluator's host accumulation - against the plain references of tests/val_reference.py at the places where the
kernels decide something and random scenes do not go: rectangular grids and saturated logits in the decode; candidate
counts around the sort's padding / chunk / global-pass edges, mixed in one batch; score ties; IoU exactly at the threshold;
suppression inside a 64-lane batch and across batches; the max_det / max_nms / key_cap cuts; matching at exact thresholds,
equal IoUs, taken ground truths, the per-class budget, the 256-bit `used` map; score ties across images in the accumulation.

Every stage is called through the C ABI with the test's own buffers and through the public wrapper (get_detections,
non_max_suppression, DeviceMAPEvaluator).  NMS rows, sort keys, candidate counts, `tp` and `counted` are compared exactly;
the evaluator's report within 1e-12; the decode within V.DECODE_BOX_ULP / V.DECODE_SCORE_REL (twice the fp32 CPU oracle's own
error on the same inputs, tests/val_reference.py), with exact 0 / 1 where fp64 rounds to it.  That every input reaches what
it was built for is asserted on the CPU (tests/test_val_reference.py).  Figures are printed before they are asserted
(`pytest -s`).

Measured on an MI355X with the tolerances chosen beforehand, max over the 18 decode cases: box error 2.83 ulp32 (tolerance
6; the fp32 CPU oracle has 2.83 on the same case), score error 1.28e-7 relative (tolerance 2.38e-7; oracle 1.18e-7), no
exact 0 / 1 missed, no NaN.  Everything else is exact; the evaluator's reports differed from the oracle's by 0.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import val_reference as V  # noqa: E402
from hip_helpers import stream  # noqa: E402
from oracle import map_eval as M  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402
from object_detection_cib_amd.core.nms import non_max_suppression  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.data.detection import DetectionTarget  # noqa: E402
from object_detection_cib_amd.lightning.callbacks.map_eval import DeviceMAPEvaluator  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.layers import get_detections  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo  # noqa: E402

ANCH = LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
GUARD = 1024
POISON_KEY = 0x5A5A5A5A5A5A5A5A


# ------------------------------------------------------------------------------------------------------------ decode
def _decode_direct(raws):
    """kodhip_decode on the three [B, A, h, w, P] tensors; the output sits inside a poisoned buffer -> (det, intact)"""
    dev = [r.cuda().contiguous() for r in raws]
    B, A, _, _, P = dev[0].shape
    levels = (_lib.KodDecodeLevel * 3)()
    rows = 0
    for lv, t, s, anc in zip(levels, dev, V.STRIDES, V.ANCHORS):
        lv.raw, lv.h, lv.w, lv.stride = t.data_ptr(), t.shape[2], t.shape[3], s
        for k, (aw, ah) in enumerate(anc):
            lv.anchor_w[k], lv.anchor_h[k] = float(aw), float(ah)
        rows += A * t.shape[2] * t.shape[3]
    n = B * rows * P
    buf = torch.full((n + 2 * GUARD,), -7.0, device="cuda")
    out = buf[GUARD:GUARD + n].view(B, rows, P)
    _lib.check(_lib.lib().kodhip_decode(levels, out.data_ptr(), B, A, P - 5, stream()), "decode")
    torch.cuda.synchronize()
    intact = bool((buf[:GUARD] == -7.0).all()) and bool((buf[-GUARD:] == -7.0).all())
    return out.cpu(), intact


@pytest.mark.parametrize("name", list(V.decode_cases()))
def test_decode_rectangular_saturated_vs_fp64(name):
    w, h, nc, B, seed = V.decode_cases()[name]
    case = V.decode_case(w, h, nc, B, seed)
    ref = V.decode_ref(case.raws, V.STRIDES, V.ANCHORS, w, h)
    got, intact = _decode_direct(case.raws)
    assert intact, "decode wrote outside its output"
    assert got.shape == ref.shape
    box, rel, missed = V.decode_errors(got, ref)
    print(f"VALEDGE decode {name} box {box:.3f} ulp32 (tol {V.DECODE_BOX_ULP}), score {rel:.4e} rel (tol {V.DECODE_SCORE_REL:.4e}), "
          f"exact 0/1 missed {missed} of {case.facts['exact_zero'] + case.facts['exact_one']}")
    assert not bool(torch.isnan(got).any()) and bool(torch.isfinite(got).all())
    assert missed == 0
    assert box <= V.DECODE_BOX_ULP and rel <= V.DECODE_SCORE_REL
    # the public wrapper runs the same launch: bit for bit
    net = tuple((r[..., :4].cuda(), r[..., 4:5].cuda(), r[..., 5:].cuda()) for r in case.raws)
    pub = get_detections(FeatureShape(width=w, height=h), net, ANCH)
    assert torch.equal(pub.cpu().view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("w,h", V.DECODE_SHAPES)
def test_per_level_prediction_classes_equal_get_detections_rectangular(w, h):
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.layers import (
        Yolov5BoxPrediction, Yolov5ClassPrediction, Yolov5ObjectnessPrediction, Yolov5Prediction, Yolov5PredictionAssembler)
    nc, B = 2, 3
    case = V.decode_case(w, h, nc, B, seed=41)
    shape = FeatureShape(width=w, height=h)
    net = tuple((r[..., :4].cuda(), r[..., 4:5].cuda(), r[..., 5:].cuda()) for r in case.raws)
    want = get_detections(shape, net, ANCH)
    preds = []
    for (box, obj, cls), info in zip(net, ANCH):
        p = Yolov5Prediction(info.stride, shape, info.boxes_wh)(box, obj, cls)
        assert p.box.shape == (B, 3 * (h // info.stride) * (w // info.stride), 4)
        assert torch.equal(Yolov5BoxPrediction(info.stride, shape, info.boxes_wh)(box).view(torch.int32), p.box.contiguous().view(torch.int32))
        assert torch.equal(Yolov5ObjectnessPrediction()(obj).view(torch.int32), p.obj.contiguous().view(torch.int32))
        assert torch.equal(Yolov5ClassPrediction()(cls).view(torch.int32), p.cls.contiguous().view(torch.int32))
        preds.append(p)
    det = Yolov5PredictionAssembler()([p.box for p in preds], [p.obj for p in preds], [p.cls for p in preds])
    assert torch.equal(det.view(torch.int32), want.view(torch.int32))


# --------------------------------------------------------------------------------------------------------------- NMS
def _nms_direct(det, conf, thr, key_cap, max_det=300, max_nms=30000, max_wh=4096.0):
    """kodhip_nms with the test's own buffers.  The key workspace is followed by GUARD poisoned words, the output rows
    and counts are poisoned.  -> dict(ncand, keys [B, key_cap] uint64, rows (list of [n, 6]), nout, guard_intact)"""
    d = torch.from_numpy(np.ascontiguousarray(det, dtype=np.float32)).cuda()
    B, rows, P = d.shape
    keys = torch.full((B * key_cap + GUARD,), POISON_KEY, dtype=torch.int64, device="cuda")
    ncand = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    nout = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    out = torch.full((B, max_det, 6), -7.0, device="cuda")
    _lib.check(_lib.lib().kodhip_nms(d.data_ptr(), keys.data_ptr(), key_cap, ncand.data_ptr(), out.data_ptr(), nout.data_ptr(),
                                     B, rows, P - 5, float(conf), float(thr), max_det, max_nms, float(max_wh), stream()), "nms")
    torch.cuda.synchronize()
    k = keys.cpu().numpy().view(np.uint64)
    n = nout.cpu().numpy()
    o = out.cpu().numpy()
    assert ((0 <= n) & (n <= max_det)).all(), n
    for b in range(B):                                       # nothing written behind the survivors
        assert (o[b, n[b]:] == -7.0).all()
    return dict(ncand=ncand.cpu().numpy(), keys=k[:B * key_cap].reshape(B, key_cap), rows=[o[b, :n[b]] for b in range(B)],
                nout=n, guard_intact=bool((k[B * key_cap:] == np.uint64(POISON_KEY)).all()))


def _cap_for(det):
    need, cap = det.shape[1] * (det.shape[2] - 5), 64
    while cap < need:
        cap <<= 1
    return cap


def _same_rows(got, want, tag):
    assert [len(g) for g in got] == [len(w) for w in want], (tag, [len(g) for g in got], [len(w) for w in want])
    for b, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(np.asarray(g).view(np.uint32), w.view(np.uint32), err_msg=f"{tag} image {b}")


def _wrapper(det, conf, thr, **kw):
    return [r.cpu().numpy() for r in non_max_suppression(torch.from_numpy(det).cuda(), conf, thr, **kw)]


def test_nms_sort_reach_counts_keys_and_rows():
    """ten images with 0 .. 9600 candidates in ONE batch, key_cap 16384: padding to 64 and to the next power of two, the
    4096-key chunk edge, the first global pass at 8193, and every early exit of the small images beside the large ones"""
    det, conf, thr, facts = V.sort_reach_case()
    assert tuple(facts["counts"]) == V.SORT_COUNTS
    ref_keys = V.nms_keys_ref(det, conf)
    want = V.nms_ref(det, conf, thr)
    r = _nms_direct(det, conf, thr, key_cap=16384)
    assert r["guard_intact"]
    np.testing.assert_array_equal(r["ncand"], np.asarray(V.SORT_COUNTS, dtype=np.int32))
    for b, (_, order) in enumerate(ref_keys):
        np.testing.assert_array_equal(r["keys"][b, :len(order)], order, err_msg=f"sorted keys of image {b}")
    _same_rows(r["rows"], want, "sort reach direct")
    _same_rows(_wrapper(det, conf, thr), want, "sort reach wrapper")


def test_nms_clustered_deep_walks():
    """boxes clustered around 40 centres per class: the greedy walk goes past ranks 4096 and 8192 before the 300th
    survivor, ends short of 300 on one image and stops at exactly 300 on others"""
    det, conf, thr, facts = V.cluster_case()
    print("VALEDGE cluster", facts)
    assert max(facts["last_rank"]) > 8192 and min(facts["survivors"]) < 300
    want = V.nms_ref(det, conf, thr)
    ref_keys = V.nms_keys_ref(det, conf)
    r = _nms_direct(det, conf, thr, key_cap=_cap_for(det))
    assert r["guard_intact"]
    np.testing.assert_array_equal(r["ncand"], [len(k) for k, _ in ref_keys])
    for b, (_, order) in enumerate(ref_keys):
        np.testing.assert_array_equal(r["keys"][b, :len(order)], order, err_msg=f"sorted keys of image {b}")
    _same_rows(r["rows"], want, "cluster direct")
    _same_rows(_wrapper(det, conf, thr), want, "cluster wrapper")


def test_nms_ties_follow_score_desc_index_asc():
    det, conf, thr, facts = V.ties_case()
    print("VALEDGE ties", facts)
    assert facts["tied_share"] >= 0.25 and any(facts["rule_changes_survivors"])
    want = V.nms_ref(det, conf, thr)
    ref_keys = V.nms_keys_ref(det, conf)
    r = _nms_direct(det, conf, thr, key_cap=_cap_for(det))
    np.testing.assert_array_equal(r["ncand"], [len(k) for k, _ in ref_keys])
    for b, (_, order) in enumerate(ref_keys):
        np.testing.assert_array_equal(r["keys"][b, :len(order)], order, err_msg=f"sorted keys of image {b}")
    _same_rows(r["rows"], want, "ties direct")
    _same_rows(_wrapper(det, conf, thr), want, "ties wrapper")


@pytest.mark.parametrize("name", list(V.hand_cases()) + list(V.cap_cases()))
def test_nms_hand_built_decisions_and_caps(name):
    c = {**V.hand_cases(), **V.cap_cases()}[name]
    want = V.nms_ref(c.det, c.conf, c.thr, **c.kwargs)
    kept = c.det[0, c.kept_rows]                              # the issue's table, independent of nms_ref
    r = _nms_direct(c.det, c.conf, c.thr, key_cap=_cap_for(c.det), **c.kwargs)
    assert r["guard_intact"]
    print(f"VALEDGE hand {name} nout {r['nout'].tolist()} expected {len(c.kept_rows)}")
    assert r["nout"].tolist() == [len(c.kept_rows)]
    np.testing.assert_array_equal(r["rows"][0][:, :4], kept[:, :4])
    _same_rows(r["rows"], want, name + " direct")
    if not c.kwargs:
        _same_rows(_wrapper(c.det, c.conf, c.thr), want, name + " wrapper")


def test_nms_key_cap_below_the_candidate_count():
    """key_cap 256 against ~1170 candidates per image: the first 256 candidates in (row, class) order take part (the ABI
    comment), ncand says 256, and nothing is written behind the B * key_cap keys"""
    det, conf, thr, facts = V.key_cap_case()
    assert min(facts["candidates"]) > 256 and all(facts["cap_changes_result"])
    want = V.nms_ref(det, conf, thr, key_cap=256)
    r = _nms_direct(det, conf, thr, key_cap=256)
    assert r["guard_intact"], "keys were written behind B * key_cap"
    assert r["ncand"].tolist() == [256, 256]
    for b, (keys, _) in enumerate(V.nms_keys_ref(det, conf)):
        np.testing.assert_array_equal(r["keys"][b], np.sort(keys[:256]), err_msg=f"image {b}")
    _same_rows(r["rows"], want, "key_cap 256")


def test_nms_wrapper_class_filter_and_strided_input():
    det, conf, thr = V.wrapper_case()
    _same_rows(_wrapper(det, conf, thr, classes=[1, 4]), V.nms_ref(det, conf, thr, classes=[1, 4]), "classes=[1, 4]")
    _same_rows(_wrapper(det, conf, thr, classes=(5,)), V.nms_ref(det, conf, thr, classes=[5]), "classes=(5,)")
    want = V.nms_ref(det, conf, thr)
    wide = torch.full((det.shape[0], det.shape[1], det.shape[2] + 3), float("nan"))
    wide[..., :det.shape[2]] = torch.from_numpy(det)
    view = wide.cuda()[..., :det.shape[2]]                        # row stride 14, not 11
    assert not view.is_contiguous()
    _same_rows([r.cpu().numpy() for r in non_max_suppression(view, conf, thr)], want, "strided rows")
    tr = torch.from_numpy(det).cuda().permute(1, 0, 2).contiguous().permute(1, 0, 2)      # image stride < row stride
    assert not tr.is_contiguous()
    _same_rows([r.cpu().numpy() for r in non_max_suppression(tr, conf, thr)], want, "transposed batch")


def test_nms_argument_checks_return_an_error_code():
    """out-of-range arguments end in the ABI's own checks: a status, and no launch (the poisoned outputs stay)"""
    det = V.hand_cases()["iou_equals_thr"].det
    for kw, msg in ((dict(key_cap=100), "power of two"), (dict(key_cap=32), "power of two"), (dict(key_cap=64, max_det=301), "max_det")):
        d = torch.from_numpy(det).cuda()
        keys = torch.full((256,), 3, dtype=torch.int64, device="cuda")
        nc_, no_ = torch.full((1,), -1, dtype=torch.int32, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda")
        out = torch.full((1, 301, 6), -7.0, device="cuda")
        rc = _lib.lib().kodhip_nms(d.data_ptr(), keys.data_ptr(), kw["key_cap"], nc_.data_ptr(), out.data_ptr(), no_.data_ptr(),
                                   1, det.shape[1], det.shape[2] - 5, 0.25, 0.45, kw.get("max_det", 300), 30000, 4096.0, stream())
        torch.cuda.synchronize()
        assert rc != 0 and msg in _lib.lib().kodhip_last_error().decode()
        assert int(nc_) == -1 and int(no_) == -1 and bool((out == -7.0).all()) and bool((keys == 3).all())


# ---------------------------------------------------------------------------------------------------------- matching
def _match_direct(det, nd, gt, lab, start, nc, thrs, max_per_class=100):
    """kodhip_map_match with the test's own buffers, outputs poisoned with 7 -> (tp, counted) uint8 arrays"""
    B, max_det, _ = det.shape
    T = len(thrs)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()           # noqa: E731
    d, n_, s_ = dv(det), dv(nd), dv(start)
    g, l = (dv(gt), dv(lab)) if len(lab) else (None, None)
    tp = torch.full((B, max_det, T), 7, dtype=torch.uint8, device="cuda")
    counted = torch.full((B, max_det), 7, dtype=torch.uint8, device="cuda")
    thr = (C.c_double * T)(*thrs)
    _lib.check(_lib.lib().kodhip_map_match(d.data_ptr(), n_.data_ptr(), g.data_ptr() if g is not None else None,
                                           l.data_ptr() if l is not None else None, s_.data_ptr(), tp.data_ptr(),
                                           counted.data_ptr(), B, max_det, nc, thr, T, max_per_class, stream()), "map_match")
    torch.cuda.synchronize()
    return tp.cpu().numpy(), counted.cpu().numpy()


def _check_match(tag, det, nd, gt, lab, start, nc, thrs):
    want_tp, want_c = V.match_ref(det, nd, gt, lab, start, nc, thrs, 100)
    tp, counted = _match_direct(det, nd, gt, lab, start, nc, thrs)
    for b in range(det.shape[0]):
        n = min(int(nd[b]), det.shape[1])
        np.testing.assert_array_equal(tp[b, :n], want_tp[b, :n], err_msg=f"{tag} tp of image {b}")
        np.testing.assert_array_equal(counted[b, :n], want_c[b, :n], err_msg=f"{tag} counted of image {b}")
        assert (tp[b, n:] == 7).all() and (counted[b, n:] == 7).all(), f"{tag}: image {b} written behind its detections"
    return want_tp, want_c


@pytest.mark.parametrize("nc", [2, 80])
@pytest.mark.parametrize("thrs", [V.THRS4, V.THRS8], ids=["T4", "T8"])
def test_matching_hand_built_batch(nc, thrs):
    case = V.match_case(nc, thrs)
    f = case.facts
    assert f["exact_thr"] >= len(thrs) and f["equal_iou"] and f["stolen"] and f["over_budget"] == 30
    assert set(V.BITMAP_INDICES) <= f["matched_index"]
    det, nd, gt, lab, start = V._pack(case.dets, case.gts)
    want_tp, want_c = _check_match(f"nc {nc} T {len(thrs)}", det, nd, gt, lab, start, nc, thrs)
    print(f"VALEDGE match nc {nc} T {len(thrs)} tp {int(want_tp.sum())} counted {int(want_c.sum())}")
    # ndet beyond max_det: the buffer holds 60 rows per image, image 2 announces all 170
    det2, nd2, *_ = V._pack(case.dets, case.gts, max_det=60)
    assert int(nd2[2]) == 170 > det2.shape[1]
    _check_match(f"nc {nc} T {len(thrs)} max_det 60", det2, nd2, gt, lab, start, nc, thrs)
    # a batch without any ground truth (null ground-truth pointers), and single images (each is then the last)
    empty = [(np.zeros((0, 4)), np.zeros(0, np.int64))] * len(case.dets)
    _check_match("no ground truth", *V._pack(case.dets, empty), nc, thrs)
    for b in (4, 5):
        _check_match(f"image {b} alone", *V._pack(case.dets[b:b + 1], case.gts[b:b + 1]), nc, thrs)


def _targets(gts):
    return tuple(DetectionTarget(torch.from_numpy(np.asarray(g, dtype=np.float64).reshape(-1, 4)), torch.from_numpy(l)) for g, l in gts)


def _report_equal(got, want, tol=1e-12):
    assert set(got) == set(want)
    worst = 0.0
    for k in want:
        if np.isnan(want[k]):
            assert np.isnan(got[k]), k
        else:
            worst = max(worst, abs(got[k] - want[k]))
    print(f"VALEDGE report max |diff| {worst:.3e}")
    assert worst <= tol


@pytest.mark.parametrize("nc", [2, 80])
def test_evaluator_on_the_hand_built_batch(nc):
    case = V.match_case(nc, V.THRS4)
    ev = DeviceMAPEvaluator(nc)
    ev.add_batch(_targets(case.gts), [torch.from_numpy(d).cuda() for d in case.dets])
    det, nd, gt, lab, start = V._pack(case.dets, case.gts)
    tp, counted = V.match_ref(det, nd, gt, lab, start, nc, V.THRS4, 100)
    want = M.report(M.accumulate(V.per_image_records(det, nd, tp, counted, lab, start, nc), nc))
    _report_equal(ev.get_report(), want)


def test_evaluator_refuses_257_ground_truths():
    g = V._grid_boxes(257).astype(np.float64)
    det = [torch.from_numpy(V._f32([[0, 0, 10, 10, 0.9, 0]])).cuda()]
    ev = DeviceMAPEvaluator(2)
    with pytest.raises(ValueError, match="257"):
        ev.add_batch(_targets([(g, np.zeros(257, np.int64))]), det)
    ev.add_batch(_targets([(g[:256], np.zeros(256, np.int64))]), det)          # 256 is accepted
    assert ev.get_report()["map50_0"] > 0


def test_evaluator_score_ties_across_images_and_one_sided_classes():
    batches, per_image, facts = V.evaluator_batches()
    print("VALEDGE evaluator", facts)
    assert facts["order_matters"] and facts["dets_without_gt"] and facts["gt_without_dets"]
    nc = 5
    ev = DeviceMAPEvaluator(nc)
    for dets, gts in batches:
        ev.add_batch(_targets(gts), [torch.from_numpy(d).cuda() for d in dets])
    want = M.report(M.accumulate(per_image, nc))
    got = ev.get_report()
    assert np.isnan(got["map50_3"]) and got["map50_4"] == 0.0
    _report_equal(got, want)
