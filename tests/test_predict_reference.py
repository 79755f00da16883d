"""The inference references (tests/predict_reference.py) on their own: with the options off they are the validation
reference, the best-class form equals a direct torch restatement of YOLOv5's non_max_suppression (multi_label=False) on
tie-free inputs, and every constructed case reaches what it was built for.  Also the host side of the new interface that
needs no GPU: the ABI's argument checks and the Detector's letterbox table.  Runs anywhere (no GPU)."""
import inspect

import numpy as np
import pytest
import torch

from oracle import detection as D
import predict_reference as R
import val_reference as V


def _rows_equal(got, want):
    assert [len(g) for g in got] == [len(w) for w in want]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(np.asarray(g, np.float32).view(np.uint32), np.asarray(w, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------- options off = nms_ref
@pytest.mark.parametrize("name", list(V.hand_cases()) + list(V.cap_cases()))
def test_options_off_equals_nms_ref_on_hand_cases(name):
    c = {**V.hand_cases(), **V.cap_cases()}[name]
    _rows_equal(R.nms_ex_ref(c.det, c.conf, c.thr, **c.kwargs), V.nms_ref(c.det, c.conf, c.thr, **c.kwargs))


@pytest.mark.parametrize("case", [V.ties_case, V.cluster_case], ids=["ties", "cluster"])
def test_options_off_equals_nms_ref_on_tie_and_cluster_cases(case):
    det, conf, thr, _ = case()
    _rows_equal(R.nms_ex_ref(det, conf, thr), V.nms_ref(det, conf, thr))
    ident = R.nms_ex_ref(det, conf, thr, letterbox=R.identity_letterbox(len(det)))
    _rows_equal(ident, V.nms_ref(det, conf, thr))                 # boxes inside [0, extent]: the identity changes no bit


# ------------------------------------------------------------------------------- best class = YOLOv5 multi_label=False
def _yolov5_best_class(det, conf_thres, iou_thres, classes=None, agnostic=False, max_det=300, max_wh=4096.0, max_nms=30000):
    """general.py non_max_suppression with multi_label=False, in torch fp32 (greedy NMS: oracle.detection.greedy_nms)"""
    out = []
    for x in torch.from_numpy(det):
        x = x[x[:, 4] > conf_thres].clone()
        x[:, 5:] *= x[:, 4:5]
        conf, j = x[:, 5:].max(1, keepdim=True)
        x = torch.cat((x[:, :4], conf, j.float()), 1)[conf.view(-1) > conf_thres]
        if classes is not None:
            x = x[(x[:, 5:6] == torch.tensor(classes, dtype=torch.float32)).any(1)]
        x = x[x[:, 4].argsort(descending=True, stable=True)[:max_nms]]
        c = x[:, 5:6] * (0.0 if agnostic else max_wh)
        i = D.greedy_nms(x[:, :4] + c, x[:, 4], iou_thres)[:max_det]
        out.append(x[i].numpy().reshape(-1, 6))
    return out


@pytest.mark.parametrize("nc", [1, 2, 80])
@pytest.mark.parametrize("kw", [{}, dict(agnostic=True), dict(max_det=5), dict(classes=[0, 1])], ids=["plain", "agnostic", "max_det5", "classes"])
def test_best_class_equals_yolov5_restatement_on_tie_free_inputs(nc, kw):
    det, conf, thr, facts = R.random_case(nc)
    assert facts["tie_free"]
    if kw.get("classes"):
        kw = dict(kw, classes=[c for c in kw["classes"] if c < nc])
    want = _yolov5_best_class(det, conf, thr, **kw)
    got = R.nms_ex_ref(det, conf, thr, max_det=kw.get("max_det", 300), max_wh=0 if kw.get("agnostic") else 4096, best_class=True,
                       classes=kw.get("classes"))
    assert sum(len(w) for w in want) > 0
    _rows_equal(got, want)


def test_unletterbox_ref_is_scale_boxes_then_clip():
    """against fp64 on values where every step is exact (dyadic offsets and scales)"""
    rows = np.float32([[10.5, 20.25, 100.75, 90.5, 0.5, 1], [-4, 3, 700, 650, 0.25, 0]])
    got = R.unletterbox_ref(rows, [8, 16, 0.5, 2.0, 300, 1000])
    np.testing.assert_array_equal(got[:, :4], [[1.25, 8.5, 46.375, 149.0], [0, 0, 300, 1000]])
    np.testing.assert_array_equal(got[:, 4:], rows[:, 4:])


# ------------------------------------------------------------------------------------------------- the cases' facts
@pytest.mark.parametrize("nc", [1, 2, 80])
def test_random_case_facts(nc):
    _, _, _, f = R.random_case(nc)
    assert f["tie_free"] and min(f["best"]) > 64 and min(f["best_beyond_1024"]) > 0
    if nc == 1:
        assert f["best"] == f["multi"]
    else:
        assert all(b < m for b, m in zip(f["best"], f["multi"])) and f["rows_with_two_over_conf"] > 0


@pytest.mark.parametrize("name", list(R.hand_cases()))
def test_hand_case_facts(name):
    det, conf, thr, classes, f = R.hand_cases()[name]
    assert [len(k) for k, _ in R.keys_ex_ref(det, conf, False, classes)] == [f["multi"]]
    assert [len(k) for k, _ in R.keys_ex_ref(det, conf, True, classes)] == [f["best"]]
    best = R.nms_ex_ref(det, conf, thr, best_class=True, classes=classes)[0]
    assert sorted(best[:, 5].tolist()) == sorted(f["best_classes"])
    if name == "equal_products":
        assert f["rows_with_equal_best_products"] == 2
        # the other tie rule (highest index among equal maxima) would name classes 2 and 2
        assert sorted(best[:, 5].tolist()) == [0.0, 1.0]
    if name == "best_unlisted":
        masked = R.nms_ex_ref(det, conf, thr, best_class=False, classes=classes)[0]           # column masking keeps row 0
        assert len(masked) == 2 and len(best) == 1 and best[0, 0] == 50.0


def test_big_case_facts():
    _, _, _, f = R.big_case()
    assert 4096 < f["best"][0] <= R.BIG_ROWS
    assert f["multi_key_cap"] == 64 * R.BIG_KEY_CAP
    assert f["survivors"][0] > 0 and f["last_rank"][0] > 64


def test_counts_case_facts():
    _, _, _, f = R.counts_case()
    assert tuple(f["best"]) == R.COUNTS and f["multi"][-1] > R.COUNTS_KEY_CAP


def test_agnostic_case_facts():
    _, _, _, f = R.agnostic_case()
    assert f["with_offset"] == 3 and f["agnostic"] == 2
    assert f["agnostic_scores"] == [0.75, 0.625] and f["agnostic_classes"] == [2.0, 1.0]


def test_max_det_case_facts():
    det, conf, thr, f = R.max_det_case()
    assert f["candidates"] == 320 and f["uncapped"] == 300
    for m in R.MAX_DETS:
        assert len(R.nms_ex_ref(det, conf, thr, max_det=m, best_class=True)[0]) == m < f["candidates"]


def test_letterbox_case_facts():
    _, _, _, _, f = R.letterbox_case()
    assert f["rows"] == [6, 6, 6] and f["transforms_differ"]
    for c in f["clipped"]:
        assert all(c.values()), c


# ------------------------------------------------------------------------------------------- host side, no GPU needed
def test_nms_ex_argument_checks_name_the_entry_point():
    from object_detection_cib_amd import _lib, build
    build.build(verbose=False)
    h = _lib.lib()
    assert h.kodhip_letterbox_bytes() == 24 and h.kodhip_version() >= 103

    def call(key_cap=64, max_det=300, best=1):
        return h.kodhip_nms_ex(8, 8, key_cap, 8, 8, 8, 1, 4, 3, 0.25, 0.45, max_det, 30000, 4096.0, best, None, None, None)
    for kw, msg in ((dict(key_cap=100), b"power of two"), (dict(key_cap=32), b"power of two"), (dict(max_det=301), b"max_det"),
                    (dict(max_det=0), b"max_det"), (dict(best=2), b"best_class"), (dict(best=-1), b"best_class")):
        assert call(**kw) < 0
        err = h.kodhip_last_error()
        assert b"nms_ex" in err and msg in err, err
    assert h.kodhip_nms_ex(None, 8, 64, 8, 8, 8, 1, 4, 3, 0.25, 0.45, 300, 30000, 4096.0, 0, None, None, None) < 0


def test_public_signatures():
    from object_detection_cib_amd.core.nms import non_max_suppression
    from object_detection_cib_amd.inference import Detector
    p = inspect.signature(non_max_suppression).parameters
    assert list(p) == ["detections", "conf_thres", "nms_thres", "classes", "agnostic", "multi_label", "max_det", "letterbox"]
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("agnostic", "multi_label", "max_det", "letterbox"))
    assert (p["agnostic"].default, p["multi_label"].default, p["max_det"].default, p["letterbox"].default) == (False, None, 300, None)
    d = inspect.signature(Detector.__init__).parameters
    assert {k: d[k].default for k in list(d)[3:]} == dict(image_size=640, batch_size=16, conf_thres=0.25, iou_thres=0.45, classes=None,
                                                         agnostic=False, multi_label=False, max_det=300, graphed=False, eval_fused=None)


def test_letterbox_table_geometry_and_refusals():
    from object_detection_cib_amd.data.device_pipeline import letterbox_geometry
    from object_detection_cib_amd.inference import letterbox_table
    shapes = [(48, 64), (100, 37), (64, 64), (31, 17), (37, 100)]
    assert [letterbox_geometry(h, w, 64)[:2] for h, w in shapes] == [(48, 64), (64, 24), (64, 64), (64, 35), (24, 64)]
    descs, lb = letterbox_table(shapes, 64)
    assert lb.dtype == np.float32 and lb.shape == (5, 6)
    for (h, w), d, row in zip(shapes, descs, lb):
        nh, nw, top, left = letterbox_geometry(h, w, 64)
        assert (d["nh"], d["nw"], d["top"], d["left"]) == (nh, nw, top, left)
        assert row.tolist() == [left, top, np.float32(w / nw), np.float32(h / nh), w, h]
    assert lb[0].tolist() == [0, 8, 1, 1, 64, 48] and lb[2].tolist() == [0, 0, 1, 1, 64, 64]          # identity scale
    with pytest.raises(ValueError, match="image 7"):
        letterbox_table([(64, 64), (1, 200)], 64, first_index=6)
