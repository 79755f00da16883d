"""The inference post-process and the Detector on the device: kodhip_nms_ex (csrc/postproc.hip) through the C ABI with the
test's own poisoned buffers, through `non_max_suppression`'s keywords, and end to end through
`object_detection_cib_amd.inference.Detector`, against the plain references of tests/predict_reference.py.

Everything is compared exactly, on fp32 bit patterns: every stage is comparison logic or singly rounded fp32 arithmetic
(the library is built without contraction), as in tests/test_hip_val_edges.py.  That every input reaches what it was
built for is asserted on the CPU (tests/test_predict_reference.py); the Detector test asserts its own conditions on the
composed reference before it compares.  Figures are printed before they are asserted (`pytest -s`).

Measured on an MI355X: every comparison exact; the Detector test's five images give 11, 7, 10, 5 and 2 rows (5, 5, 5, 5, 2 with
max_det = 5).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import predict_reference as R  # noqa: E402
import val_reference as V  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402
from object_detection_cib_amd.core.nms import PackedDetections, non_max_suppression  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.data.device_pipeline import DeviceValPipeline, letterbox_geometry  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.layers import get_detections  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo  # noqa: E402

ANCH = LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
GUARD = 1024
POISON_KEY = 0x5A5A5A5A5A5A5A5A


def _nms_ex_direct(det, conf, thr, key_cap, max_det=300, max_nms=30000, max_wh=4096.0, best_class=False, classes=None,
                   letterbox=None, entry="kodhip_nms_ex"):
    """kodhip_nms_ex (or kodhip_nms) with the test's own buffers: the key workspace is followed by GUARD poisoned words,
    the output rows and counts are poisoned.  -> dict(ncand, keys [B, key_cap] uint64, rows, nout, guard_intact)"""
    d = torch.from_numpy(np.ascontiguousarray(det, dtype=np.float32)).cuda()
    B, rows, P = d.shape
    keys = torch.full((B * key_cap + GUARD,), POISON_KEY, dtype=torch.int64, device="cuda")
    ncand = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    nout = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    out = torch.full((B, max_det, 6), -7.0, device="cuda")
    args = [d.data_ptr(), keys.data_ptr(), key_cap, ncand.data_ptr(), out.data_ptr(), nout.data_ptr(), B, rows, P - 5, float(conf),
            float(thr), max_det, max_nms, float(max_wh)]
    if entry == "kodhip_nms_ex":
        keep = lb = None
        if classes is not None:
            k = np.zeros(P - 5, np.uint8); k[list(classes)] = 1
            keep = torch.from_numpy(k).cuda()
        if letterbox is not None:
            lb = torch.from_numpy(np.ascontiguousarray(letterbox, dtype=np.float32)).cuda()
            assert tuple(lb.shape) == (B, 6)
        args += [1 if best_class else 0, keep.data_ptr() if keep is not None else None, lb.data_ptr() if lb is not None else None]
    _lib.check(getattr(_lib.lib(), entry)(*args, stream()), entry)
    torch.cuda.synchronize()
    k = keys.cpu().numpy().view(np.uint64)
    n = nout.cpu().numpy()
    o = out.cpu().numpy()
    assert ((0 <= n) & (n <= max_det)).all(), n
    for b in range(B):                                       # nothing written behind the survivors
        assert (o[b, n[b]:] == -7.0).all()
    return dict(ncand=ncand.cpu().numpy(), keys=k[:B * key_cap].reshape(B, key_cap), rows=[o[b, :n[b]] for b in range(B)],
                nout=n, guard_intact=bool((k[B * key_cap:] == np.uint64(POISON_KEY)).all()))


def _same_rows(got, want, tag):
    assert [len(g) for g in got] == [len(w) for w in want], (tag, [len(g) for g in got], [len(w) for w in want])
    for b, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(np.asarray(g, np.float32).view(np.uint32), np.asarray(w, np.float32).view(np.uint32),
                                      err_msg=f"{tag} image {b}")


def _check(tag, det, conf, thr, key_cap, **kw):
    """direct call vs nms_ex_ref: candidate counts, sorted keys, rows, guard"""
    best, classes = kw.get("best_class", False), kw.get("classes")
    ref_keys = R.keys_ex_ref(det, conf, best, classes)
    want = R.nms_ex_ref(det, conf, thr, key_cap=key_cap, **kw)
    r = _nms_ex_direct(det, conf, thr, key_cap, **kw)
    print(f"PREDICT {tag}: candidates {r['ncand'].tolist()} kept {r['nout'].tolist()}")
    assert r["guard_intact"], f"{tag}: keys were written behind B * key_cap"
    np.testing.assert_array_equal(r["ncand"], [min(len(k), key_cap) for k, _ in ref_keys], err_msg=tag)
    for b, (k, _) in enumerate(ref_keys):
        np.testing.assert_array_equal(r["keys"][b, :min(len(k), key_cap)], np.sort(k[:key_cap]), err_msg=f"{tag}: sorted keys of image {b}")
    _same_rows(r["rows"], want, tag)
    return r, want


def _wrapper(det, conf, thr, **kw):
    res = non_max_suppression(torch.from_numpy(np.ascontiguousarray(det, dtype=np.float32)).cuda(), conf, thr, **kw)
    assert isinstance(res, PackedDetections) and tuple(res.packed.shape) == (len(det), kw.get("max_det", 300), 6)
    assert res.counts.cpu().tolist() == [len(r) for r in res]
    return [r.cpu().numpy() for r in res]


# ------------------------------------------------------------------------------------------------------ C ABI
def test_options_off_is_kodhip_nms_bit_for_bit():
    """best_class = 0, class_keep = NULL, letterbox = NULL: the rows AND the sorted key workspace of kodhip_nms"""
    for det, conf, thr in (V.ties_case()[:3], V.sort_reach_case()[:3], V.wrapper_case()):
        cap = R.cap_for(det.shape[1] * (det.shape[2] - 5))
        a = _nms_ex_direct(det, conf, thr, cap, entry="kodhip_nms")
        b = _nms_ex_direct(det, conf, thr, cap)
        assert a["guard_intact"] and b["guard_intact"]
        np.testing.assert_array_equal(a["ncand"], b["ncand"])
        np.testing.assert_array_equal(a["keys"], b["keys"])
        _same_rows(b["rows"], a["rows"], "options off")
        _same_rows(b["rows"], V.nms_ref(det, conf, thr), "options off vs nms_ref")


@pytest.mark.parametrize("nc", [1, 2, 80])
def test_best_class_random_scenes(nc):
    det, conf, thr, facts = R.random_case(nc)
    rows = det.shape[1]
    r, _ = _check(f"best nc {nc}", det, conf, thr, R.cap_for(rows), best_class=True)
    assert r["ncand"].tolist() == facts["best"]
    _check(f"multi nc {nc}", det, conf, thr, R.cap_for(rows * nc))
    assert (r["ncand"] <= rows).all()


@pytest.mark.parametrize("name", list(R.hand_cases()))
def test_best_class_hand_cases(name):
    det, conf, thr, classes, f = R.hand_cases()[name]
    best, _ = _check(name + " best", det, conf, thr, 64, best_class=True, classes=classes)
    multi, _ = _check(name + " multi", det, conf, thr, 64, classes=classes)
    assert best["ncand"].tolist() == [f["best"]] and multi["ncand"].tolist() == [f["multi"]]
    assert sorted(best["rows"][0][:, 5].tolist()) == sorted(float(c) for c in f["best_classes"])
    if classes is not None:                                   # class_keep in multi-label mode = today's column masking
        _same_rows(multi["rows"], V.nms_ref(det, conf, thr, classes=classes), name + " masking")


def test_best_class_5000_rows_in_an_8192_key_workspace():
    det, conf, thr, facts = R.big_case()
    assert 4096 < facts["best"][0] <= R.BIG_KEY_CAP == facts["multi_key_cap"] // 64
    r, _ = _check("big", det, conf, thr, R.BIG_KEY_CAP, best_class=True)
    assert r["ncand"].tolist() == facts["best"] and r["nout"].tolist() == facts["survivors"]


def test_best_class_candidate_counts_0_1_64_65_key_cap_in_one_batch():
    det, conf, thr, facts = R.counts_case()
    assert tuple(facts["best"]) == R.COUNTS
    r, _ = _check("counts", det, conf, thr, R.COUNTS_KEY_CAP, best_class=True)
    assert tuple(r["ncand"].tolist()) == R.COUNTS


def test_agnostic_is_max_wh_zero():
    det, conf, thr, f = R.agnostic_case()
    off, _ = _check("class offset", det, conf, thr, 64, best_class=True)
    agn, _ = _check("agnostic", det, conf, thr, 64, best_class=True, max_wh=0.0)
    assert off["nout"].tolist() == [3] and agn["nout"].tolist() == [2]
    assert agn["rows"][0][:, 4].tolist() == f["agnostic_scores"] == [0.75, 0.625]
    _same_rows(_wrapper(det, conf, thr, agnostic=True, multi_label=False), agn["rows"], "agnostic wrapper")
    _same_rows(_wrapper(det, conf, thr, multi_label=False), off["rows"], "offset wrapper")


@pytest.mark.parametrize("max_det", R.MAX_DETS)
def test_max_det_caps_the_output(max_det):
    det, conf, thr, f = R.max_det_case()
    for best in (True, False):
        r, _ = _check(f"max_det {max_det} best {best}", det, conf, thr, R.cap_for(det.shape[1] * 2), best_class=best, max_det=max_det)
        assert r["nout"].tolist() == [max_det] and f["candidates"] > max_det
    _same_rows(_wrapper(det, conf, thr, max_det=max_det), r["rows"], "max_det wrapper")


def test_letterbox_maps_and_clips_per_image():
    det, conf, thr, lbs, f = R.letterbox_case()
    assert f["transforms_differ"] and all(all(c.values()) for c in f["clipped"])
    for best in (True, False):
        r, want = _check(f"letterbox best {best}", det, conf, thr, 64, best_class=best, letterbox=lbs)
        plain = _nms_ex_direct(det, conf, thr, 64, best_class=best)
        for b, lb in enumerate(lbs):                         # scores and classes pass through; the boxes moved
            np.testing.assert_array_equal(r["rows"][b][:, 4:], plain["rows"][b][:, 4:])
            assert (r["rows"][b][:, :4] >= 0).all() and (r["rows"][b][:, [0, 2]] <= lb[4]).all() and (r["rows"][b][:, [1, 3]] <= lb[5]).all()
            assert not np.array_equal(r["rows"][b][:, :4], plain["rows"][b][:, :4])
    want = R.nms_ex_ref(det, conf, thr, best_class=True, letterbox=lbs)
    _same_rows(_wrapper(det, conf, thr, multi_label=False, letterbox=lbs), want, "letterbox wrapper (array)")
    _same_rows(_wrapper(det, conf, thr, multi_label=False, letterbox=torch.from_numpy(lbs)), want, "letterbox wrapper (tensor)")


def test_identity_letterbox_changes_no_bit():
    det, conf, thr, _ = R.random_case(2)
    cap = R.cap_for(det.shape[1])
    plain = _nms_ex_direct(det, conf, thr, cap, best_class=True)
    ident = _nms_ex_direct(det, conf, thr, cap, best_class=True, letterbox=R.identity_letterbox(len(det)))
    assert min(plain["nout"]) > 0 and min(float(r[:, :4].min()) for r in plain["rows"]) >= 0
    _same_rows(ident["rows"], plain["rows"], "identity")


def test_nms_ex_argument_checks_launch_nothing():
    det = V.hand_cases()["iou_equals_thr"].det
    for kw, msg in ((dict(key_cap=100), "power of two"), (dict(key_cap=32), "power of two"), (dict(max_det=301), "max_det"),
                    (dict(max_det=0), "max_det"), (dict(best=2), "best_class")):
        d = torch.from_numpy(det).cuda()
        keys = torch.full((256,), 3, dtype=torch.int64, device="cuda")
        nc_, no_ = torch.full((1,), -1, dtype=torch.int32, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda")
        out = torch.full((1, 301, 6), -7.0, device="cuda")
        rc = _lib.lib().kodhip_nms_ex(d.data_ptr(), keys.data_ptr(), kw.get("key_cap", 64), nc_.data_ptr(), out.data_ptr(), no_.data_ptr(),
                                      1, det.shape[1], det.shape[2] - 5, 0.25, 0.45, kw.get("max_det", 300), 30000, 4096.0,
                                      kw.get("best", 1), None, None, stream())
        torch.cuda.synchronize()
        err = _lib.lib().kodhip_last_error().decode()
        assert rc < 0 and "nms_ex" in err and msg in err, (rc, err)
        assert int(nc_) == -1 and int(no_) == -1 and bool((out == -7.0).all()) and bool((keys == 3).all())


# ----------------------------------------------------------------------------------------------------- wrapper
def test_wrapper_keywords_equal_the_direct_call():
    det, conf, thr = V.wrapper_case()
    rows, nc = det.shape[1], det.shape[2] - 5
    lbs = np.float32([[10, 20, 1.5, 1.25, 700, 500], [0, 0, 1, 1, 640, 640], [64, 0, 0.37, 0.41, 200, 260]])
    cases = [(dict(multi_label=False), dict(best_class=True)),
             (dict(multi_label=True), dict()),
             (dict(multi_label=False, classes=[1, 4]), dict(best_class=True, classes=[1, 4])),
             (dict(multi_label=True, classes=[1, 4]), dict(classes=[1, 4])),
             (dict(agnostic=True), dict(max_wh=0.0)),
             (dict(max_det=7), dict(max_det=7)),
             (dict(letterbox=lbs, classes=(5,)), dict(letterbox=lbs, classes=[5])),
             (dict(multi_label=False, agnostic=True, max_det=20, classes=[0, 2, 3], letterbox=lbs),
              dict(best_class=True, max_wh=0.0, max_det=20, classes=[0, 2, 3], letterbox=lbs))]
    for kw, direct in cases:
        cap = R.cap_for(rows if direct.get("best_class") else rows * nc)
        want = R.nms_ex_ref(det, conf, thr, **direct)
        _same_rows(_nms_ex_direct(det, conf, thr, cap, **direct)["rows"], want, f"direct {direct.keys()}")
        _same_rows(_wrapper(det, conf, thr, **kw), want, f"wrapper {kw.keys()}")


def test_wrapper_defaults_are_todays_function():
    det, conf, thr = V.wrapper_case()
    _same_rows(_wrapper(det, conf, thr), V.nms_ref(det, conf, thr), "defaults")
    _same_rows(_wrapper(det, conf, thr, classes=[1, 4]), V.nms_ref(det, conf, thr, classes=[1, 4]), "defaults, classes")
    cap = R.cap_for(det.shape[1] * (det.shape[2] - 5))
    _same_rows(_wrapper(det, conf, thr), _nms_ex_direct(det, conf, thr, cap, entry="kodhip_nms")["rows"], "defaults vs kodhip_nms")


def test_wrapper_value_errors():
    det, conf, thr = V.wrapper_case()
    d = torch.from_numpy(det).cuda()
    for bad in (0, 301, -1):
        with pytest.raises(ValueError, match="max_det"):
            non_max_suppression(d, conf, thr, max_det=bad)
    with pytest.raises(ValueError, match="letterbox"):
        non_max_suppression(d, conf, thr, letterbox=np.zeros((2, 6), np.float32))


# ---------------------------------------------------------------------------------------------------- Detector
SIZES = ((48, 64), (100, 37), (64, 64), (31, 17), (37, 100))          # h x w
S, BATCH, NC = 64, 4, 3
CONF, IOU = 0.25, 0.05          # (IoU 0.05: the boxes of neighbouring cells in the padding of image 4 suppress each other)
IMAGE_RANGES = ((0, 256), (0, 48), (0, 256), (208, 256), (96, 160))
OBJ_BIAS, OBJ_GAIN, CLS_BIAS = -10.8, 2.0 ** 23, (1.0, 0.5, 1.5)


def _images(seed=3, ranges=None):
    """one uint8 noise image per entry of SIZES, image k drawn from [lo_k, hi_k) (IMAGE_RANGES: from full-range noise to
    nearly flat dark and bright ones, so that the network answers the images differently)"""
    rng = np.random.default_rng(seed)
    return [rng.integers(lo, hi, (h, w, 3), dtype=np.uint8) for (h, w), (lo, hi) in zip(SIZES, ranges or IMAGE_RANGES)]


def _network(seed=5, obj_bias=OBJ_BIAS, obj_gain=OBJ_GAIN):
    """random-init yv5n-width network, 3 classes, set up so that detections exist and their number depends on the image.
    With the initial BatchNorm statistics (mean 0, variance 1) the activations shrink from layer to layer and the network is
    nearly linear in the image: the objectness logits are a few 1e-6, larger for a bright image than for a dark one.  The
    objectness weights times 2^23 (exact in bf16) bring them to about 10 - 34 at each image's best rows, the objectness bias
    puts the threshold between them, and the class biases make class 2 the usual best class."""
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    torch.manual_seed(seed)
    net = Yolov5Network(3, NC, widen_factor=0.25, deepen_factor=0.33)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("obj_head.conv.bias"):
                p.fill_(obj_bias)
            elif name.endswith("obj_head.conv.weight"):
                p.mul_(obj_gain)
            elif name.endswith("cls_head.conv.bias"):
                p.copy_(torch.tensor(CLS_BIAS).repeat(p.numel() // NC))
    return net.cuda().eval()


def _letterbox_rows():
    rows = []
    for h, w in SIZES:
        nh, nw, top, left = letterbox_geometry(h, w, S)
        rows.append([left, top, np.float32(w / nw), np.float32(h / nh), w, h])
    return np.float32(rows)


def _composed(net, images, forward, max_det, **kw):
    """DeviceValPipeline.make_batch -> `forward` -> nms_ex_ref on the downloaded detections -> unletterbox_ref, in chunks of
    BATCH with the last image repeated"""
    none = [np.zeros((0, 4))] * len(images), [np.zeros(0, np.int64)] * len(images)
    pipe = DeviceValPipeline(images, none[0], none[1], S, torch.device("cuda", 0))
    lbs = _letterbox_rows()
    out = []
    for i in range(0, len(images), BATCH):
        idx = list(range(i, min(i + BATCH, len(images))))
        n = len(idx)
        idx += [idx[-1]] * (BATCH - n)
        img, _, _ = pipe.make_batch(idx)
        det = forward(img).cpu().numpy()
        rows = R.nms_ex_ref(det, CONF, IOU, max_det=max_det, best_class=True, **kw)
        out += [R.unletterbox_ref(r, lbs[k]) for r, k in zip(rows[:n], idx[:n])]
    return out


def _eager(net):
    def forward(img):
        with torch.no_grad():
            return get_detections(FeatureShape(width=S, height=S), net(img), ANCH)
    return forward


@pytest.fixture(scope="module")
def net():
    return _network()


def test_detector_letterboxed_sizes():
    assert [letterbox_geometry(h, w, S)[:2] for h, w in SIZES] == [(48, 64), (64, 24), (64, 64), (64, 35), (24, 64)]


@pytest.mark.parametrize("max_det", [300, 5])
def test_detector_equals_the_composition(net, max_det):
    from object_detection_cib_amd.inference import Detector
    images = _images()
    net.fuse_eval(False)
    want = _composed(net, images, _eager(net), max_det)
    counts = [len(w) for w in want]
    print(f"PREDICT detector max_det {max_det}: rows per image {counts}")
    assert min(counts) >= 1
    if max_det == 5:
        assert max(counts) == 5 and min(counts) < 5
    modes = [m.training for m in net.modules()]
    got = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=CONF, iou_thres=IOU, max_det=max_det)(images)
    assert [m.training for m in net.modules()] == modes
    assert len(got) == len(images) and all(g.shape[1] == 6 for g in got)
    _same_rows([g.cpu().numpy() for g in got], want, f"detector max_det {max_det}")
    for g, (h, w) in zip(got, SIZES):                       # in the image's own pixels
        g = g.cpu().numpy()
        assert (g[:, :4] >= 0).all() and (g[:, [0, 2]] <= w).all() and (g[:, [1, 3]] <= h).all()


def test_detector_options_reach_the_nms(net):
    from object_detection_cib_amd.inference import Detector
    images = _images()
    net.fuse_eval(False)
    want = _composed(net, images, _eager(net), 300, classes=[0, 2], max_wh=0)
    got = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=CONF, iou_thres=IOU, classes=[0, 2], agnostic=True)(images)
    _same_rows([g.cpu().numpy() for g in got], want, "detector classes + agnostic")
    # a train-mode network comes back in train mode, every submodule with its own mode
    net.train()
    next(net.children()).eval()
    modes = [m.training for m in net.modules()]
    again = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=CONF, iou_thres=IOU, classes=[0, 2], agnostic=True)(images[:2])
    assert [m.training for m in net.modules()] == modes
    net.eval()
    _same_rows([g.cpu().numpy() for g in again], want[:2], "detector on a train-mode network")


def test_detector_eval_fused(net):
    from object_detection_cib_amd.inference import Detector
    images = _images()
    got = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=CONF, iou_thres=IOU, eval_fused=True)(images)
    assert net.engine().opt.eval_fused is True
    want = _composed(net, images, _eager(net), 300)               # the fused forward, through the same composition
    net.fuse_eval(False)
    assert min(len(w) for w in want) >= 1
    _same_rows([g.cpu().numpy() for g in got], want, "detector eval_fused")


def test_detector_graphed(net):
    from object_detection_cib_amd.inference import Detector
    images = _images()
    net.fuse_eval(False)
    d = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=CONF, iou_thres=IOU, graphed=True)
    got = [g.clone() for g in d(images)]
    assert list(d._geval) == [(BATCH, 3, S, S)]                  # one shape set serves the full and the padded chunk
    gf = d._geval[(BATCH, 3, S, S)]
    want = _composed(net, images, lambda img: gf(img).clone(), 300)
    assert min(len(w) for w in want) >= 1
    _same_rows([g.cpu().numpy() for g in got], want, "detector graphed")


def test_detector_value_errors(net):
    from object_detection_cib_amd.inference import Detector
    with pytest.raises(ValueError, match="image_size"):
        Detector(net, ANCH, image_size=100)
    with pytest.raises(ValueError, match="max_det"):
        Detector(net, ANCH, image_size=S, max_det=301)
    d = Detector(net, ANCH, image_size=S, batch_size=BATCH)
    with pytest.raises(ValueError, match="image 1"):
        d([np.zeros((64, 64, 3), np.uint8), np.zeros((1, 200, 3), np.uint8)])
    with pytest.raises(ValueError, match="image 0"):
        d([np.zeros((64, 64), np.uint8)])
    assert d([]) == []
