"""Test-time augmentation on the device: kodhip_tta_view (csrc/tta.hip) and kodhip_decode_view (csrc/postproc.hip) through
the C ABI with the test's own poisoned buffers, `get_detections_augmented`, GraphedAugmentedForward, AugmentedDetector
and DefaultYolov5Experiment(val_augment=True), against the plain references of tests/tta_reference.py.

What is compared how:
* the view input (`out_f32`, `out_pairs`) bit for bit: singly rounded fp32 arithmetic in a prescribed order;
* the de-scaled decode against the fp64 `descale_ref` within 2 * TTA_BOX_ULP_MEASURED ulp32 / DECODE_SCORE_REL (the device's
  expf is not numpy's), the identity view against kodhip_decode bit for bit;
* the composition: each `scale_view_ref` view is uploaded and run through the plain eval forward at its own shape and
  decoded by kodhip_decode.  The SCORES of the merged tensor equal the trimmed kodhip_decode scores bit for bit (same
  forward bits, same expf, untouched by the de-scaling), and so do the boxes of the first view (division by 1, no flip).
  The boxes of the scaled views cannot be rebuilt bit for bit on the host - kodhip_decode hands out corners, not centres, and
  the host's expf differs - so they are held to `descale_ref` of the downloaded head tensors within the decode tolerance;
* graphed against eager, Detector and validation_step against the composition of their pieces, NMS against nms_ref: bit for bit.

yv5n width, 3 classes, B = 2.  Figures are printed before they are asserted (`pytest -s`).

Measured on an MI355X: every bit-for-bit comparison exact (0 differing values in every view input); decode_view against fp64
at most 1.99 ulp32 on the constructed logits and 1.88 ulp32 behind a real forward (tolerance 6), scores at most 1.24e-7
relative (tolerance 2.38e-7); the Detector's five images give 12, 7, 13, 8 and 4 rows with augmentation (11, 7, 10, 5, 2 without).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import predict_reference as R  # noqa: E402
import tta_reference as T  # noqa: E402
import val_reference as V  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402
from object_detection_cib_amd.core.nms import non_max_suppression  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.engine.tta import tta_plan  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.layers import get_detections, get_detections_augmented  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo  # noqa: E402

ANCH = LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
GUARD, SENTINEL = 1024, -7.0
NC, B = 3, 2


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same_rows(got, want, tag):
    assert [len(g) for g in got] == [len(w) for w in want], (tag, [len(g) for g in got], [len(w) for w in want])
    for b, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{tag} image {b}")


# --------------------------------------------------------------------------------------------------- kodhip_tta_view
def _tta_view_direct(x, v, with_f32=True):
    """kodhip_tta_view into guarded, sentinel-filled buffers -> (out_f32 numpy or None, out_pairs int16 tensor, intact)"""
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    Bx, _, H, W = x.shape
    n32, n16 = Bx * 3 * v.Hp * v.Wp, Bx * v.Hp * v.Wp * 4
    f32 = torch.full((n32 + 2 * GUARD,), SENTINEL, device="cuda")
    pairs = torch.full((n16 + 2 * GUARD,), 0x5A5A, dtype=torch.int16, device="cuda")
    rc = _lib.lib().kodhip_tta_view(xd.data_ptr(), pairs[GUARD:].data_ptr(), f32[GUARD:].data_ptr() if with_f32 else None, Bx, H, W,
                                    v.h, v.w, v.Hp, v.Wp, int(v.flip), float(T.PAD), stream())
    _lib.check(rc, "tta_view")
    torch.cuda.synchronize()
    intact = all(bool((t[:GUARD] == s).all()) and bool((t[-GUARD:] == s).all()) for t, s in ((f32, SENTINEL), (pairs, 0x5A5A)))
    if not with_f32:
        intact = intact and bool((f32 == SENTINEL).all())
    out = f32[GUARD:GUARD + n32].view(Bx, 3, v.Hp, v.Wp).cpu().numpy() if with_f32 else None
    return out, pairs[GUARD:GUARD + n16].view(Bx, v.Hp, v.Wp, 4).clone(), intact


def _pairs_of(f32):
    """kodhip_nchw_to_nhwc4 of an fp32 NCHW array -> int16 [B, H, W, 4]"""
    t = torch.from_numpy(np.ascontiguousarray(f32)).cuda()
    Bx, C, H, W = t.shape
    y = torch.full((Bx, H, W, 4), 0x5A5A, dtype=torch.int16, device="cuda")
    _lib.check(_lib.lib().kodhip_nchw_to_nhwc4(t.data_ptr(), y.data_ptr(), Bx, C, H, W, stream()), "nchw_to_nhwc4")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("size", T.PLAN_SIZES)
def test_tta_view_bits(size):
    H, W = size
    x = T.image_batch(B, H, W, seed=3 * H + W)
    views, _ = T.tta_plan_ref(H, W)
    views = list(views) + [T.ViewRef(1.0, True, H, W, H, W, (0, 1, 2), 0, 0)]          # ratio 1 with a flip: h = H, w = W
    for v in views:
        want = T.scale_view_ref(x, v)
        got, pairs, intact = _tta_view_direct(x, v)
        assert intact, f"{v}: tta_view wrote outside its outputs"
        diff = int((_bits(got) != _bits(want)).sum())
        print(f"TTA view {H}x{W} ratio {v.ratio} flip {v.flip} -> {v.Hp}x{v.Wp} (image {v.h}x{v.w}): {diff} of {want.size} values differ")
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(v))
        if v.ratio != 1.0:
            assert (_bits(got[:, :, v.h:, :]) == T.PAD.view(np.uint32)).all() and (_bits(got[:, :, :, v.w:]) == T.PAD.view(np.uint32)).all()
        assert torch.equal(pairs, _pairs_of(got)), f"{v}: out_pairs is not kodhip_nchw_to_nhwc4 of out_f32"
        _, alone, intact = _tta_view_direct(x, v, with_f32=False)                        # out_f32 = NULL: the same pairs
        assert intact and torch.equal(alone, pairs)
    assert x[0, 0, 0, 0] == 0 and x[0, 0, 0, -1] == 1 and got[0, 0, 0, 0] == 1            # the flip moved the planted corner


def test_tta_view_argument_errors_launch_nothing():
    x = torch.rand(1, 3, 64, 64, device="cuda")
    lib = _lib.lib()
    for kw, msg in ((dict(h=65), "down-scaling"), (dict(w=65), "down-scaling"), (dict(Hp=32), "canvas"), (dict(Wp=32), "canvas"),
                    (dict(Wp=63, w=53), "even"), (dict(x=None), "null"), (dict(pairs=None), "null"), (dict(flip=2), "flip_lr")):
        a = dict(h=53, w=53, Hp=64, Wp=64, flip=0)
        a.update({k: v for k, v in kw.items() if k not in ("x", "pairs")})
        f32 = torch.full((3 * 64 * 64,), SENTINEL, device="cuda")
        pairs = torch.full((64 * 64 * 4,), 0x5A5A, dtype=torch.int16, device="cuda")
        rc = lib.kodhip_tta_view(None if "x" in kw else x.data_ptr(), None if "pairs" in kw else pairs.data_ptr(), f32.data_ptr(), 1, 64, 64,
                                 a["h"], a["w"], a["Hp"], a["Wp"], a["flip"], 0.447, stream())
        torch.cuda.synchronize()
        err = lib.kodhip_last_error().decode()
        assert rc < 0 and "tta_view" in err and msg in err, (kw, rc, err)
        assert bool((f32 == SENTINEL).all()) and bool((pairs == 0x5A5A).all()), kw


# ------------------------------------------------------------------------------------------------ kodhip_decode_view
def _levels(dev_raws):
    levels = (_lib.KodDecodeLevel * 3)()
    for lv, t, s, anc in zip(levels, dev_raws, V.STRIDES, V.ANCHORS):
        lv.raw, lv.h, lv.w, lv.stride = t.data_ptr(), t.shape[2], t.shape[3], s
        for k, (aw, ah) in enumerate(anc):
            lv.anchor_w[k], lv.anchor_h[k] = float(aw), float(ah)
    return levels


def _decode_view_direct(raws, v, W, merged, rows_total, mask=None, offset=None, ratio=None, flip=None):
    """kodhip_decode_view of one view into `merged` (a [B, rows_total, P] device view)"""
    dev = [r.cuda().contiguous() for r in raws]
    Bx, A, _, _, P = dev[0].shape
    mask = sum(1 << l for l in v.levels) if mask is None else mask
    rc = _lib.lib().kodhip_decode_view(_levels(dev), merged.data_ptr(), Bx, A, P - 5, v.ratio if ratio is None else ratio,
                                       int(v.flip if flip is None else flip), float(W), mask, v.row_offset if offset is None else offset,
                                       rows_total, stream())
    torch.cuda.synchronize()
    return rc


def _guarded(Bx, rows, P, fill):
    buf = torch.full((Bx * rows * P + 2 * GUARD,), fill, device="cuda")
    return buf, buf[GUARD:GUARD + Bx * rows * P].view(Bx, rows, P)


def _guards_intact(buf, fill):
    g = torch.cat((buf[:GUARD], buf[-GUARD:]))
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


@pytest.mark.parametrize("name", ["96x64_nc1_b3", "64x160_nc2_b1", "160x96_nc80_b3"])
def test_decode_view_identity_is_kodhip_decode(name):
    w, h, nc, Bx, seed = V.decode_cases()[name]
    case = V.decode_case(w, h, nc, Bx, seed)
    rows = case.facts["rows"]
    dev = [r.cuda().contiguous() for r in case.raws]
    plain = torch.full((Bx, rows, 5 + nc), SENTINEL, device="cuda")
    _lib.check(_lib.lib().kodhip_decode(_levels(dev), plain.data_ptr(), Bx, 3, nc, stream()), "decode")
    buf, out = _guarded(Bx, rows, 5 + nc, SENTINEL)
    ident = T.ViewRef(1.0, False, h, w, h, w, (0, 1, 2), 0, rows)
    assert _decode_view_direct(case.raws, ident, w, out, rows) == 0
    assert _guards_intact(buf, SENTINEL)
    assert torch.equal(out.view(torch.int32), plain.view(torch.int32))


@pytest.mark.parametrize("size", [(128, 128), (64, 128)])
def test_decode_view_writes_its_own_rows_and_nothing_else(size):
    H, W = size
    case = T.decode_view_case(H, W, NC, B, seed=500 + W)
    P, nan = 5 + NC, float("nan")
    refs = [T.descale_ref(r, v, W) for r, v in zip(case.raws, case.views)]
    all_buf, all_out = _guarded(B, case.rows, P, nan)
    for raws, v, ref in zip(case.raws, case.views, refs):
        buf, out = _guarded(B, case.rows, P, nan)
        for target in (out, all_out):
            assert _decode_view_direct(raws, v, W, target, case.rows) == 0
        assert _guards_intact(buf, nan), f"view {v.ratio}: wrote outside the merged tensor"
        got = out.cpu().numpy()
        mine = got[:, v.row_offset:v.row_offset + v.rows]
        assert not np.isnan(mine).any()
        assert np.isnan(got[:, :v.row_offset]).all() and np.isnan(got[:, v.row_offset + v.rows:]).all(), "rows of another view were written"
        box, rel = T.box_errors(mine, T.trim_ref(ref, v), W)
        print(f"TTA decode_view {H}x{W} ratio {v.ratio} flip {v.flip}: rows {v.rows} at {v.row_offset}, box {box:.3f} ulp32 (tol {T.TTA_BOX_ULP}), "
              f"score {rel:.4e} rel (tol {V.DECODE_SCORE_REL:.4e})")
        assert box <= T.TTA_BOX_ULP and rel <= V.DECODE_SCORE_REL
    assert _guards_intact(all_buf, nan)
    merged = all_out.cpu().numpy()
    assert not np.isnan(merged).any() and np.isfinite(merged).all()
    box, rel = T.box_errors(merged, T.merge_ref(refs, case.views), W)
    assert box <= T.TTA_BOX_ULP and rel <= V.DECODE_SCORE_REL


def test_decode_view_planted_boxes_land_mirrored():
    H = W = 128
    case, expected = T.planted_case(H, W, NC, 1)
    _, out = _guarded(1, case.rows, 5 + NC, float("nan"))
    for raws, v in zip(case.raws, case.views):
        assert _decode_view_direct(raws, v, W, out, case.rows) == 0
    m = out.cpu().numpy().astype(np.float64)
    assert np.nonzero(m[0, :, 4] > 0.5)[0].tolist() == [e["row"] for e in expected]
    for e in expected:
        b = m[0, e["row"], :4]
        np.testing.assert_allclose(((b[0] + b[2]) / 2, (b[1] + b[3]) / 2, b[2] - b[0], b[3] - b[1]), e["cxcywh"], rtol=1e-5)


def test_decode_view_argument_errors_launch_nothing():
    case = T.decode_view_case(128, 128, NC, 1, seed=9)
    v = case.views[2]
    for kw, msg in ((dict(mask=0), "level_mask"), (dict(mask=8), "level_mask"), (dict(offset=case.rows - v.rows + 1), "do not fit"),
                    (dict(offset=-1), "do not fit"), (dict(ratio=0.0), "scale"), (dict(flip=2), "flip_lr")):
        buf, out = _guarded(1, case.rows, 5 + NC, SENTINEL)
        rc = _decode_view_direct(case.raws[2], v, 128, out, case.rows, **kw)
        err = _lib.lib().kodhip_last_error().decode()
        assert rc < 0 and "decode_view" in err and msg in err, (kw, rc, err)
        assert bool((buf == SENTINEL).all()), kw


# ------------------------------------------------------------------------------------------------------ composition
@pytest.fixture(scope="module")
def net():
    from test_hip_predict import _network
    return _network()


def _plain(net, xv):
    """the plain eval forward + kodhip_decode of one uploaded view -> (head tensors on the host, decoded [B, rows, P] numpy)"""
    from object_detection_cib_amd.nn.heads.types import DetectionHeadResult
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5NetworkResult
    with torch.no_grad():
        raws = net.forward_raw(xv)
        res = Yolov5NetworkResult(*[DetectionHeadResult(t[..., 0:4], t[..., 4:5], t[..., 5:]) for t in raws])
        det = get_detections(FeatureShape(width=xv.shape[3], height=xv.shape[2]), res, ANCH)
    return [r.cpu() for r in raws], det.cpu().numpy()


def _conf_for(det, k=150):
    """a confidence threshold (fp32, between two scores) that leaves at least k candidates in every image: the input of the NMS
    comparison, chosen from the detections so that the comparison has rows to compare"""
    s = np.sort((det[..., 5:] * det[..., 4:5]).reshape(len(det), -1), axis=1)[:, ::-1]
    k = min(k, s.shape[1] - 2)
    return float(np.float32((s[:, k].min() + s[:, k + 1].min()) / 2))


@pytest.mark.parametrize("size", [(128, 128), (192, 192)])
def test_augmented_detections_equal_the_composition(net, size):
    H, W = size
    net.fuse_eval(False)
    x = T.image_batch(B, H, W, seed=21 + H)
    views, rows = T.tta_plan_ref(H, W)
    got = get_detections_augmented(torch.from_numpy(x).cuda(), net, ANCH)
    assert tuple(got.shape) == (B, rows, 5 + NC)
    got = got.cpu().numpy()
    assert np.isfinite(got).all()
    for v in views:
        raws, plain = _plain(net, torch.from_numpy(T.scale_view_ref(x, v)).cuda())
        mine, theirs = got[:, v.row_offset:v.row_offset + v.rows], T.trim_ref(plain, v)
        np.testing.assert_array_equal(_bits(mine[..., 4:]), _bits(theirs[..., 4:]), err_msg=f"scores of view {v.ratio}")
        if v.ratio == 1.0 and not v.flip:
            np.testing.assert_array_equal(_bits(mine), _bits(theirs), err_msg="first view")
        box, rel = T.box_errors(mine, T.trim_ref(T.descale_ref(raws, v, W), v), W)
        print(f"TTA composition {H}x{W} ratio {v.ratio}: box {box:.3f} ulp32 (tol {T.TTA_BOX_ULP}), score {rel:.4e} rel")
        assert box <= T.TTA_BOX_ULP and rel <= V.DECODE_SCORE_REL
    # one NMS over the merged tensor: comparison logic, row for row
    conf = _conf_for(got)
    want = V.nms_ref(got, conf, 0.45)
    res = non_max_suppression(torch.from_numpy(got).cuda(), conf, 0.45)
    print(f"TTA composition {H}x{W}: conf {conf:.6g}, kept {[len(w) for w in want]}")
    assert min(len(w) for w in want) >= 1
    _same_rows([r.cpu().numpy() for r in res], want, "nms of the merged tensor")


def test_graphed_equals_eager_bit_for_bit(net):
    from object_detection_cib_amd.engine.graphed import GraphedAugmentedForward
    H = W = 128
    net.fuse_eval(False)
    gf = GraphedAugmentedForward(net, ANCH, B, H, W)
    eng = net.engine()
    for seed in (31, 32, 33):                                  # capture + replay, then two replays on new batches
        x = torch.from_numpy(T.image_batch(B, H, W, seed=seed)).cuda()
        g = gf(x).clone()
        e = get_detections_augmented(x, net, ANCH)
        assert tuple(g.shape) == (B, tta_plan(H, W).rows, 5 + NC)
        assert torch.equal(g.view(torch.int32), e.view(torch.int32)), f"batch {seed}"
    assert not torch.equal(g, gf(torch.from_numpy(T.image_batch(B, H, W, seed=31)).cuda()))
    assert {(B, hp, wp) for hp, wp in tta_plan(H, W).shapes()} <= eng._pinned


# --------------------------------------------------------------------------------------------------------- Detector
@pytest.mark.parametrize("graphed", [False, True])
def test_detector_augment_equals_the_composition(net, graphed):
    from object_detection_cib_amd.data.device_pipeline import DeviceValPipeline
    from object_detection_cib_amd.inference import AugmentedDetector, Detector
    from test_hip_predict import BATCH, CONF, IOU, S, SIZES, _images, _letterbox_rows
    images = _images()
    assert len(images) == len(SIZES) and len(images) % BATCH != 0          # a partial last chunk
    net.fuse_eval(False)
    assert Detector.augment is False and AugmentedDetector.augment is True
    d = AugmentedDetector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=CONF, iou_thres=IOU, graphed=graphed)
    got = [g.clone().cpu().numpy() for g in d(images)]
    plain = [g.clone().cpu().numpy() for g in Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=CONF, iou_thres=IOU)(images)]
    none = [np.zeros((0, 4))] * len(images), [np.zeros(0, np.int64)] * len(images)
    pipe = DeviceValPipeline(images, none[0], none[1], S, torch.device("cuda", 0))
    lbs, want = _letterbox_rows(), []
    for i in range(0, len(images), BATCH):
        idx = list(range(i, min(i + BATCH, len(images))))
        n = len(idx)
        idx += [idx[-1]] * (BATCH - n)
        img, _, _ = pipe.make_batch(idx)
        det = get_detections_augmented(img, net, ANCH).cpu().numpy()
        assert det.shape[1] == tta_plan(S, S).rows
        rows = R.nms_ex_ref(det, CONF, IOU, best_class=True)
        want += [R.unletterbox_ref(r, lbs[k]) for r, k in zip(rows[:n], idx[:n])]
    print(f"TTA detector graphed {graphed}: rows per image {[len(w) for w in want]}, without augmentation {[len(p) for p in plain]}")
    assert sum(len(w) for w in want) >= 1
    _same_rows(got, want, f"detector augment graphed {graphed}")
    assert any(g.shape != p.shape or not np.array_equal(g, p) for g, p in zip(got, plain)), "augmentation changed nothing"
    if graphed:
        assert list(d._geval) == [(BATCH, 3, S, S)] and type(d._geval[(BATCH, 3, S, S)]).__name__ == "GraphedAugmentedForward"


# ------------------------------------------------------------------------------------------------------- validation
@pytest.mark.parametrize("graphed", [False, True])
def test_validation_step_val_augment(net, graphed):
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
    H = W = 128
    net.fuse_eval(False)
    x = torch.from_numpy(T.image_batch(B, H, W, seed=41)).cuda()
    det = get_detections_augmented(x, net, ANCH)
    conf = _conf_for(det.cpu().numpy())
    modes = [m.training for m in net.modules()]
    exp = DefaultYolov5Experiment(net, None, ANCH, val_nms_conf_threshold=conf, val_nms_iou_threshold=0.6, graphed=graphed, val_augment=True)
    targets, out = exp.validation_step((x, "targets", None))
    assert targets == "targets" and [m.training for m in net.modules()] == modes
    want = non_max_suppression(det, conf, 0.6)
    print(f"TTA validation_step graphed {graphed}: conf {conf:.6g}, kept {[len(w) for w in want]}")
    assert min(len(w) for w in want) >= 1
    _same_rows([o.cpu().numpy() for o in out], [w.cpu().numpy() for w in want], "validation_step val_augment")
    # val_augment=False is the experiment without the keyword
    off = DefaultYolov5Experiment(net, None, ANCH, val_nms_conf_threshold=conf, val_nms_iou_threshold=0.6, graphed=graphed, val_augment=False)
    base = DefaultYolov5Experiment(net, None, ANCH, val_nms_conf_threshold=conf, val_nms_iou_threshold=0.6, graphed=graphed)
    a = [o.clone().cpu().numpy() for o in off.validation_step((x, None, None))[1]]
    b = [o.clone().cpu().numpy() for o in base.validation_step((x, None, None))[1]]
    _same_rows(a, b, "val_augment=False")
    assert any(len(p) != len(q) or not np.array_equal(p, q) for p, q in zip(a, [o.cpu().numpy() for o in out]))


# -------------------------------------------------------------------------------------------------------- shape sets
def test_three_view_shapes_fit_beside_a_pinned_training_set():
    """320 px: three DISTINCT view shapes (320, 288, 224) + the training shape = the default KODHIP_MAX_SHAPE_SETS"""
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    torch.manual_seed(13)
    net = Yolov5Network(3, NC, widen_factor=0.25, deepen_factor=0.33).cuda()
    eng = net.engine()
    assert eng.max_shape_sets == 4
    plan = tta_plan(320, 320)
    assert plan.shapes() == [(320, 320), (288, 288), (224, 224)]
    with torch.no_grad():
        eng.forward(torch.rand(B, 3, 96, 96, device="cuda"), training=True)          # the training-shape set, built by a training forward
    eng.pin_shape(B, 96, 96)
    train_set = eng._sets[(B, 96, 96)]
    net.eval()
    x = torch.from_numpy(T.image_batch(B, 320, 320, seed=51)).cuda()
    first = get_detections_augmented(x, net, ANCH).clone()
    kept = dict(eng._sets)
    second = get_detections_augmented(x, net, ANCH)
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    assert set(eng._sets) == {(B, 96, 96)} | {(B, hp, wp) for hp, wp in plan.shapes()} and len(eng._sets) == 4
    assert all(eng._sets[k] is v for k, v in kept.items()), "a view's set was dropped and rebuilt between two augmented forwards"
    assert eng._sets[(B, 96, 96)] is train_set
