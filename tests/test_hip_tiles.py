"""Tiled inference on the device: kodhip_tile_batch and kodhip_merge_detections (csrc/tiles.hip) through the C ABI with the
test's own poisoned buffers, `merge_detections`, and `TiledDetector` end to end, against the plain references of
tests/tiles_reference.py.

Everything is compared exactly, on bit patterns: the tile cut is one fp32 division per value, the merge is comparison logic
on singly rounded fp32 arithmetic (the library is built without contraction) and exact min / max.  That the merge inputs
reach what they were built for (absorptions, survivors, grown hulls, ties, the max_det cut) is asserted on the CPU
(tests/test_tiles_reference.py); the detector tests assert their own conditions on the composed reference before they
compare.  Figures are printed before they are asserted (`pytest -s`).

Measured on an MI355X: every comparison exact (0 differing values in every tile); the identity test compares 28 rows; the
detector test's nine views give 40 - 55 rows each, 139 and 41 merged rows with 203 and 58 absorbed and 69 and 17 grown hulls,
the same eager and graphed.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import predict_reference as R  # noqa: E402
import tiles_reference as T  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402
from object_detection_cib_amd.core.nms import PackedDetections, merge_detections  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.layers import get_detections  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo  # noqa: E402

ANCH = LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
GUARD, SENTINEL = 1024, -7.0
POISON_KEY = 0x5A5A5A5A5A5A5A5A
S, OVERLAP = 64, 0.25                     # o = 16 pixels


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same_rows(got, want, tag):
    assert [len(g) for g in got] == [len(w) for w in want], (tag, [len(g) for g in got], [len(w) for w in want])
    for b, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{tag} image {b}")


# ------------------------------------------------------------------------------------------------- kodhip_tile_batch
def _pool(images):
    from object_detection_cib_amd.data.device_pipeline import ImagePool
    return ImagePool(images, torch.device("cuda", 0))


def _tile_descs(pool, slots):
    from object_detection_cib_amd.inference import TILE_DESC
    d = np.zeros(len(slots), dtype=TILE_DESC)
    for k, (i, x0, y0) in enumerate(slots):
        d[k] = (pool.offsets[i], pool.shapes[i][0], pool.shapes[i][1], x0, y0)
    return torch.from_numpy(d.view(np.uint8).reshape(-1)).cuda()


def _tile_batch_direct(pool, slots, size, with_f32=True, with_pairs=True):
    """kodhip_tile_batch into guarded, sentinel-filled buffers -> (out_f32 numpy | None, out_pairs int16 numpy | None, intact)"""
    n = len(slots)
    n32, n16 = n * 3 * size * size, n * size * size * 4
    f32 = torch.full((n32 + 2 * GUARD,), SENTINEL, device="cuda")
    pairs = torch.full((n16 + 2 * GUARD,), 0x5A5A, dtype=torch.int16, device="cuda")
    d = _tile_descs(pool, slots)
    rc = _lib.lib().kodhip_tile_batch(pool.data.data_ptr(), d.data_ptr(), f32[GUARD:].data_ptr() if with_f32 else None,
                                      pairs[GUARD:].data_ptr() if with_pairs else None, n, size, stream())
    _lib.check(rc, "tile_batch")
    torch.cuda.synchronize()
    intact = all(bool((t[:GUARD] == s).all()) and bool((t[-GUARD:] == s).all()) for t, s in ((f32, SENTINEL), (pairs, 0x5A5A)))
    if not with_f32:
        intact = intact and bool((f32 == SENTINEL).all())
    if not with_pairs:
        intact = intact and bool((pairs == 0x5A5A).all())
    return (f32[GUARD:GUARD + n32].view(n, 3, size, size).cpu().numpy() if with_f32 else None,
            pairs[GUARD:GUARD + n16].view(n, size, size, 4).cpu().numpy() if with_pairs else None, intact)


IMAGES = ((100, 150, 11), (40, 50, 12))           # h, w, seed


def _images():
    return [T.noise_image(h, w, seed) for h, w, seed in IMAGES]


@pytest.mark.parametrize("size", [64, 6])          # 64: four pixels per thread; 6 (S % 4 == 2): two
def test_tile_batch_bits(size):
    images = _images()
    pool = _pool(images)
    o = int(size * OVERLAP)
    slots = [(i, x0, y0) for i, im in enumerate(images) for y0 in T.origins_ref(im.shape[0], size, o) for x0 in T.origins_ref(im.shape[1], size, o)]
    if size == 64:
        assert len(slots) == 6 + 1
        slots += [(1, -3, -2), (0, 149, 99), (0, 87, 37)]       # corners outside the image on every side; odd byte alignments
    else:
        slots = slots[::37] + [(0, 145, 95), (1, 47, 36)]
    want = np.stack([T.tile_ref(images[i], x0, y0, size) for i, x0, y0 in slots])
    got, pairs, intact = _tile_batch_direct(pool, slots, size)
    assert intact, "tile_batch wrote outside its outputs"
    diff = int((_bits(got) != _bits(want)).sum())
    print(f"TILES tile_batch S {size}: {len(slots)} slots, {diff} of {want.size} values differ")
    np.testing.assert_array_equal(_bits(got), _bits(want))
    np.testing.assert_array_equal(pairs, T.pairs_ref(want))
    if size == 64:
        pad = (np.float32(114) / np.float32(255)).view(np.uint32)
        assert (_bits(got[6][:, 40:, :]) == pad).all() and (_bits(got[6][:, :, 50:]) == pad).all()      # the 40 x 50 image's padding
    alone, none, intact = _tile_batch_direct(pool, slots, size, with_pairs=False)
    assert intact and none is None
    np.testing.assert_array_equal(_bits(alone), _bits(want))
    none, alone, intact = _tile_batch_direct(pool, slots, size, with_f32=False)
    assert intact and none is None
    np.testing.assert_array_equal(alone, pairs)


def test_tile_is_a_letterbox_at_scale_one():
    """the 64 x 64 window of a 64 x 64 image is what kodhip_val_prep_batch makes of it"""
    from object_detection_cib_amd.data.device_pipeline import DeviceValPipeline
    img = T.noise_image(64, 64, 13)
    pipe = DeviceValPipeline([img], [np.zeros((0, 4))], [np.zeros(0, np.int64)], 64, torch.device("cuda", 0))
    want, _, _ = pipe.make_batch([0])
    got, _, _ = _tile_batch_direct(_pool([img]), [(0, 0, 0)], 64)
    np.testing.assert_array_equal(_bits(got), _bits(want.cpu().numpy()))


# ------------------------------------------------------------------------------------------- kodhip_merge_detections
def _merge_direct(case, thr, metric="ios", mode="nmm", agnostic=False, max_det=300):
    """kodhip_merge_detections with the test's own buffers: the key workspace is followed by GUARD poisoned words, the
    output rows and counts are poisoned -> (rows per image, guard intact)"""
    rows = torch.from_numpy(case.rows).cuda()
    counts = torch.from_numpy(case.counts).cuda()
    vs = torch.from_numpy(case.view_start.astype(np.int32)).cuda()
    n = len(case.view_start) - 1
    key_cap = R.cap_for(int(np.diff(case.view_start).max()) * case.max_rows)
    keys = torch.full((n * key_cap + GUARD,), POISON_KEY, dtype=torch.int64, device="cuda")
    out = torch.full((n, max_det, 6), SENTINEL, device="cuda")
    nout = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = _lib.lib().kodhip_merge_detections(rows.data_ptr(), counts.data_ptr(), vs.data_ptr(), keys.data_ptr(), key_cap, out.data_ptr(),
                                            nout.data_ptr(), n, case.max_rows, max_det, dict(iou=0, ios=1)[metric], float(thr),
                                            dict(nms=0, nmm=1)[mode], int(agnostic), stream())
    _lib.check(rc, "merge_detections")
    torch.cuda.synchronize()
    k, o = nout.cpu().numpy(), out.cpu().numpy()
    assert ((0 <= k) & (k <= max_det)).all(), k
    for b in range(n):                                        # nothing written behind the kept rows
        assert (o[b, k[b]:] == SENTINEL).all()
    return [o[b, :k[b]] for b in range(n)], bool((keys[n * key_cap:] == POISON_KEY).all())


@pytest.mark.parametrize("name", T.RANDOM_CASES)
def test_merge_random_cases(name):
    case = T.random_case(name)
    for metric, mode, agnostic, max_det in T.OPTIONS:
        info = []
        want = T.merge_ref(case.rows, case.counts, case.view_start, T.THR, metric, mode, agnostic, max_det, info=info)
        assert sum(i["absorbed"] for i in info) >= 1 and sum(i["kept"] for i in info) >= 1
        got, intact = _merge_direct(case, T.THR, metric, mode, agnostic, max_det)
        print(f"TILES merge {name} {metric} {mode} agnostic {agnostic} max_det {max_det}: candidates {[i['candidates'] for i in info]} "
              f"kept {[len(g) for g in got]} absorbed {[i['absorbed'] for i in info]} grown {[i['grown'] for i in info]}")
        assert intact, "keys were written behind n_images * key_cap"
        _same_rows(got, want, f"{name} {metric} {mode} {agnostic} {max_det}")


@pytest.mark.parametrize("name", list(T.hand_cases()))
def test_merge_hand_cases(name):
    case, opt, want = T.hand_case(name)
    got, intact = _merge_direct(case, T.THR, **opt)
    assert intact
    _same_rows(got, [want], name)


def test_merge_wrapper_equals_the_direct_call():
    case = T.random_case("three")
    rows, counts = torch.from_numpy(case.rows).cuda(), torch.from_numpy(case.counts).cuda()
    for metric, mode, agnostic, max_det in T.OPTIONS[::3]:
        res = merge_detections(rows, counts, case.view_start, thres=T.THR, metric=metric, mode=mode, agnostic=agnostic, max_det=max_det)
        assert isinstance(res, PackedDetections) and tuple(res.packed.shape) == (3, max_det, 6)
        assert res.counts.cpu().tolist() == [len(r) for r in res]
        _same_rows([r.cpu().numpy() for r in res], T.merge_ref(case.rows, case.counts, case.view_start, T.THR, metric, mode, agnostic, max_det),
                   f"wrapper {metric} {mode}")
    for kw, msg in ((dict(metric="giou"), "metric"), (dict(mode="soft"), "mode"), (dict(max_det=301), "max_det"), (dict(thres=1.5), "thres")):
        with pytest.raises(ValueError, match=msg):
            merge_detections(rows, counts, case.view_start, **kw)
    with pytest.raises(ValueError, match="view_start"):
        merge_detections(rows, counts, [0, 9])
    with pytest.raises(ValueError, match="more than"):
        merge_detections(torch.empty((300, 300, 6), device="cuda"), torch.zeros(300, dtype=torch.int32, device="cuda"), [0, 300])


def test_merge_argument_errors_launch_nothing():
    case, _, _ = T.hand_case("hull_nmm")
    rows, counts = torch.from_numpy(case.rows).cuda(), torch.from_numpy(case.counts).cuda()
    vs = torch.from_numpy(case.view_start).cuda()
    for kw, msg in ((dict(max_det=301), "max_det"), (dict(metric=2), "metric"), (dict(mode=-1), "mode"), (dict(thr=1.25), "thr"),
                    (dict(key_cap=96), "key_cap"), (dict(n_images=0), "n_images")):
        a = dict(key_cap=64, n_images=1, max_det=300, metric=1, thr=0.5, mode=1)
        a.update(kw)
        keys = torch.full((256,), 3, dtype=torch.int64, device="cuda")
        out, nout = torch.full((1, 301, 6), SENTINEL, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda")
        rc = _lib.lib().kodhip_merge_detections(rows.data_ptr(), counts.data_ptr(), vs.data_ptr(), keys.data_ptr(), a["key_cap"], out.data_ptr(),
                                                nout.data_ptr(), a["n_images"], case.max_rows, a["max_det"], a["metric"], a["thr"], a["mode"], 0,
                                                stream())
        torch.cuda.synchronize()
        err = _lib.lib().kodhip_last_error().decode()
        assert rc < 0 and "merge_detections" in err and msg in err, (kw, rc, err)
        assert int(nout) == -1 and bool((out == SENTINEL).all()) and bool((keys == 3).all()), kw


# ------------------------------------------------------------------------------------------------------ TiledDetector
@pytest.fixture(scope="module")
def net():
    from test_hip_predict import _network
    return _network()


def _forward_eager(net, x):
    with torch.no_grad():
        return get_detections(FeatureShape(width=x.shape[3], height=x.shape[2]), net(x), ANCH)


def _letterbox_row(h, w, size):
    from object_detection_cib_amd.inference import letterbox_table
    return letterbox_table([(h, w)], size)[1][0]


def _slot_inputs(images, size, overlap, full_view=True):
    """the reference slot stream: (fp32 [3, S, S] per slot, KodLetterbox row per slot, view_start).  Tiles from tile_ref;
    the letterboxed full views from the validation pipeline's make_batch (kodhip_val_prep_batch, pinned by its own tests)."""
    from object_detection_cib_amd.data.device_pipeline import DeviceValPipeline
    none = [np.zeros((0, 4))] * len(images), [np.zeros(0, np.int64)] * len(images)
    pipe = DeviceValPipeline(images, none[0], none[1], size, torch.device("cuda", 0))
    xs, lbs, start = [], [], [0]
    for i, im in enumerate(images):
        for v in T.plan_ref(im.shape[0], im.shape[1], size, overlap, full_view, letterbox_row=_letterbox_row):
            xs.append(pipe.make_batch([i])[0][0].cpu().numpy() if v.full else T.tile_ref(im, v.x0, v.y0, size))
            lbs.append(v.letterbox)
        start.append(len(xs))
    return xs, np.float32(lbs), np.asarray(start, np.int32)


def _conf_for(det, k=40):
    """a confidence threshold (fp32, between two scores) that leaves about k best-class candidates in the sparsest slot"""
    s = np.sort((det[..., 5:] * det[..., 4:5]).max(-1), axis=1)[:, ::-1]
    k = min(k, s.shape[1] - 2)
    return float(np.float32((s[:, k].min() + s[:, k + 1].min()) / 2))


def _composed(xs, lbs, start, forward, batch, conf, iou, tile_max_det, **merge):
    """forward + kodhip_decode per chunk of `batch` slots (the last slot repeated), nms_ex_ref + unletterbox per slot on the
    downloaded detections, then the numpy merge"""
    n = len(xs)
    idx = list(range(n)) + [n - 1] * (-n % batch)
    views = []
    dets = []
    for c in range(0, len(idx), batch):
        x = torch.from_numpy(np.stack([xs[k] for k in idx[c:c + batch]])).cuda()
        dets.append(forward(x).cpu().numpy())
    det = np.concatenate(dets)[:n]
    for k, rows in enumerate(R.nms_ex_ref(det, conf, iou, max_det=tile_max_det, best_class=True)):
        views.append(R.unletterbox_ref(rows, lbs[k]))
    rows, counts = T.pack_views(views, tile_max_det)
    return T.merge_ref(rows, counts, start, **merge), det, [len(v) for v in views]


def test_identity_one_tile_is_the_detector():
    """nc = 1, one S x S image, no full view, merge = the NMS's own rule: nothing is left to suppress, Detector bit for bit"""
    from object_detection_cib_amd.inference import Detector, TiledDetector
    from object_detection_cib_amd.nn.networks.yolov5 import Yolov5Network
    torch.manual_seed(7)
    net1 = Yolov5Network(3, 1, widen_factor=0.25, deepen_factor=0.33)
    with torch.no_grad():
        # small boxes at the cell centres (w, h = (2 * sigmoid(-2.2))^2 = 0.04 anchors): a random-init network's boxes are as
        # large as the 64 px image, the clip of the un-letterbox launch would make them one box, and rows that the NMS kept
        # apart would suppress each other afterwards - the identity holds for boxes inside the image, as asserted below
        for name, p in net1.named_parameters():
            if name.endswith("box_head.conv.bias"):
                p.copy_(torch.tensor([0.0, 0.0, -2.2, -2.2]).repeat(p.numel() // 4))
    net1 = net1.cuda().eval()
    img = T.noise_image(S, S, 14)
    x = torch.from_numpy(T.tile_ref(img, 0, 0, S)[None]).cuda()
    conf, iou = _conf_for(_forward_eager(net1, x).cpu().numpy()), 0.45
    kw = dict(image_size=S, batch_size=2, conf_thres=conf, iou_thres=iou)
    want = [g.clone().cpu().numpy() for g in Detector(net1, ANCH, **kw)([img])]
    # the precondition, on the CPU: the clipped rows the Detector returns do not suppress each other under the same rule
    rows, counts = T.pack_views(want, 300)
    again = T.merge_ref(rows, counts, [0, 1], iou, "iou", "nms", False, 300)
    assert len(want[0]) >= 5
    _same_rows(again, want, "precondition: the merge reference leaves the Detector's rows alone")
    d = TiledDetector(net1, ANCH, full_view=False, merge="nms", merge_metric="iou", merge_thres=iou, **kw)
    got = [g.cpu().numpy() for g in d([img])]
    print(f"TILES identity: conf {conf:.6g}, rows {[len(w) for w in want]}")
    _same_rows(got, want, "identity")


@pytest.mark.parametrize("graphed", [False, True])
def test_tiled_detector_equals_the_composition(net, graphed):
    from object_detection_cib_amd.inference import TiledDetector
    images = _images()
    net.fuse_eval(False)
    xs, lbs, start = _slot_inputs(images, S, OVERLAP)
    assert start.tolist() == [0, 7, 9] and len(xs) == 9                      # 6 tiles + full view, 1 tile + full view
    batch, iou = 4, 0.45
    conf = _conf_for(_forward_eager(net, torch.from_numpy(np.stack(xs)).cuda()).cpu().numpy())
    d = TiledDetector(net, ANCH, image_size=S, batch_size=batch, overlap=OVERLAP, conf_thres=conf, iou_thres=iou, graphed=graphed)
    modes = [m.training for m in net.modules()]
    got = [g.clone().cpu().numpy() for g in d(images)]
    assert [m.training for m in net.modules()] == modes
    forward = (lambda x: d._geval[(batch, 3, S, S)](x).clone()) if graphed else (lambda x: _forward_eager(net, x))
    info_kw = dict(thr=0.5, metric="ios", mode="nmm", agnostic=False, max_det=300)
    want, det, per_view = _composed(xs, lbs, start, forward, batch, conf, iou, 300, **info_kw)
    info = []
    rows, counts = T.pack_views([R.unletterbox_ref(r, lb) for r, lb in zip(R.nms_ex_ref(det, conf, iou, best_class=True), lbs)], 300)
    T.merge_ref(rows, counts, start, info=info, **info_kw)
    print(f"TILES detector graphed {graphed}: conf {conf:.6g}, rows per view {per_view}, merged {[len(w) for w in want]}, "
          f"absorbed {[i['absorbed'] for i in info]}, grown {[i['grown'] for i in info]}")
    assert min(per_view) >= 1 and min(len(w) for w in want) >= 1 and sum(i["absorbed"] for i in info) >= 1
    assert len(got) == 2 and all(g.shape[1] == 6 for g in got)
    _same_rows(got, want, f"tiled detector graphed {graphed}")
    for g, (h, w, _) in zip(got, IMAGES):                                     # in the image's own pixels
        assert (g[:, :4] >= 0).all() and (g[:, [0, 2]] <= w).all() and (g[:, [1, 3]] <= h).all()
    if graphed:
        assert list(d._geval) == [(batch, 3, S, S)]                           # one shape set serves all three chunks
        eager = TiledDetector(net, ANCH, image_size=S, batch_size=batch, overlap=OVERLAP, conf_thres=conf, iou_thres=iou)(images)
        _same_rows(got, [e.cpu().numpy() for e in eager], "graphed against eager")


def test_tiled_detector_value_errors(net):
    from object_detection_cib_amd.inference import TiledDetector
    for kw, msg in ((dict(overlap=1.0), "overlap"), (dict(merge="soft"), "merge"), (dict(merge_metric="giou"), "merge_metric"),
                    (dict(merge_thres=2), "merge_thres"), (dict(tile_max_det=301), "tile_max_det"), (dict(image_size=100), "image_size")):
        with pytest.raises(ValueError, match=msg):
            TiledDetector(net, ANCH, **dict(dict(image_size=S), **kw))
    d = TiledDetector(net, ANCH, image_size=32, batch_size=4, overlap=0.0, full_view=False)
    limit = _lib.lib().kodhip_merge_max_rows()
    too_wide = 32 * (limit // 300 + 1)
    with pytest.raises(ValueError, match="tile_max_det"):
        d.plans([(32, too_wide)])
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="tile_max_det"):                     # refused on the plan: nothing is uploaded
        d([np.broadcast_to(np.zeros((1, 1, 3), np.uint8), (32, too_wide, 3))])
    assert torch.cuda.memory_allocated() == before
    with pytest.raises(ValueError, match="image 1"):
        d([np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64), np.uint8)])
    assert d([]) == []
