"""Weighted boxes fusion on the device: kodhip_fuse_detections (csrc/fusion.hip) through the C ABI with the test's own poisoned
buffers, `fuse_detections`, and `EnsembleDetector` end to end, against the plain reference of tests/fusion_reference.py.

The kernel is compared with the reference exactly, on bit patterns: the fusion is comparison logic and singly rounded fp32
arithmetic (the library is built without contraction; fp32 division is correctly rounded).  That the inputs reach what they
were built for (joins that are not the first cluster over the threshold, clusters with more members than W, a final order
that differs from the creation order, the max_det cut, more than 2048 candidates and 300 clusters) is asserted on the CPU
(tests/test_fusion_reference.py); the detector tests assert their own conditions before they compare.  Figures are printed
before they are asserted (`pytest -s`).

Measured on an MI355X: every comparison exact; the large case fuses 2284 candidates into 454 clusters; the two-network detector
test fuses 130 - 168 candidates per image (83 - 110 and 41 - 58 rows from the members) into 118 - 147 rows, the same eager and
graphed; the twins test compares 82 / 41 / 82 / 105 / 65 rows, boxes at most 1 ulp apart.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fusion_helpers as H  # noqa: E402
import fusion_reference as fr  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402
from object_detection_cib_amd.core.nms import PackedDetections, fuse_detections, non_max_suppression  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.layers import get_detections  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo  # noqa: E402

ANCH = LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
GUARD, SENTINEL = 1024, -7.0
POISON_KEY = 0x5A5A5A5A5A5A5A5A


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _same_rows(got, want, tag):
    assert [len(g) for g in got] == [len(w) for w in want], (tag, [len(g) for g in got], [len(w) for w in want])
    for b, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{tag} image {b}")


def _cap_for(n):
    cap = 64
    while cap < n:
        cap <<= 1
    return cap


# -------------------------------------------------------------------------------------------- kodhip_fuse_detections
def _fuse_direct(case, weights=None, thr=fr.THR, agnostic=False, max_det=300, key_cap=None):
    """kodhip_fuse_detections with the test's own buffers: the key workspace is followed by GUARD poisoned words, the output
    rows and counts are poisoned -> (rows per image, guard intact)"""
    rows = torch.from_numpy(case.rows).cuda()
    counts = torch.from_numpy(case.counts).cuda()
    vs = torch.from_numpy(case.view_start.astype(np.int32)).cuda()
    w = torch.from_numpy(np.ones(len(case.counts), np.float32) if weights is None else np.asarray(weights, np.float32)).cuda()
    n = len(case.view_start) - 1
    key_cap = key_cap or _cap_for(int(np.diff(case.view_start).max()) * case.max_rows)
    keys = torch.full((n * key_cap + GUARD,), POISON_KEY, dtype=torch.int64, device="cuda")
    out = torch.full((n, max_det, 6), SENTINEL, device="cuda")
    nout = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    rc = _lib.lib().kodhip_fuse_detections(rows.data_ptr(), counts.data_ptr(), vs.data_ptr(), w.data_ptr(), keys.data_ptr(), key_cap,
                                           out.data_ptr(), nout.data_ptr(), n, case.max_rows, max_det, float(thr), int(agnostic), stream())
    _lib.check(rc, "fuse_detections")
    torch.cuda.synchronize()
    k, o = nout.cpu().numpy(), out.cpu().numpy()
    assert ((0 <= k) & (k <= max_det)).all(), k
    for b in range(n):                                        # nothing written behind the emitted rows
        assert (o[b, k[b]:] == SENTINEL).all()
    return [o[b, :k[b]] for b in range(n)], bool((keys[n * key_cap:] == POISON_KEY).all())


@functools.lru_cache(maxsize=None)
def _random_want(name, weights, agnostic, max_det):
    case = fr.random_case(name)
    info = []
    return fr.fuse_ref(case.rows, case.counts, case.view_start, fr.case_weights(case, weights), fr.THR, agnostic, max_det, info=info), info


@pytest.mark.parametrize("name", fr.RANDOM_CASES)
def test_fuse_random_cases(name):
    case = fr.random_case(name)
    for weights, agnostic, max_det in fr.OPTIONS:
        want, info = _random_want(name, weights, agnostic, max_det)
        got, intact = _fuse_direct(case, fr.case_weights(case, weights), fr.THR, agnostic, max_det)
        print(f"FUSION {name} weights {weights} agnostic {agnostic} max_det {max_det}: candidates {[i['candidates'] for i in info]} "
              f"clusters {[i['clusters'] for i in info]} emitted {[len(g) for g in got]} not-first joins {[i['not_first'] for i in info]} "
              f"crowded {[i['crowded'] for i in info]}")
        assert intact, "keys were written behind n_images * key_cap"
        _same_rows(got, want, f"{name} {weights} {agnostic} {max_det}")


@pytest.mark.parametrize("name", sorted(fr.hand_cases()))
def test_fuse_hand_cases(name):
    case, opt, closed = fr.hand_case(name)
    want = fr.fuse_ref(case.rows, case.counts, case.view_start, opt["weights"], opt["thr"], opt["agnostic"], opt["max_det"])
    got, intact = _fuse_direct(case, opt["weights"], opt["thr"], opt["agnostic"], opt["max_det"])
    assert intact
    _same_rows(got, want, name)
    np.testing.assert_allclose(got[0].astype(np.float64), closed, rtol=1e-6, atol=0)      # (the closed form, as on the CPU)


def test_fuse_wrapper_equals_the_direct_call():
    case = fr.random_case("three")
    rows, counts = torch.from_numpy(case.rows).cuda(), torch.from_numpy(case.counts).cuda()
    for weights, agnostic, max_det in fr.OPTIONS[::3]:
        w = fr.case_weights(case, weights)
        res = fuse_detections(rows, counts, case.view_start, None if weights == "unit" else w, thres=fr.THR, agnostic=agnostic, max_det=max_det)
        assert isinstance(res, PackedDetections) and tuple(res.packed.shape) == (3, max_det, 6)
        assert res.counts.cpu().tolist() == [len(r) for r in res]
        direct, _ = _fuse_direct(case, w, fr.THR, agnostic, max_det)
        _same_rows([r.cpu().numpy() for r in res], direct, f"wrapper {weights} {agnostic} {max_det}")
        _same_rows(direct, _random_want("three", weights, agnostic, max_det)[0], "direct")
    V = len(case.counts)
    for kw, msg in ((dict(max_det=301), "max_det"), (dict(max_det=0), "max_det"), (dict(thres=1.5), "thres"), (dict(weights=[1.0] * (V - 1)), "weights"),
                    (dict(weights=[0.0] + [1.0] * (V - 1)), "weights"), (dict(weights=[np.inf] + [1.0] * (V - 1)), "weights"),
                    (dict(weights=[np.nan] + [1.0] * (V - 1)), "weights"), (dict(view_start=[0, 9]), "view_start")):
        a = dict(dict(view_start=case.view_start, weights=None), **kw)
        with pytest.raises(ValueError, match=msg):
            fuse_detections(rows, counts, a.pop("view_start"), a.pop("weights"), **a)
    with pytest.raises(ValueError, match="rows"):
        fuse_detections(rows[..., :5], counts, case.view_start)
    limit = _lib.lib().kodhip_fuse_max_rows()
    assert limit == 4096
    with pytest.raises(ValueError, match="more than"):
        fuse_detections(torch.empty((14, 300, 6), device="cuda"), torch.zeros(14, dtype=torch.int32, device="cuda"), [0, 14])


def test_fuse_argument_errors_launch_nothing():
    case, _, _ = fr.hand_case("pair")
    rows, counts = torch.from_numpy(case.rows).cuda(), torch.from_numpy(case.counts).cuda()
    vs = torch.from_numpy(case.view_start).cuda()
    w = torch.ones(2, device="cuda")
    for kw, msg in ((dict(max_det=301), "max_det"), (dict(max_det=0), "max_det"), (dict(agnostic=2), "agnostic"), (dict(thr=1.25), "thr"),
                    (dict(thr=-0.5), "thr"), (dict(key_cap=96), "key_cap"), (dict(key_cap=8192), "key_cap"), (dict(key_cap=32), "key_cap"),
                    (dict(n_images=0), "n_images"), (dict(max_rows=0), "max_rows"), (dict(w=None), "null")):
        a = dict(key_cap=64, n_images=1, max_det=300, thr=0.55, agnostic=0, max_rows=case.max_rows, w=w.data_ptr())
        a.update(kw)
        keys = torch.full((8192 + 256,), 3, dtype=torch.int64, device="cuda")
        out, nout = torch.full((1, 301, 6), SENTINEL, device="cuda"), torch.full((1,), -1, dtype=torch.int32, device="cuda")
        rc = _lib.lib().kodhip_fuse_detections(rows.data_ptr(), counts.data_ptr(), vs.data_ptr(), a["w"], keys.data_ptr(), a["key_cap"],
                                               out.data_ptr(), nout.data_ptr(), a["n_images"], a["max_rows"], a["max_det"], a["thr"],
                                               a["agnostic"], stream())
        torch.cuda.synchronize()
        err = _lib.lib().kodhip_last_error().decode()
        assert rc < 0 and "fuse_detections" in err and msg in err, (kw, rc, err)
        assert int(nout) == -1 and bool((out == SENTINEL).all()) and bool((keys == 3).all()), kw


def test_fuse_short_key_cap_writes_nothing_beyond_it():
    """one image, 8 views x 300 rows under key_cap 1024: views 0 .. 2 fit, view 3 with its first 124 rows, the others not at
    all - the result is the reference's on those rows (W still sums all eight weights), the words behind key_cap stay"""
    case = fr.random_case("big")
    w = fr.case_weights(case, "mixed")
    cut = case.counts.copy()
    cut[3], cut[4:] = min(cut[3], 1024 - 900), 0
    assert case.counts[:4].min() > 124
    want = fr.fuse_ref(case.rows, cut, case.view_start, w, fr.THR, False, 300)
    got, intact = _fuse_direct(case, w, fr.THR, False, 300, key_cap=1024)
    assert intact, "keys were written behind key_cap"
    _same_rows(got, want, "short key_cap")


# ---------------------------------------------------------------------------------------------------- EnsembleDetector
CONF_K, IOU, FUSE = 40, 0.45, 0.55


@pytest.fixture(scope="module")
def nets():
    return H.network(5, 0.25), H.network(6, 0.5)


def _eager(net, x):
    with torch.no_grad():
        return get_detections(FeatureShape(width=x.shape[3], height=x.shape[2]), net(x), ANCH)


@pytest.fixture(scope="module")
def scene(nets):
    """(images, chunks, conf): conf leaves about CONF_K candidates of either network in its sparsest image"""
    imgs = H.images()
    for net in nets:
        net.fuse_eval(False)
    chunks = H.chunks(imgs)
    conf = min(H.conf_for(np.concatenate([_eager(net, x).cpu().numpy()[:n] for _, n, x, _ in chunks])) for net in nets)
    return imgs, chunks, conf


def _np(rows):
    return [r.clone().cpu().numpy() for r in rows]


@pytest.mark.parametrize("graphed", [False, True])
def test_ensemble_wbf_equals_the_composition(nets, scene, graphed):
    from object_detection_cib_amd.inference import EnsembleDetector
    imgs, chunks, conf = scene
    weights = [1.0, 0.5]
    d = EnsembleDetector(nets, ANCH, image_size=H.S, batch_size=H.BATCH, conf_thres=conf, iou_thres=IOU, graphed=graphed, merge="wbf",
                         weights=weights, fuse_thres=FUSE)
    modes = [[m.training for m in net.modules()] for net in nets]
    got = _np(d(imgs))
    assert [[m.training for m in net.modules()] for net in nets] == modes
    want, ref, per_member, infos = [], [], [], []
    for idx, n, x, lbs in chunks:
        outs = []
        for k, net in enumerate(nets):
            det = d.members[k]._geval[(H.BATCH, 3, H.S, H.S)](x).clone() if graphed else _eager(net, x)
            outs.append(non_max_suppression(det, conf, IOU, agnostic=False, multi_label=False, max_det=300, letterbox=lbs))
        rows = torch.stack([o.packed for o in outs], 1).reshape(H.BATCH * 2, 300, 6)
        counts = torch.stack([o.counts for o in outs], 1).reshape(-1)
        start, w = np.arange(H.BATCH + 1) * 2, np.tile(np.float32(weights), H.BATCH)
        want += _np(fuse_detections(rows, counts, start, w, thres=FUSE)[:n])
        r, c = rows.cpu().numpy(), counts.cpu().numpy()
        r[np.arange(300)[None, :] >= c[:, None]] = np.nan           # (rows beyond a count are uninitialised: never read)
        info = []
        ref += fr.fuse_ref(r, c, start, w, FUSE, info=info)[:n]
        infos += info[:n]
        per_member += c.reshape(H.BATCH, 2)[:n].tolist()
    print(f"FUSION ensemble graphed {graphed}: conf {conf:.6g}, rows per image and member {per_member}, fused {[len(w) for w in want]}, "
          f"clusters {[i['clusters'] for i in infos]} of candidates {[i['candidates'] for i in infos]}")
    assert len(got) == len(imgs) == 5 and min(min(p) for p in per_member) >= 1
    assert sum(i["candidates"] - i["clusters"] for i in infos) >= 1, "no box of one member joined a box of the other"
    _same_rows(want, ref, "the composition against the reference")
    _same_rows(got, want, f"ensemble wbf graphed {graphed}")
    for g, (h, w) in zip(got, H.SIZES):                                        # in the image's own pixels
        assert (g[:, :4] >= 0).all() and (g[:, [0, 2]] <= w).all() and (g[:, [1, 3]] <= h).all()
    if graphed:
        assert all(list(m._geval) == [(H.BATCH, 3, H.S, H.S)] for m in d.members)
        assert d.members[0]._geval is not d.members[1]._geval


def test_ensemble_nms_is_one_nms_over_all_rows(nets, scene):
    from object_detection_cib_amd.inference import EnsembleDetector
    imgs, chunks, conf = scene
    got = _np(EnsembleDetector(nets, ANCH, image_size=H.S, batch_size=H.BATCH, conf_thres=conf, iou_thres=IOU, merge="nms", max_det=50)(imgs))
    want = []
    for idx, n, x, lbs in chunks:
        det = torch.cat([_eager(net, x) for net in nets], dim=1)
        want += _np(non_max_suppression(det, conf, IOU, agnostic=False, multi_label=False, max_det=50, letterbox=lbs)[:n])
    print(f"FUSION ensemble nms: rows {[len(w) for w in want]}")
    assert min(len(w) for w in want) >= 1
    _same_rows(got, want, "ensemble nms")


@pytest.mark.parametrize("graphed", [False, True])
def test_ensemble_of_one_is_the_detector(nets, scene, graphed):
    from object_detection_cib_amd.inference import Detector, EnsembleDetector
    imgs, _, conf = scene
    kw = dict(image_size=H.S, batch_size=H.BATCH, conf_thres=conf, iou_thres=IOU, graphed=graphed)
    want = _np(Detector(nets[0], ANCH, **kw)(imgs))
    assert min(len(w) for w in want) >= 1
    for merge in ("wbf", "nms"):
        _same_rows(_np(EnsembleDetector([nets[0]], ANCH, merge=merge, **kw)(imgs)), want, f"one member {merge} graphed {graphed}")


def test_ensemble_of_twins_confirms_the_detector(nets):
    """[a, a] finds every box twice: the same counts, scores and classes bit for bit (st / n = (t + t) / 2 = t, min(2, 2) / 2
    = 1), boxes within 4 ulp (fl(fl(t * x) + fl(t * x)) / fl(t + t) = fl(fl(t * x) / t): two roundings)"""
    from object_detection_cib_amd.inference import Detector, EnsembleDetector
    # square images: in the letterbox padding of the others a kept box is clipped to nothing at the border, and a box without
    # area never matches its twin (the zero_area hand case) - that is the definition at work, not a difference to the detector
    imgs = H.images(H.SQUARE_SIZES, seed=4)
    nets[0].fuse_eval(False)
    conf = H.conf_for(np.concatenate([_eager(nets[0], x).cpu().numpy()[:n] for _, n, x, _ in H.chunks(imgs)]))
    kw = dict(image_size=H.S, batch_size=H.BATCH, conf_thres=conf, iou_thres=IOU)
    want = _np(Detector(nets[0], ANCH, **kw)(imgs))
    # the precondition, on the CPU: the detector's own rows have an area and do not fuse with each other
    for k, r in enumerate(want):
        assert ((r[:, 2] > r[:, 0]) & (r[:, 3] > r[:, 1])).all(), f"image {k}: a row without area"
        rows, counts = fr.pack_views([r], 300)
        alone, = fr.fuse_ref(rows, counts, [0, 1], None, FUSE)
        assert alone.tobytes() == r.tobytes(), f"image {k}: the detector's rows fuse with each other"
    got = _np(EnsembleDetector([nets[0], nets[0]], ANCH, merge="wbf", fuse_thres=FUSE, **kw)(imgs))
    counts = [len(w) for w in want]
    ulp = max((int(np.abs(_bits(g[:, :4]).astype(np.int64) - _bits(w[:, :4]).astype(np.int64)).max()) for g, w in zip(got, want) if len(w)
               and len(g) == len(w)), default=-1)
    print(f"FUSION twins: conf {conf:.6g}, rows {counts}, largest box difference {ulp} ulp")
    assert sum(counts) >= 5 and min(counts) >= 1
    assert [len(g) for g in got] == counts
    for g, w in zip(got, want):
        np.testing.assert_array_equal(_bits(g[:, 4:]), _bits(w[:, 4:]))
    assert 0 <= ulp <= 4


def test_ensemble_value_errors(nets):
    from object_detection_cib_amd.inference import EnsembleDetector
    a, b = nets
    for args, kw, msg in (([a, b], dict(merge="soft"), "merge"), ([a, b], dict(merge="nms", weights=[1, 1]), "weights"),
                          ([a, b], dict(weights=[1.0]), "weights"), ([a, b], dict(weights=[1.0, 0.0]), "weights"),
                          ([a, b], dict(weights=[1.0, float("nan")]), "weights"), ([a, b], dict(fuse_thres=0.3), "fuse_thres"),
                          ([a, b], dict(fuse_thres=1.5), "fuse_thres"), ([], {}, "nets"), ([a, b], dict(max_det=301), "max_det"),
                          ([a, b], dict(image_size=100), "image_size"), ([a] * 14, {}, "max_det")):
        with pytest.raises(ValueError, match=msg):
            EnsembleDetector(args, ANCH, **dict(dict(image_size=H.S), **kw))
    with pytest.raises(ValueError, match="anchor_info"):
        EnsembleDetector([a, b], [ANCH], image_size=H.S)
    EnsembleDetector([a, b], [ANCH, ANCH], image_size=H.S, fuse_thres=0.45)         # fuse_thres == iou_thres is allowed
    EnsembleDetector([a, b], ANCH, image_size=H.S, merge="nms", fuse_thres=0.1)     # merge "nms" does not fuse
    d = EnsembleDetector([a, b], ANCH, image_size=H.S, batch_size=H.BATCH)
    with pytest.raises(ValueError, match="image 1"):
        d([np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64), np.uint8)])
    assert d([]) == []
