"""CPU checks of the auto-anchor feature: the numpy reference of tests/autoanchor_reference.py on hand cases with
closed-form answers, the mutation table, the host helpers of core/anchors/autoanchor.py and the argument validation of the
kodhip_anchor_* entry points (which happens before any launch, so it needs no GPU)."""
import ctypes as C
import math
import warnings

import numpy as np
import pytest

import autoanchor_reference as R
from object_detection_cib_amd.core.anchors import autoanchor as A
from object_detection_cib_amd.core.anchors.info import AnchorBoxInfo, voc_anchor_info
from object_detection_cib_amd.core.types import FeatureShape

T4 = R.threshold(4.0)


def test_threshold_box_does_not_count():
    wh = np.array([[10, 10], [40, 40], [10, 50]], dtype=np.float32)
    x = R.per_box(wh, [[10, 10]])
    assert x.dtype == np.float32 and x.ravel().tolist() == [1.0, 0.25, np.float32(0.2)]
    f, rec, pairs = R.metric(wh, [[10, 10]], T4)
    assert (f / 3, rec / 3, pairs / 3) == (1 / 3, 1 / 3, 1 / 3)


def test_anchor_equal_to_a_box_and_pair_counts():
    wh = np.array([[33, 23], [16, 30], [300, 300]], dtype=np.float32)
    k = np.array([[33, 23], [16, 30]], dtype=np.float32)
    x = R.per_box(wh, k)
    assert x[0, 0] == 1.0 and x[1, 1] == 1.0
    f, rec, pairs = R.metric(wh, k, T4)
    # box 0 is also within 4x of anchor 1 (16/33 = 0.48), box 1 of anchor 0 (16/33); box 2 is 9x away from both
    assert rec == 2 and pairs == 4 and f == 2.0
    # w = 4 kw, h = kh: exactly at the threshold on one side
    assert R.metric(np.array([[132, 23]], dtype=np.float32), k[:1], T4) == (0.0, 0, 0)
    assert R.metric(np.array([[131, 23]], dtype=np.float32), k[:1], T4)[1:] == (1, 1)


def test_two_pixel_filter_keeps_a_box_with_one_long_side():
    wh = np.array([[1.5, 1.9], [1.0, 30.0], [2.0, 1.0], [5.0, 5.0], [1.99, 1.99]], dtype=np.float32)
    want = wh[[1, 2, 3]]
    assert np.array_equal(R.filter_wh(wh), want) and np.array_equal(A.filter_wh(wh), want)


def test_lloyd_step_empty_cluster_and_tie():
    pts = np.array([[0, 0], [2, 0], [0, 2], [10, 10]], dtype=np.float32)
    # restart 0: centroid 2 is far from everything and stays; restart 1: [1, 0] is equidistant from centroids 0 and 1
    cent = np.array([[[0, 0], [10, 10], [100, 100]],
                     [[0, 0], [2, 0], [10, 10]]], dtype=np.float32)
    pts = np.concatenate([pts, np.array([[1, 0]], dtype=np.float32)])
    new, labels, counts, dist, _ = R.lloyd_step(pts, cent)
    assert labels[0].tolist() == [0, 0, 0, 1, 0] and counts[0].tolist() == [4, 1, 0]
    assert new[0, 2].tolist() == [100, 100]                              # the empty cluster keeps its centroid
    assert new[0, 0].tolist() == [0.75, 0.5] and new[0, 1].tolist() == [10, 10]
    assert dist[0] == 0 + 4 + 4 + 0 + 1
    assert labels[1].tolist() == [0, 1, 0, 2, 0]                         # the tie of [1, 0] goes to the lower index
    assert counts[1].tolist() == [3, 1, 1] and dist[1] == 0 + 0 + 4 + 0 + 1
    assert new.dtype == np.float32 and np.allclose(new[1, 0], [1 / 3, 2 / 3])


def test_candidates_multiply_then_clip():
    k = np.array([[3, 100]], dtype=np.float32)
    v = np.array([[[0.3, 3.0]], [[1.0, 0.5]]], dtype=np.float32)
    c = R.candidates(k, v)
    assert c.dtype == np.float32 and c.tolist() == [[[2.0, 300.0]], [[3.0, 50.0]]]


def test_mutation_table():
    a = A.mutation_table(np.random.default_rng(7), 50, 4, 9)
    b = A.mutation_table(np.random.default_rng(7), 50, 4, 9)
    r = R.mutation_table(np.random.default_rng(7), 50, 4, 9)
    assert a.dtype == np.float32 and a.shape == (50, 4, 9, 2)
    assert np.array_equal(a, b) and np.array_equal(a, r)                 # same seed, same table; the reference's restatement agrees
    assert a.min() >= np.float32(0.3) and a.max() <= np.float32(3.0)
    assert not (a == 1).all(axis=(2, 3)).any()                           # no candidate that changes nothing
    assert (a == 1).any() and not np.array_equal(a, A.mutation_table(np.random.default_rng(8), 50, 4, 9))


@pytest.mark.parametrize("shape", R.EVOLVE_SHAPES)
def test_evolution_cases_are_decidable(shape):
    """The GPU test compares decisions entry for entry: every decision of the reference run must be further from a tie
    than a reordered fp64 sum can move it, and both branches (accepted / rejected) must occur."""
    c = R.evolve_case(shape)
    print("smallest gap", c["gap"], "accepted", sum(a for _, a, _ in c["trace"]), "of", shape[1])
    assert c["gap"] > 1e-9
    acc = [a for _, a, _ in c["trace"]]
    assert 0 < sum(acc) < len(acc)
    assert c["f"] >= c["f0"]
    assert c["gap"] > 100 * shape[0] * 2.0 ** -52 * c["f"]                # two orders above the reordering bound


def test_evolve_reference_rejects_equal_and_prefers_lower_index():
    wh = np.array([[10, 10], [20, 20]], dtype=np.float32)
    k = np.array([[10, 10]], dtype=np.float32)
    f0 = R.metric(wh, k, T4)[0]
    ones = np.ones((1, 2, 1, 2), dtype=np.float32)                       # both candidates equal the current anchors
    k1, f1, trace, gap = R.evolve(wh, k, f0, ones, T4)
    assert trace == [(0, 0, f0)] and f1 == f0 and np.array_equal(k1, k) and gap == 0.0


# ---- host helpers -----------------------------------------------------------------------------------------------------

def test_label_wh_scales_by_the_longer_side():
    boxes = [np.array([[10, 20, 110, 70], [0, 0, 50, 25]], dtype=np.float64), np.zeros((0, 4)), np.array([[5, 5, 25, 45]])]
    shapes = [(500, 1000), (300, 300), (320, 160)]
    wh = A.label_wh(boxes, shapes, 640)
    assert wh.dtype == np.float32 and wh.shape == (3, 2)
    assert np.array_equal(wh, np.array([[64, 32], [32, 16], [40, 80]], dtype=np.float32))
    with pytest.raises(ValueError):
        A.label_wh(boxes, shapes[:2], 640)
    assert A.label_wh([], [], 640).shape == (0, 2)


def test_dataset_label_wh():
    from datetime import datetime
    from object_detection_cib_amd.data.cache import DatasetInfo, ImageMetadata, SampleInfo, TargetInfo
    s = [SampleInfo("a", "a.jpg", ImageMetadata(1000, 500, 3, "image/jpeg", 1), [TargetInfo((10, 20, 110, 70), "x")]),
         SampleInfo("b", "b.jpg", ImageMetadata(160, 320, 3, "image/jpeg", 1), [TargetInfo((5, 5, 25, 45), "y")]),
         SampleInfo("c", "c.jpg", ImageMetadata(100, 100, 3, "image/jpeg", 1), [])]
    wh = A.dataset_label_wh(DatasetInfo("d", datetime(2020, 1, 1), ["x", "y"], s), 640)
    assert np.array_equal(wh, np.array([[64, 32], [40, 80]], dtype=np.float32))


def _voc():
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo
    return LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))


def test_split_levels_by_area():
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo
    voc = A.anchors_array(_voc())
    assert voc.shape == (9, 2) and voc[0].tolist() == [10, 13] and voc[8].tolist() == [373, 326]
    info = A.split_levels(voc[::-1] + np.float32(0.5), [8, 16, 32])
    assert isinstance(info, LayerwiseAnchorInfo) and [lv.stride for lv in info] == [8, 16, 32]
    # (62, 45) has a smaller area than (30, 61)?  62.5 * 45.5 = 2843.75 > 30.5 * 61.5 = 1875.75: order as in the VOC table
    assert [(b.width, b.height) for b in info.ml.boxes_wh] == [(30.5, 61.5), (62.5, 45.5), (59.5, 119.5)]
    assert [(b.width, b.height) for b in info.ll.boxes_wh] == [(10.5, 13.5), (16.5, 30.5), (33.5, 23.5)]
    assert all(type(v) is float for lv in info for b in lv.boxes_wh for v in b)
    with pytest.raises(ValueError):
        A.split_levels(voc[:8], [8, 16, 32])
    assert len(A.split_levels(voc[:6], [8, 16])) == 2


def test_anchor_info_yaml_layout():
    texts = A.anchor_info_yaml(_voc())
    assert len(texts) == 3
    assert texts[0] == ("_target_: kod.core.anchors.info.AnchorBoxInfo\nstride: 8\nboxes_wh:\n"
                        "  - _target_: kod.core.types.FeatureShape\n    width: 10\n    height: 13\n"
                        "  - _target_: kod.core.types.FeatureShape\n    width: 16\n    height: 30\n"
                        "  - _target_: kod.core.types.FeatureShape\n    width: 33\n    height: 23\n")
    assert "stride: 32" in texts[2] and "width: 373" in texts[2]
    frac = A.anchor_info_yaml([AnchorBoxInfo(4, [FeatureShape(width=2.504, height=7.25)])])[0]
    assert "width: 2.5\n" in frac and "height: 7.25\n" in frac


def test_device_functions_need_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="MI355X|GPU"):
        A.anchor_metrics(np.ones((4, 2), dtype=np.float32) * 10, _voc())
    with pytest.raises(RuntimeError, match="MI355X|GPU"):
        A.kmean_anchors(np.ones((40, 2), dtype=np.float32) * 10)


# ---- argument validation through the built library ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def h():
    from object_detection_cib_amd import _lib, build
    build.build(verbose=False)
    return _lib.lib()


def test_limits_and_sizes(h):
    assert h.kodhip_version() >= 105
    assert h.kodhip_anchor_max_anchors() >= 12 and h.kodhip_anchor_max_population() >= 16 and h.kodhip_anchor_max_restarts() >= 30
    assert h.kodhip_anchor_trace_bytes() == 16
    block, cap = h.kodhip_anchor_block_size(), h.kodhip_anchor_grid_cap()
    assert block % 64 == 0 and cap >= 1
    assert h.kodhip_anchor_workspace_bytes(0, 1) == 0 and h.kodhip_anchor_workspace_bytes(10, 0) == 0
    one = h.kodhip_anchor_workspace_bytes(1, 1)
    # a slab row per set and (anchor + 1), a slot per block, 24 bytes per slot; beyond the cap the grid no longer grows
    assert one >= (h.kodhip_anchor_max_anchors() + 1) * 24
    assert h.kodhip_anchor_workspace_bytes(block + 1, 1) > one
    assert h.kodhip_anchor_workspace_bytes(block * cap * 3, 2) == h.kodhip_anchor_workspace_bytes(block * cap, 2)
    assert h.kodhip_anchor_workspace_bytes(block * cap, 64) >= 64 * (h.kodhip_anchor_max_anchors() + 1) * cap * 24


def test_argument_validation_without_a_gpu(h):
    buf = (C.c_double * 64)()                     # host memory: never dereferenced, validation comes before any launch
    p = C.addressof(buf)
    err = lambda: h.kodhip_last_error()           # noqa: E731
    nmax, pmax, rmax = h.kodhip_anchor_max_anchors(), h.kodhip_anchor_max_population(), h.kodhip_anchor_max_restarts()

    def metric(wh=p, N=10, k=p, P=1, n=9, t=0.25, ws=p, f=p, r=p, c=p):
        return h.kodhip_anchor_metric(wh, N, k, P, n, t, ws, f, r, c, None)
    for kw in (dict(wh=None), dict(k=None), dict(ws=None), dict(f=None), dict(r=None), dict(c=None)):
        assert metric(**kw) < 0 and b"anchor_metric" in err() and b"null" in err(), kw
    for kw in (dict(N=0), dict(N=-5), dict(n=0), dict(n=nmax + 1), dict(P=0), dict(P=pmax + 1), dict(t=math.nan), dict(t=math.inf),
               dict(wh=p + 4)):
        assert metric(**kw) < 0 and b"anchor_metric" in err(), kw
    assert metric(n=nmax + 1) < 0 and str(nmax).encode() in err()

    def evolve(wh=p, N=10, k=p, fit=p, v=p, gen=2, P=1, n=9, t=0.25, tr=p, ws=p):
        return h.kodhip_anchor_evolve(wh, N, k, fit, v, gen, P, n, t, tr, ws, None)
    for kw in (dict(wh=None), dict(k=None), dict(fit=None), dict(v=None), dict(tr=None), dict(ws=None), dict(N=0), dict(gen=-1),
               dict(n=0), dict(n=nmax + 1), dict(P=0), dict(P=pmax + 1), dict(t=math.nan), dict(t=-math.inf)):
        assert evolve(**kw) < 0 and b"anchor_evolve" in err(), kw
    assert evolve(gen=0, v=None, tr=None) == 0                           # nothing to enqueue

    def kmeans(pts=p, N=10, c=p, R=2, n=3, ws=p, d=p, cnt=p, lab=None):
        return h.kodhip_anchor_kmeans_step(pts, N, c, R, n, ws, d, cnt, lab, None)
    for kw in (dict(pts=None), dict(c=None), dict(ws=None), dict(d=None), dict(cnt=None), dict(N=0), dict(R=0), dict(R=rmax + 1),
               dict(n=0), dict(n=nmax + 1)):
        assert kmeans(**kw) < 0 and b"anchor_kmeans_step" in err(), kw


def test_python_limits_are_checked_before_the_device():
    with pytest.raises(ValueError, match="three anchors per level"):
        A.check_anchors(np.ones((4, 2), dtype=np.float32), [AnchorBoxInfo(8, [FeatureShape(1, 1)] * 2)])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError):
            A.anchors_array(np.zeros((3, 3)))
