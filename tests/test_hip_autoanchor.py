"""csrc/anchors.hip (kodhip_anchor_metric / _evolve / _kmeans_step) and core/anchors/autoanchor.py against the numpy
reference of tests/autoanchor_reference.py.

Tolerances are derived, not measured.  Per-box values are the same fp32 operations on both sides, so counts, labels,
decisions and evolved anchors are compared exactly.  A sum of N fp64 terms of one sign, added in another order, moves by at
most N * 2^-52 relative: that is the bound on fitness sums and distortions.  A centroid is float32(fp64 sum / count): two
fp64 quotients that close round to the same or to neighbouring float32 values, hence 1 ulp.  Workspaces are poisoned with
0xFF bytes (NaN / huge integers), so a slot read before it is written shows."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import autoanchor_reference as R  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.anchors import autoanchor as A  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402

EPS = 2.0 ** -52
T4 = float(R.threshold(4.0))
TRACE = np.dtype([("winner", "<i4"), ("accepted", "<i4"), ("fitness", "<f8")])


def _lim():
    h = _lib.lib()
    return h.kodhip_anchor_max_anchors(), h.kodhip_anchor_max_population(), h.kodhip_anchor_max_restarts()


def _big_n():
    h = _lib.lib()
    return h.kodhip_anchor_grid_cap() * h.kodhip_anchor_block_size() + 3


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ws(N, sets):
    return torch.full((_lib.lib().kodhip_anchor_workspace_bytes(N, sets),), 0xFF, dtype=torch.uint8, device="cuda")


def _metric(wh, k):
    """k [P, n, 2] -> host (fitness_sum [P], n_recalled [P], n_pairs [P])"""
    P, n, _ = k.shape
    d_wh, d_k, ws = _dev(wh), _dev(k), _ws(len(wh), P)
    f = torch.full((P,), float("nan"), dtype=torch.float64, device="cuda")
    r = torch.full((P,), -1, dtype=torch.int64, device="cuda")
    c = torch.full((P,), -1, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().kodhip_anchor_metric(d_wh.data_ptr(), len(wh), d_k.data_ptr(), P, n, T4, ws.data_ptr(), f.data_ptr(),
                                               r.data_ptr(), c.data_ptr(), stream()), "anchor_metric")
    torch.cuda.synchronize()
    return f.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy()


def _metric_cases():
    nmax, pmax, _ = 32, 64, 64                     # asserted against the library in the test
    cases = [(N, 9, 8) for N in (1, 63, 64, 65, 257)]
    cases += [(1000, n, P) for n in (1, 9, 12, nmax) for P in (1, 8, pmax)]
    cases += [("big", 9, 1), ("big", 12, 8)]
    return cases


def _metric_inputs(N, n, P):
    rng = np.random.default_rng(7 * N + 31 * n + P)
    wh = R.lognormal_wh(rng, N)
    k = R.lognormal_wh(rng, P * n).reshape(P, n, 2)
    wh[0] = (4 * k[0, 0, 0], k[0, 0, 1])           # exactly at the threshold of set 0's first anchor: w = 4 kw, h = kh
    if N > 2:
        wh[1] = k[0, 0]                            # exactly on an anchor
        wh[2] = (k[0, n - 1, 0], 4 * k[0, n - 1, 1])
    return wh, k


@pytest.mark.parametrize("N,n,P", _metric_cases())
def test_metric_matches_reference(N, n, P):
    nmax, pmax, _ = _lim()
    assert (nmax, pmax) == (32, 64)
    if N == "big":
        N = _big_n()                               # one more than grid cap x block: the grid-stride path
    wh, k = _metric_inputs(N, n, P)
    f, r, c = _metric(wh, k)
    f2, r2, c2 = _metric(wh, k)
    assert f.tobytes() == f2.tobytes() and np.array_equal(r, r2) and np.array_equal(c, c2)      # run to run: the same bits
    for p in range(P):
        wf, wr, wc = R.metric(wh, k[p], T4)
        print(f"N {N} n {n} P {P} set {p}: fitness {f[p]!r} ref {wf!r} rel {abs(f[p] - wf) / max(wf, 1e-300):.3e} bound {N * EPS:.3e}")
        assert r[p] == wr and c[p] == wc, (p, r[p], wr, c[p], wc)
        assert abs(f[p] - wf) <= N * EPS * wf, (p, f[p], wf)
    if N > 2 and n == 1:
        # with a single anchor the threshold box is recalled by nobody
        assert R.per_box(wh[:1], k[0])[0, 0] == np.float32(0.25)


def test_metric_threshold_and_exact_hit_by_hand():
    wh = np.array([[10, 10], [40, 40], [10, 50]], dtype=np.float32)
    f, r, c = _metric(wh, np.array([[[10, 10]]], dtype=np.float32))
    assert (f[0], r[0], c[0]) == (1.0, 1, 1)
    m = A.anchor_metrics(wh, np.array([[10, 10]], dtype=np.float32))
    assert m == A.AnchorMetrics(bpr=1 / 3, aat=1 / 3, fitness=1 / 3, n=3)


@pytest.mark.parametrize("shape", R.EVOLVE_SHAPES)
def test_evolution_matches_reference(shape):
    N, gen, P, n = shape
    c = R.evolve_case(shape)
    assert c["gap"] > 1e-9                          # the reference's decisions are not at the mercy of the summation order
    acc_ref = sum(a for _, a, _ in c["trace"])
    assert 0 < acc_ref < gen
    h = _lib.lib()
    assert h.kodhip_anchor_trace_bytes() == TRACE.itemsize
    d_wh, d_k, d_v = _dev(c["wh"]), _dev(c["k0"]), _dev(c["table"])
    d_f = torch.tensor([c["f0"]], dtype=torch.float64, device="cuda")
    d_tr = torch.full((gen * TRACE.itemsize,), 0xFF, dtype=torch.uint8, device="cuda")
    ws = _ws(N, P)
    _lib.check(h.kodhip_anchor_evolve(d_wh.data_ptr(), N, d_k.data_ptr(), d_f.data_ptr(), d_v.data_ptr(), gen, P, n, float(c["t"]),
                                      d_tr.data_ptr(), ws.data_ptr(), stream()), "anchor_evolve")
    torch.cuda.synchronize()
    tr = d_tr.cpu().numpy().view(TRACE)
    want = c["trace"]
    worst = max(abs(tr["fitness"][g] - want[g][2]) / want[g][2] for g in range(gen))
    print(f"{shape}: gap {c['gap']:.3e}, accepted {acc_ref}/{gen}, worst trace fitness rel {worst:.3e} bound {N * EPS:.3e}")
    assert tr["winner"].tolist() == [w for w, _, _ in want]
    assert tr["accepted"].tolist() == [a for _, a, _ in want]
    assert worst <= N * EPS
    k = d_k.cpu().numpy()
    assert k.tobytes() == c["k"].tobytes()
    f = float(d_f.cpu()[0])
    assert f >= c["f0"] and abs(f - c["f"]) <= N * EPS * c["f"]
    assert f == max([c["f0"]] + [float(x) for x, a in zip(tr["fitness"], tr["accepted"]) if a])


def _kmeans_inputs(R_, n, N):
    rng = np.random.default_rng(100 * R_ + 10 * n + N)
    wh = R.lognormal_wh(rng, N)
    pts = (wh / wh.std(0)).astype(np.float32)
    pts[0] = (1.0, 1.0)
    pts[5:10] = pts[10:15]                          # duplicate points
    cent = np.stack([pts[rng.choice(N, n, replace=False)] for _ in range(R_)])
    cent[0, 0], cent[0, 1] = (1.25, 1.0), (0.75, 1.0)      # equidistant from pts[0]: 0.0625 each, exact in fp32
    cent[R_ - 1, n - 1] = (1000.0, 1000.0)          # nobody's nearest centroid: stays empty, stays put
    return pts, np.ascontiguousarray(cent, dtype=np.float32)


@pytest.mark.parametrize("R_", [1, 30])
@pytest.mark.parametrize("n", [3, 9])
@pytest.mark.parametrize("N", [65, 1000])
def test_kmeans_step_teacher_forced(R_, n, N):
    pts, cent = _kmeans_inputs(R_, n, N)
    h = _lib.lib()
    d_pts, d_c, ws = _dev(pts), _dev(cent), _ws(N, R_)
    d_dist = torch.full((R_,), float("nan"), dtype=torch.float64, device="cuda")
    d_cnt = torch.full((R_, n), -1, dtype=torch.int64, device="cuda")
    d_lab = torch.full((R_, N), -1, dtype=torch.int32, device="cuda")
    saw_tie = saw_empty = False
    for step in range(10):
        before = d_c.cpu().numpy()
        _lib.check(h.kodhip_anchor_kmeans_step(d_pts.data_ptr(), N, d_c.data_ptr(), R_, n, ws.data_ptr(), d_dist.data_ptr(),
                                               d_cnt.data_ptr(), d_lab.data_ptr(), stream()), "anchor_kmeans_step")
        torch.cuda.synchronize()
        new, labels, counts, dist, _ = R.lloyd_step(pts, before)
        got = d_c.cpu().numpy()
        assert np.array_equal(d_lab.cpu().numpy(), labels), step
        assert np.array_equal(d_cnt.cpu().numpy(), counts), step
        ulp = np.abs(got.view(np.int32).astype(np.int64) - new.view(np.int32).astype(np.int64)).max()
        rel = np.abs(d_dist.cpu().numpy() - dist) / dist
        print(f"R {R_} n {n} N {N} step {step}: centroid ulp {ulp}, distortion rel {rel.max():.3e} bound {N * EPS:.3e}")
        assert ulp <= 1, step
        assert (rel <= N * EPS).all(), step
        if step == 0:
            d0 = (pts[0, 0] - before[0, :, 0]) ** 2 + (pts[0, 1] - before[0, :, 1]) ** 2
            saw_tie = d0[0] == d0[1] == d0.min() and labels[0, 0] == 0
        empty = counts == 0
        saw_empty |= bool(empty.any())
        assert np.array_equal(got[empty], before[empty])                  # an empty cluster keeps its centroid
    assert saw_tie and saw_empty
    # no labels wanted: the same centroids
    d_c2 = _dev(before)
    _lib.check(h.kodhip_anchor_kmeans_step(d_pts.data_ptr(), N, d_c2.data_ptr(), R_, n, ws.data_ptr(), d_dist.data_ptr(),
                                           d_cnt.data_ptr(), None, stream()), "anchor_kmeans_step")
    torch.cuda.synchronize()
    assert d_c2.cpu().numpy().tobytes() == got.tobytes()


# ---- end to end ---------------------------------------------------------------------------------------------------------

CENTRES = np.array([[w, h] for w in (30, 110, 200) for h in (50, 140, 260)], dtype=np.float32)
SPREAD = 1.5


def _cluster_wh():
    rng = np.random.default_rng(5)
    return np.concatenate([c + rng.uniform(-SPREAD, SPREAD, (200, 2)) for c in CENTRES]).astype(np.float32)


def _voc():
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo
    return LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))


def test_kmean_anchors_finds_separated_clusters():
    """Lloyd steps from n random points can stall with two centroids in one cluster; the best of 30 restarts is the true
    optimum for 7 of the seeds 0..11 on the numpy reference (seed 2 among them, seed 0 not): the seed is chosen there."""
    k = A.kmean_anchors(_cluster_wh(), n=9, gen=0, seed=2)
    assert k.dtype == np.float32 and k.shape == (9, 2)
    area = k.prod(1)
    assert (np.diff(area) >= 0).all()
    d = np.abs(k[:, None, :] - CENTRES[None]).max(2)           # [anchor, centre]
    assert (d.min(1) <= SPREAD).all(), k
    assert sorted(d.argmin(1).tolist()) == list(range(9)), k    # every centre found once


def test_evolution_does_not_lower_fitness_and_repeats():
    wh = R.lognormal_wh(np.random.default_rng(3), 2000)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        k0 = A.kmean_anchors(wh, n=9, gen=0, seed=1)
        k1 = A.kmean_anchors(wh, n=9, gen=100, population=16, seed=1)
        k2 = A.kmean_anchors(wh, n=9, gen=100, population=16, seed=1)
    whf = A.filter_wh(wh)
    m0, m1 = A.anchor_metrics(whf, k0), A.anchor_metrics(whf, k1)
    print("fitness gen=0", m0.fitness, "gen=100 x 16", m1.fitness, "bpr", m0.bpr, m1.bpr)
    assert m1.fitness >= m0.fitness
    assert k1.tobytes() == k2.tobytes()                         # same seed: the same anchors bit for bit
    assert (np.diff(k1.prod(1)) >= 0).all() and (k1 >= 2).all()


def test_check_anchors_keeps_anchors_that_fit():
    voc = _voc()
    rng = np.random.default_rng(11)
    wh = (np.repeat(A.anchors_array(voc), 100, axis=0) * rng.uniform(0.8, 1.25, (900, 2))).astype(np.float32)
    info, rep = A.check_anchors(wh, voc)
    assert rep.before.bpr > 0.98 and not rep.replaced and rep.after == rep.before
    assert info is voc


def test_check_anchors_refits_small_boxes():
    """Boxes more than 4 x narrower than every VOC anchor (the smallest is 10 x 13), as small as the 2 px filter of
    kmean_anchors allows: the assigner with the VOC anchors would take none of them."""
    from object_detection_cib_amd.core.label_assignment.yv5 import Yolov5LabelAssigner
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo
    voc = _voc()
    rng = np.random.default_rng(12)
    wh = np.stack([rng.uniform(2.0, 2.4, 600), rng.uniform(2.0, 3.2, 600)], 1).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                         # every box has a side under 3 px
        info, rep = A.check_anchors(wh, voc, gen=50, population=8, seed=2)
    assert rep.before.bpr == 0.0 and rep.before.aat == 0.0 and rep.before.fitness == 0.0 and rep.before.n == 600
    assert rep.replaced and rep.after.bpr > rep.before.bpr and rep.after.bpr > 0.98
    assert isinstance(info, LayerwiseAnchorInfo) and [lv.stride for lv in info] == [8, 16, 32]
    flat = [(b.width, b.height) for lv in info for b in lv.boxes_wh]
    assert len(flat) == 9 and all(type(v) is float and v >= 2.0 for wh_ in flat for v in wh_)
    assert [w * h_ for w, h_ in flat] == sorted(w * h_ for w, h_ in flat)
    assert A.anchor_metrics(wh, info) == rep.after
    Yolov5LabelAssigner(info)
    texts = A.anchor_info_yaml(info)
    assert len(texts) == 3 and texts[1].startswith("_target_: kod.core.anchors.info.AnchorBoxInfo\nstride: 16\n")
