"""CPU checks of the detection confusion matrix: the plain reference (tests/confusion_reference.py) gives the hand-evaluated
matrices, conserves ground truths and kept detections on every case, agrees with a second, dense-numpy formulation of the
rule, and its inputs reach the events they were built for; per-class precision / recall arithmetic; the C entry point's
argument checks (no launch, no GPU); the cross-rank sum under gloo."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import confusion_reference as R
from object_detection_cib_amd.lightning.callbacks.confusion import DeviceConfusionMatrix, per_class_from, reduce_counts

HAND = R.hand_cases()
RANDOM = R.random_cases()
ALL = {**HAND, **RANDOM}


def _run(case, events=None):
    return R.confusion_ref(case.dets, case.gts, case.nc, case.conf, case.iou, events)


@pytest.mark.parametrize("name", sorted(HAND))
def test_reference_gives_the_hand_matrices(name):
    case = HAND[name]
    np.testing.assert_array_equal(_run(case), R.expected_matrix(case))


def test_hand_cases_reach_their_events():
    ev = {n: {} for n in HAND}
    for n in HAND:
        _run(HAND[n], ev[n])
    assert ev["A_equal_iou_lower_gt"]["tie3"] == 1 and ev["A_equal_iou_lower_gt"]["offdiag"] == 1
    assert ev["B_equal_iou_lower_det"]["tie4"] == 1 and ev["B_equal_iou_lower_det"]["lost"] == 1
    assert ev["C_exact_thresholds"]["exact_thr"] == 1 and ev["C_exact_thresholds"]["exact_conf"] == 1
    assert ev["D_loser_not_rematched"]["lost"] == 1 and ev["D_loser_not_rematched"]["tie4"] == 0
    e = ev["E_300_ground_truths"]
    assert (e["matched"], e["bg_fp"], e["missed"], e["tie4"]) == (4, 4, 296, 4)
    assert len(HAND["E_300_ground_truths"].gts[0][1]) == 300


@pytest.mark.parametrize("name", sorted(RANDOM))
def test_random_scenes_reach_lost_and_off_diagonal_matches(name):
    case, ev = RANDOM[name], {}
    _run(case, ev)
    print(f"CONFUSION {name} nc {case.nc} events {ev}")
    assert len(case.dets) == 16
    assert ev["lost"] >= 5
    if case.nc > 1:
        assert ev["offdiag"] >= 3
    assert R.on_lattice(case, 8.0 if name == "lattice8" else 0.25)


def test_scenes_lie_on_both_sides_of_the_kernel_switch_over():
    from object_detection_cib_amd import _lib
    limit = _lib.lib().kodhip_confusion_lds_classes()
    assert R.SWITCH_NC[0] <= limit < R.SWITCH_NC[1]
    ncs = {c.nc for c in RANDOM.values()}
    assert {1, 5, 200, *R.SWITCH_NC} <= ncs


@pytest.mark.parametrize("name", sorted(ALL))
def test_reference_conserves_ground_truths_and_detections(name):
    case = ALL[name]
    assert R.on_lattice(case, 8.0 if name == "lattice8" else 0.25)
    M = _run(case)
    nc = case.nc
    labels = np.concatenate([l for _, l in case.gts]) if case.gts else np.zeros(0, np.int64)
    labels = labels[(labels >= 0) & (labels < nc)]
    np.testing.assert_array_equal(M[:, :nc].sum(0), np.bincount(labels, minlength=nc))
    kept = 0
    for d in case.dets:
        for row in d:
            c = R.det_class(row[5])
            kept += int(row[4] > np.float32(case.conf) and c is not None and 0 <= c < nc)
    assert M[:nc].sum() == kept
    assert M[nc, nc] == 0


def _dense(case):
    """The rule once more: dense IoU matrix, first-occurrence argmax per detection over its candidates, first-occurrence
    argmax per ground truth over the detections that chose it."""
    nc = case.nc
    M = np.zeros((nc + 1, nc + 1), np.int64)
    for d, (g, l) in zip(case.dets, case.gts):
        d = np.asarray(d, dtype=np.float32).reshape(-1, 6)
        g = np.asarray(g, dtype=np.float64).reshape(-1, 4)
        l = np.asarray(l, dtype=np.int64)
        cls = np.trunc(d[:, 5]).astype(np.int64)
        dk = np.nonzero((d[:, 4] > np.float32(case.conf)) & (cls >= 0) & (cls < nc))[0]
        gk = np.nonzero((l >= 0) & (l < nc))[0]
        b, cls, g, l = d[dk, :4].astype(np.float64), cls[dk], g[gk], l[gk]
        w = np.clip(np.minimum(b[:, None, 2], g[None, :, 2]) - np.maximum(b[:, None, 0], g[None, :, 0]), 0, None)
        h = np.clip(np.minimum(b[:, None, 3], g[None, :, 3]) - np.maximum(b[:, None, 1], g[None, :, 1]), 0, None)
        inter = w * h
        ad, ag = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]), (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = inter / (ad[:, None] + ag[None, :] - inter)
        cand = np.where(iou > case.iou, iou, -1.0)                     # (NaN > thr is False)
        choice = np.full(len(b), -1)
        if len(g) and len(b):
            first = np.argmax(cand, axis=1)
            has = cand[np.arange(len(b)), first] > 0
            choice[has] = first[has]
        taken = np.zeros(len(b), bool)
        for j in range(len(g)):
            col = np.where(choice == j, cand[:, j] if len(b) else np.zeros(0), -1.0)
            if len(b) and col.max() > 0:
                i = int(np.argmax(col))
                taken[i] = True
                M[cls[i], l[j]] += 1
            else:
                M[nc, l[j]] += 1
        np.add.at(M, (cls[~taken], np.full(int((~taken).sum()), nc)), 1)
    return M


@pytest.mark.parametrize("name", sorted(ALL))
def test_reference_equals_dense_formulation(name):
    np.testing.assert_array_equal(_run(ALL[name]), _dense(ALL[name]))


def test_evaluator_cases_cover_empty_sides():
    batches = R.evaluator_cases()
    assert len(batches) >= 5
    assert any(all(len(d) == 0 for d in dets) and sum(len(l) for _, l in gts) > 0 for dets, gts in batches)
    assert any(sum(len(l) for _, l in gts) == 0 and sum(len(d) for d in dets) > 0 for dets, gts in batches)
    ev = {}
    for dets, gts in batches[:3]:
        R.confusion_ref(dets, gts, 5, events=ev)
    assert ev["matched"] > 0 and ev["bg_fp"] > 0 and ev["missed"] > 0


def test_per_class_arithmetic_and_nan():
    #            true 0  1  2  bg
    m = np.array([[6, 1, 0, 3],      # predicted 0: precision 6 / 10
                  [2, 0, 0, 0],      # predicted 1: precision 0 / 2, recall 0 / 4 -> f1 NaN (0 / 0)
                  [0, 0, 0, 0],      # predicted 2: never predicted -> precision NaN; no ground truth -> recall NaN
                  [0, 3, 0, 0]], np.int64)
    pc = per_class_from(m)
    np.testing.assert_array_equal(pc["precision"][:2], [0.6, 0.0])
    np.testing.assert_array_equal(pc["recall"][:2], [0.75, 0.0])
    assert pc["f1"][0] == 2 * 0.6 * 0.75 / (0.6 + 0.75)
    assert np.isnan(pc["f1"][1]) and np.isnan(pc["precision"][2]) and np.isnan(pc["recall"][2]) and np.isnan(pc["f1"][2])
    np.testing.assert_array_equal(pc["missed"], [0, 3, 0])
    np.testing.assert_array_equal(pc["background_fp"], [3, 0, 0])
    assert all(len(pc[k]) == 3 for k in pc)
    cm = DeviceConfusionMatrix(3, ["a", "b", "c"])                     # nothing added: zeros, no device needed
    assert cm.names == ["a", "b", "c"] and (cm.conf_thres, cm.iou_thres) == (0.25, 0.45)
    assert cm.matrix().shape == (4, 4) and cm.matrix().dtype == np.int64 and not cm.matrix().any()
    assert np.isnan(cm.per_class()["precision"]).all()
    cm.reset()


def test_entry_point_refuses_bad_arguments_before_any_launch():
    from object_detection_cib_amd import _lib
    h = _lib.lib()
    assert h.kodhip_version() >= 102
    assert h.kodhip_confusion_max_det() >= 1024
    p = 4096                                                       # (a non-null address; a refused call never reads it)
    ok = dict(det=p, ndet=p, gt=None, lab=None, start=p, matrix=p, B=1, max_det=8, nc=3)

    def call(**kw):
        a = {**ok, **kw}
        return h.kodhip_confusion_match(a["det"], a["ndet"], a["gt"], a["lab"], a["start"], a["matrix"], a["B"], a["max_det"],
                                        a["nc"], 0.25, 0.45, None)
    for bad in (dict(det=None), dict(ndet=None), dict(start=None), dict(matrix=None), dict(nc=0), dict(B=0), dict(max_det=0),
                dict(nc=-1), dict(max_det=h.kodhip_confusion_max_det() + 1)):
        assert h.kodhip_nms(None, None, 0, None, None, None, 0, 0, 0, 0.0, 0.0, 0, 0, 0.0, None) < 0      # another error text in between
        assert b"confusion_match" not in h.kodhip_last_error()
        assert call(**bad) < 0, bad
        assert b"confusion_match" in h.kodhip_last_error(), (bad, h.kodhip_last_error())


def _sum_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        mine = torch.arange(16, dtype=torch.int64) * (rank + 1) + rank
        before = mine.clone()
        got = reduce_counts(mine, dist.group.WORLD)
        want = sum(torch.arange(16, dtype=torch.int64) * (r + 1) + r for r in range(world))
        ok = torch.equal(got, want) and got.dtype == torch.int64 and torch.equal(mine, before)
        ok = ok and torch.equal(reduce_counts(mine, None), mine)                 # no group: no collective
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_counts_are_summed_over_ranks_world2_gloo():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sum_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
    assert res == [(0, True), (1, True)]
