"""The validation references (tests/val_reference.py) against the oracle on tie-free inputs - so that what the GPU tests
of decode, NMS and matching compare with is torch's / COCOeval's semantics, not a transcription of the kernels - and the
constructed cases on their own: every condition a case exists for holds in the reference.  Runs anywhere (no GPU)."""
import numpy as np
import pytest
import torch

from oracle import detection as D, map_eval as M, synth
from oracle.network import HeadOut, NetOut
import val_reference as V


def _decoded(size, nc, B, seed, scale):
    heads = synth.head_logits(B, size, nc, seed=seed, scale=scale)
    return D.decode(NetOut(*[HeadOut(*h) for h in heads]), size, size)


# --------------------------------------------------------------------------------------------------- references vs oracle
@pytest.mark.parametrize("size,nc,B,seed,scale", [(64, 10, 2, 21, 1.0), (96, 10, 1, 22, 3.0), (96, 1, 2, 23, 2.0), (96, 3, 1, 24, 2.0)])
@pytest.mark.parametrize("conf,thr", [(0.001, 0.6), (0.25, 0.45)])
def test_nms_ref_equals_oracle_on_tie_free_inputs(size, nc, B, seed, scale, conf, thr):
    det = _decoded(size, nc, B, seed, scale)
    keys = V.nms_keys_ref(det.numpy(), conf)
    for k, _ in keys:                                         # tie-free, and below the oracle's unstable top-30000 cut
        assert len(np.unique(k >> np.uint64(32))) == len(k) <= 30000
    assert sum(len(k) for k, _ in keys) > 0
    want = D.nms(det.clone(), conf, thr)
    got = V.nms_ref(det.numpy(), conf, thr)
    assert [len(g) for g in got] == [w.shape[0] for w in want]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w.numpy().reshape(-1, 6))


def test_nms_keys_are_the_documented_order():
    """sorted keys = (score descending, candidate index ascending), the candidate list itself in (row, class) order"""
    det, conf, _, _ = V.ties_case()
    nc = det.shape[2] - 5
    for x, (keys, order) in zip(det, V.nms_keys_ref(det, conf)):
        idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
        assert (np.diff(idx) > 0).all()
        score = (x[:, 5:] * x[:, 4:5]).reshape(-1)
        assert (score[idx] > np.float32(conf)).all() and len(idx) == int(((score.reshape(-1, nc) > np.float32(conf)) & (x[:, 4:5] > np.float32(conf))).sum())
        want = idx[np.lexsort((idx, -score[idx].astype(np.float64)))]
        np.testing.assert_array_equal((order & np.uint64(0xFFFFFFFF)).astype(np.int64), want)


@pytest.mark.parametrize("nc,seed", [(10, 0), (3, 1), (80, 2)])
def test_match_ref_equals_oracle_match_image(nc, seed):
    rng = np.random.default_rng(seed)
    dets, gts = V.random_scene(rng, nc, 8)
    det, nd, gt, lab, start = V._pack(dets, gts)
    tp, counted = V.match_ref(det, nd, gt, lab, start, nc, M.IOUS, M.MAX_DETS)
    mine = V.per_image_records(det, nd, tp, counted, lab, start, nc)
    want = [M.match_image(d, g, l, nc) for d, (g, l) in zip(dets, gts)]
    for a, b in zip(mine, want):
        for (s1, m1, n1), (s2, m2, n2) in zip(a, b):
            np.testing.assert_array_equal(s1, s2)
            np.testing.assert_array_equal(m1, m2)
            assert n1 == n2
    np.testing.assert_array_equal(M.accumulate(mine, nc), M.accumulate(want, nc))
    assert tp.sum() > 0 and (counted.sum(1) <= nd).all()


@pytest.mark.parametrize("name", list(V.decode_cases()))
def test_decode_ref_vs_fp32_oracle_within_half_the_device_tolerance(name):
    w, h, nc, B, seed = V.decode_cases()[name]
    case = V.decode_case(w, h, nc, B, seed)
    ref = V.decode_ref(case.raws, V.STRIDES, V.ANCHORS, w, h)
    got = V.oracle_decode(case)
    assert got.shape == ref.shape == (B, case.facts["rows"], 5 + nc)
    box, rel, missed = V.decode_errors(got, ref)
    print(f"VALREF decode {name} oracle box {box:.3f} ulp32, score {rel:.4e} rel, exact misses {missed}")
    assert box <= V.DECODE_BOX_ULP / 2 and rel <= V.DECODE_SCORE_REL / 2 and missed == 0
    assert V.DECODE_BOX_ULP == 2 * V.DECODE_BOX_ULP_MEASURED and V.DECODE_SCORE_REL == 2 * V.DECODE_SCORE_REL_MEASURED
    f = case.facts
    assert f["rectangular"] and f["finite"] and f["min_specials_per_field_value"] >= 1
    assert f["planted"] == 3 * (5 + nc) * len(V.SPECIAL_LOGITS)
    assert f["exact_zero"] >= 3 * (1 + nc) and f["exact_one"] >= 3 * 3 * (1 + nc) and f["subnormal"] >= 3 * (1 + nc)
    assert len(set(f["level_rows"])) == 3 and sum(f["level_rows"]) == f["rows"]


def test_decode_ref_row_order_on_a_rectangular_grid():
    """one hot cell per level: the row index is ((anchor * h) + y) * w + x behind the level's first row"""
    w, h, nc = 160, 96, 2
    raws = [torch.zeros(1, 3, h // s, w // s, 5 + nc) for s in V.STRIDES]
    where = [(2, 7, 3), (1, 0, 9), (0, 2, 4)]                      # (anchor, y, x), x beyond the grid's height on level 1
    for r, (a, y, x) in zip(raws, where):
        r[0, a, y, x, 4] = 9.0
    ref = V.decode_ref(raws, V.STRIDES, V.ANCHORS, w, h)
    hot = (ref[0, :, 4] > 0.9).nonzero().reshape(-1).tolist()
    row0, want = 0, []
    for (a, y, x), s in zip(where, V.STRIDES):
        gh, gw = h // s, w // s
        want.append(row0 + (a * gh + y) * gw + x)
        row0 += 3 * gh * gw
    assert hot == want
    for r_, (a, y, x), s in zip(hot, where, V.STRIDES):            # zero logits: the box is centred on its cell
        b = ref[0, r_, :4]
        assert float((b[0] + b[2]) / 2) == (x + 0.5) * s and float((b[1] + b[3]) / 2) == (y + 0.5) * s
        assert float(b[2] - b[0]) == V.ANCHORS[V.STRIDES.index(s)][a][0]


# ------------------------------------------------------------------------------------------------ the builders' conditions
def test_sort_reach_counts_are_met_exactly():
    det, conf, thr, f = V.sort_reach_case()
    assert det.shape == (10, 1200, 13)
    assert tuple(f["counts"]) == V.SORT_COUNTS == (0, 1, 63, 64, 65, 4095, 4096, 4097, 8193, 9600)
    assert f["obj_passes_score_fails"] > 0
    assert all(n > 0 for n in f["rows_used_beyond_1024"][5:])       # the scan carry into the second 1024-row iteration


def test_cluster_case_walk_depth_and_survivor_counts():
    _, _, _, f = V.cluster_case()
    print("VALREF cluster", f)
    assert any(4096 < r <= 8192 for r in f["last_rank"]) and any(r > 8192 for r in f["last_rank"])
    assert any(c and s < 300 for c, s in zip(f["consumed_all"], f["survivors"]))
    assert any(s == 300 and not c for c, s in zip(f["consumed_all"], f["survivors"]))
    assert all(n > 100 for n in f["suppressed_before_last"])         # suppression is frequent


def test_ties_case_makes_the_tie_rule_matter():
    _, _, _, f = V.ties_case()
    print("VALREF ties", f)
    assert f["tied_share"] >= 0.25 and any(f["rule_changes_survivors"]) and f["score_equals_conf"] > 0


@pytest.mark.parametrize("name", list(V.hand_cases()) + list(V.cap_cases()))
def test_hand_built_nms_decisions_in_the_reference(name):
    c = {**V.hand_cases(), **V.cap_cases()}[name]
    info = []
    got = V.nms_ref(c.det, c.conf, c.thr, info=info, **c.kwargs)[0]
    nc = c.det.shape[2] - 5
    want = c.det[0, c.kept_rows]
    np.testing.assert_array_equal(got[:, :4], want[:, :4])
    np.testing.assert_array_equal(got[:, 4], (want[:, 5:] * want[:, 4:5]).max(1))
    np.testing.assert_array_equal(got[:, 5], want[:, 5:].argmax(1).astype(np.float32))
    expect = dict(iou_equals_thr=2, iou_above_thr=1, same_box_two_classes=2, score_equals_conf=1, obj_passes_score_fails=1,
                  zero_area=4, batches=67, disjoint_299=299, disjoint_300=300, disjoint_301=300, max_nms_100=100, one_class=2)
    if name in expect:
        assert len(got) == expect[name]
    if name == "disjoint_301":                        # the 300th survivor is lane 43 of the fifth 64-lane batch
        assert info[0]["last_rank"] == 299 and 299 % 64 not in (0, 63) and not info[0]["consumed_all"]
    if name == "max_nms_100":                         # rank 100 survives without the cut
        assert len(V.nms_ref(c.det, c.conf, c.thr)[0]) == 120
    if name == "batches":                             # the suppressor of rank 5 / 68 is in its own batch, of rank 69 in the one before
        assert c.kept_rows[:3] == [0, 1, 2] and 5 // 64 == 2 // 64 and 68 // 64 == 66 // 64 and 69 // 64 != 0 // 64
    if name == "class79_offset_rounding":
        _, exact = V._offset_pair()
        assert (len(got) == 1) != (exact > float(np.float32(c.thr)))      # the fp32 offset rounding decides against exact IoU
        assert (c.det[0, :, :4] % 1 != 0).all() and nc == 80


def test_key_cap_case_is_cut_by_the_cap():
    _, _, _, f = V.key_cap_case()
    assert all(900 <= n <= 1200 for n in f["candidates"]) and all(f["cap_changes_result"])


def test_wrapper_case_filter_changes_the_result():
    det, conf, thr = V.wrapper_case()
    a, b = V.nms_ref(det, conf, thr), V.nms_ref(det, conf, thr, classes=[1, 4])
    for x, y in zip(a, b):
        assert len(y) > 0 and set(y[:, 5].tolist()) == {1.0, 4.0} and len(x) > len(y)
    # the same through a masked input (what the reference's post-filter amounts to before the top-30000 cut)
    masked = det.copy()
    masked[..., 5 + np.array([0, 2, 3, 5])] = 0
    for x, y in zip(b, V.nms_ref(masked, conf, thr)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("nc", [2, 80])
@pytest.mark.parametrize("thrs", [V.THRS4, V.THRS8], ids=["T4", "T8"])
def test_match_case_events_occur(nc, thrs):
    f = V.match_case(nc, thrs).facts
    print("VALREF match", nc, len(thrs), {k: v for k, v in f.items() if k != "matched_index"})
    assert f["exact_thr"] >= len(thrs) and f["equal_iou"] >= 1 and f["stolen"] >= 1 and f["over_budget"] == 30
    assert set(V.BITMAP_INDICES) <= f["matched_index"]
    assert f["over_budget_tp"] == 0 and f["duplicates_tp"] == 0 and f["firsts_tp"] == f["expected_firsts"]
    assert f["equal_pair_second_tp"] == 1             # the first detection took the LATER of the two equal ground truths
    assert f["max_gt"] == 256 and f["lanes"] == nc * len(thrs)
    assert f["classes"] == ([0, 63, 64, 79] if nc == 80 else [0, 1])
    assert (nc * len(thrs) > 64) == (nc == 80)        # 80 classes: more (class, threshold) pairs than the block's 64 lanes


def test_evaluator_batches_conditions():
    batches, per_image, f = V.evaluator_batches()
    print("VALREF evaluator", f)
    assert len(batches) == 3 and len(per_image) == 12
    assert f["cross_image_tie_groups_with_mixed_tp"] > 0 and f["order_matters"]
    assert f["dets_without_gt"] and f["gt_without_dets"]
    for dets, _ in batches:
        for d in dets:
            assert (np.diff(d[:, 4]) <= 0).all()
