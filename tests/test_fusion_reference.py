"""CPU checks of tests/fusion_reference.py: the hand cases against their closed forms, and the facts that the random cases were
built for (tests/test_hip_fusion.py compares the kernel with the same reference on the same inputs)."""
import functools

import numpy as np
import pytest

import fusion_reference as fr


@functools.lru_cache(maxsize=None)
def _facts(name):
    return fr.random_facts(fr.random_case(name))


def _run(case, opt, **kw):
    return fr.fuse_ref(case.rows, case.counts, case.view_start, opt["weights"], opt["thr"], opt["agnostic"], opt["max_det"], **kw)


@pytest.mark.parametrize("name", sorted(fr.hand_cases()))
def test_hand_cases(name):
    """expected values from the closed form in fp64; rtol 1e-6 bounds the five or so fp32 roundings (2^-24 each) between
    input and output"""
    case, opt, want = fr.hand_case(name)
    got, = _run(case, opt)
    assert got.dtype == np.float32 and got.shape == want.shape, (got, want)
    np.testing.assert_allclose(got.astype(np.float64), want, rtol=1e-6, atol=0)


def test_lonely_box_bit_for_bit():
    case, opt, _ = fr.hand_case("lonely")
    got, = _run(case, opt)
    assert got[0, :4].tobytes() == case.rows[0, 0, :4].tobytes()
    assert got[0, 4] == np.float32(np.float32(0.9) * np.float32(0.5)) and got[0, 5] == 2


def test_hand_cases_reach_their_paths():
    def info(name):
        case, opt, _ = fr.hand_case(name)
        i = []
        _run(case, opt, info=i)
        return i[0]
    assert info("best_not_first")["not_first"] == 1 and info("tie_iou")["not_first"] == 0
    assert info("overflow")["crowded"] == 1 and info("pair")["crowded"] == 0
    assert info("outranked")["reordered"] and not info("tie_score")["reordered"]
    assert info("max_det") == dict(candidates=15, clusters=10, not_first=0, crowded=0, reordered=True, cut=7)
    assert info("dropped")["candidates"] == 2 and info("zero_area")["clusters"] == 3
    assert info("drift")["clusters"] == 2 and info("at_thr")["clusters"] == 2


@pytest.mark.parametrize("name", fr.RANDOM_CASES)
def test_random_case_facts(name):
    case = fr.random_case(name)
    assert np.isnan(case.rows[np.arange(case.rows.shape[1])[None, :] >= case.counts[:, None]]).all()
    facts = _facts(name)
    views = np.diff(case.view_start)
    for (weights, agnostic, max_det), info in facts.items():
        for i, d in enumerate(info):
            if views[i] > 1 and d["candidates"]:
                assert d["not_first"] >= 1, (name, weights, agnostic, i, d)
                assert d["reordered"], (name, weights, agnostic, i, d)
                assert d["clusters"] < d["candidates"]
        assert any(d["crowded"] for d in info), (name, weights, agnostic)
        assert (sum(d["cut"] for d in info) > 0) == (max_det == 7 or name == "big")
    layout = {"three": [3, 2, 1], "two": [4, 2], "big": [8]}[name]
    assert views.tolist() == layout
    if name == "three":
        assert case.counts[3:].tolist() == [0, 0, 1]
    if name == "big":
        assert ((case.counts >= 250) & (case.counts <= 300)).all()
        for info in facts.values():
            assert info[0]["candidates"] > 2048 and info[0]["clusters"] > 300, info


def test_single_view_at_threshold_one_is_a_sort():
    """one view of weight 1, thr 1: nothing joins, min(1, 1) / 1 = 1 - the input, sorted by score, equal scores in order"""
    rng = np.random.default_rng(7)
    r = np.concatenate((rng.uniform(0, 50, (40, 2)), rng.uniform(60, 90, (40, 2)), rng.uniform(0.1, 0.9, (40, 1)), rng.integers(0, 3, (40, 1))), 1)
    r[10:20] = r[:10]                                              # exact copies: IoU 1 is not > 1
    r = r.astype(np.float32)
    rows, counts = fr.pack_views([r], 64)
    got, = fr.fuse_ref(rows, counts, [0, 1], None, 1.0)
    assert got.tobytes() == r[np.argsort(-r[:, 4], kind="stable")].tobytes()
