"""CPU checks of tiled inference: the host plan (engine/tiles.py) against the closed form and the issue's examples, the merge
reference on hand cases, the facts the GPU tests' random inputs must have, and the argument checks of the two entry points
(refused before any launch, so testable without a GPU)."""
import numpy as np
import pytest

import tiles_reference as T
from object_detection_cib_amd.engine.tiles import axis_origins, tile_plan


# ------------------------------------------------------------------------------------------------------------ plan
def test_axis_origins_examples():
    assert axis_origins(150, 64, 16) == [0, 48, 86]
    assert axis_origins(160, 64, 16) == [0, 48, 96]
    assert axis_origins(64, 64, 16) == [0]
    assert axis_origins(40, 64, 16) == [0]
    assert axis_origins(65, 64, 16) == [0, 1]
    assert axis_origins(112, 64, 16) == [0, 48]            # k * step + S == n is the final origin, not a duplicate of it


@pytest.mark.parametrize("S,o", [(64, 16), (64, 0), (32, 31), (96, 19)])
def test_axis_origins_cover_every_pixel_without_duplicates(S, o):
    for n in list(range(1, 3 * S + 5)) + [1000, 4000]:
        got = axis_origins(n, S, o)
        assert got == T.origins_ref(n, S, o), n
        assert len(set(got)) == len(got) and got == sorted(got) and got[0] == 0
        if n > S:
            assert len(got) == -(-(n - S) // (S - o)) + 1 and got[-1] == n - S
        covered = np.zeros(max(n, S), bool)
        for x0 in got:
            covered[x0:x0 + S] = True
            assert n <= S or x0 + S <= n
        assert covered[:n].all(), n
        assert all(b - a <= S - o for a, b in zip(got, got[1:]))      # neighbours overlap by at least o pixels


def test_plan_order_and_letterbox_rows():
    from object_detection_cib_amd.inference import letterbox_table
    p = tile_plan(100, 150, 64, 0.25)
    assert p.overlap_px == 16 and p.xs == (0, 48, 86) and p.ys == (0, 36) and p.n_tiles == 6 and len(p.views) == 7
    assert [(v.x0, v.y0) for v in p.views[:6]] == [(0, 0), (48, 0), (86, 0), (0, 36), (48, 36), (86, 36)]      # y outer, x inner
    assert all(not v.full and v.letterbox == (-v.x0, -v.y0, 1.0, 1.0, 150, 100) for v in p.views[:6])
    assert p.views[6].full
    for (h, w), S in (((100, 150), 64), ((40, 50), 64), ((3000, 4000), 640), ((31, 17), 64), ((64, 640), 64), ((37, 100), 96)):
        want = letterbox_table([(h, w)], S)[1][0]
        got = np.float32(tile_plan(h, w, S).views[-1].letterbox)
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        ref = T.plan_ref(h, w, S, letterbox_row=lambda h, w, S: letterbox_table([(h, w)], S)[1][0])
        mine = tile_plan(h, w, S).views
        assert [(v.full, v.x0, v.y0) for v in mine] == [(v.full, v.x0, v.y0) for v in ref]
        for a, b in zip(mine, ref):
            np.testing.assert_array_equal(np.float32(a.letterbox).view(np.uint32), b.letterbox.view(np.uint32))
    big = tile_plan(3000, 4000, 640, 0.2)
    # step 512: ceil(3360 / 512) + 1 = 8 origins along x, ceil(2360 / 512) + 1 = 6 along y
    assert big.n_tiles == 48 and len(big.views) == 49 and len(big.xs) == 8 and len(big.ys) == 6


def test_full_view_omission_rule():
    assert [v.full for v in tile_plan(64, 64, 64).views] == [False]                      # one tile, the same pixels
    assert [v.full for v in tile_plan(30, 64, 64).views] == [False]
    assert [v.full for v in tile_plan(40, 50, 64).views] == [False, True]                # one tile, but the letterbox enlarges
    assert [v.full for v in tile_plan(64, 65, 64).views] == [False, False, True]
    assert [v.full for v in tile_plan(64, 65, 64, full_view=False).views] == [False, False]
    assert [v.full for v in tile_plan(40, 50, 64, full_view=False).views] == [False]


def test_plan_value_errors():
    for bad in (0, 31, 33, 100, -64):
        with pytest.raises(ValueError, match="tile"):
            tile_plan(100, 100, bad)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="overlap"):
            tile_plan(100, 100, 64, bad)
    for h, w in ((0, 10), (10, 0), (-1, 5)):
        with pytest.raises(ValueError, match="empty"):
            tile_plan(h, w, 64)


def test_capacity_is_checked_on_the_plan():
    from object_detection_cib_amd import _lib
    from object_detection_cib_amd.inference import tiled_plans
    limit = _lib.lib().kodhip_merge_max_rows()
    assert limit >= 65536
    views = limit // 300                                                   # 218 views of 300 rows fit, 219 do not
    assert len(tiled_plans([(32, 32 * views)], 32, 0.0, False, 300)[0].views) == views
    with pytest.raises(ValueError, match="tile_max_det"):
        tiled_plans([(32, 32 * (views + 1))], 32, 0.0, False, 300)
    assert len(tiled_plans([(32, 32 * (views + 1))], 32, 0.0, False, 299)[0].views) == views + 1
    with pytest.raises(ValueError, match="image 1"):
        tiled_plans([(64, 64), (0, 5)], 64)


# ------------------------------------------------------------------------------------------------------- tile cut
def test_tile_reference_values():
    img = T.noise_image(40, 50, 1)
    t = T.tile_ref(img, 0, 0, 64)
    assert t.shape == (3, 64, 64) and t.dtype == np.float32
    np.testing.assert_array_equal(t[:, :40, :50], (img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
    pad = np.float32(114) / np.float32(255)
    assert (t[:, 40:, :] == pad).all() and (t[:, :, 50:] == pad).all()
    big = T.noise_image(100, 150, 2)
    np.testing.assert_array_equal(T.tile_ref(big, 86, 36, 64), (big[36:100, 86:150].astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
    import torch
    x = torch.from_numpy(np.stack([t, T.tile_ref(big, 48, 0, 64)]))
    want = x.to(torch.bfloat16).view(torch.int16).permute(0, 2, 3, 1).numpy()
    got = T.pairs_ref(x.numpy())
    np.testing.assert_array_equal(got[..., :3], want)
    assert (got[..., 3] == 0).all()


# ---------------------------------------------------------------------------------------------------------- merge
@pytest.mark.parametrize("name", list(T.hand_cases()))
def test_merge_reference_hand_cases(name):
    case, opt, want = T.hand_case(name)
    got = T.merge_ref(case.rows, case.counts, case.view_start, T.THR, **opt)
    assert len(got) == 1
    np.testing.assert_array_equal(got[0].view(np.uint32), want.view(np.uint32), err_msg=name)


def test_merge_reference_hand_case_figures():
    A, B = np.float32([0, 0, 100, 100]), np.float32([0, 0, 50, 50])
    inter = np.float32(2500)
    assert inter / (np.float32(10000) + np.float32(2500) - inter) == np.float32(0.25) and inter / np.float32(2500) == 1
    assert np.float32(904) + np.float32(1) * np.float32(4096) == np.float32(5000)        # what the class offset would do
    h = T.hand_cases()
    assert len(h["contained_iou"][2]) == 2 and len(h["contained_ios"][2]) == 1
    assert len(h["class_aware"][2]) == 2 and len(h["class_agnostic"][2]) == 1
    assert h["hull_nmm"][2][0][:4] == [0, 0, 140, 100] and h["hull_nms"][2][0][:4] == [0, 0, 100, 100]


@pytest.mark.parametrize("name", T.RANDOM_CASES)
def test_random_merge_cases_reach_what_they_are_built_for(name):
    case = T.random_case(name)
    assert np.isnan(case.rows[np.arange(case.max_rows)[None, :] >= case.counts[:, None]]).all()
    assert not np.isnan(case.rows[np.arange(case.max_rows)[None, :] < case.counts[:, None]]).any()
    per_image = [int(case.counts[a:b].sum()) for a, b in zip(case.view_start[:-1], case.view_start[1:])]
    if name == "three":
        assert per_image == [477, 0, 1] and (case.counts == 0).sum() == 3
    if name == "big":
        assert per_image == [5100] and (case.counts == 300).all() and len(case.counts) == 17
    assert float(case.rows[..., :4][~np.isnan(case.rows[..., :4])].max()) > 4096 + 1000
    scores = case.rows[..., 4][~np.isnan(case.rows[..., 4])]
    assert len(np.unique(scores)) < len(scores)                              # ties exist
    facts = T.random_facts(case)
    for (metric, mode, agnostic, max_det), (cand, absorbed, kept, grown) in facts.items():
        assert cand == sum(per_image) and absorbed >= 1 and kept >= 1, (name, metric, mode, agnostic, max_det)
        assert (grown >= 1) == (mode == "nmm"), (name, metric, mode, agnostic, max_det)
        if max_det == 7:
            assert kept == sum(min(7, n) for n in per_image) or name != "big"
    # the options tell the results apart
    if name == "big":
        assert facts[("iou", "nms", False, 300)][1] < facts[("ios", "nms", False, 300)][1] < facts[("ios", "nms", True, 300)][1]
    else:
        assert facts[("iou", "nms", False, 300)][2] > facts[("ios", "nms", False, 300)][2] > facts[("ios", "nms", True, 300)][2]
    if name == "big":
        assert facts[("ios", "nmm", False, 300)][2] == 300                   # the max_det cut acts at 300 too


# ------------------------------------------------------------------------------------------------------------ ABI
def test_argument_errors_without_a_gpu():
    from object_detection_cib_amd import _lib
    h = _lib.lib()
    assert h.kodhip_version() >= 106 and h.kodhip_tile_desc_bytes() == 24 and h.kodhip_merge_max_rows() >= 65536
    p = 4096                                                                 # (never dereferenced: every call is refused)
    for args, msg in (((None, p, p, p, 1, 64), "null"), ((p, None, p, p, 1, 64), "null"), ((p, p, None, None, 1, 64), "both outputs"),
                      ((p, p, p, p, 0, 64), "T must"), ((p, p, p, p, 1, 0), "S even"), ((p, p, p, p, 1, 63), "S even"),
                      ((p, p, p + 4, None, 1, 64), "aligned")):
        rc = h.kodhip_tile_batch(*args, None)
        err = h.kodhip_last_error().decode()
        assert rc < 0 and "tile_batch" in err and msg in err, (args, rc, err)
    good = dict(rows=p, counts=p, view_start=p, keys=p, key_cap=64, out=p, nout=p, n_images=1, max_rows=4, max_det=300, metric=1,
                thr=0.5, mode=1, agnostic=0)
    for kw, msg in ((dict(rows=None), "null"), (dict(counts=None), "null"), (dict(view_start=None), "null"), (dict(keys=None), "null"),
                    (dict(out=None), "null"), (dict(nout=None), "null"), (dict(max_det=0), "max_det"), (dict(max_det=301), "max_det"),
                    (dict(metric=2), "metric"), (dict(metric=-1), "metric"), (dict(mode=2), "mode"), (dict(thr=-0.1), "thr"),
                    (dict(thr=1.5), "thr"), (dict(thr=float("nan")), "thr"), (dict(key_cap=32), "key_cap"), (dict(key_cap=100), "key_cap"),
                    (dict(key_cap=2 * h.kodhip_merge_max_rows()), "key_cap"), (dict(n_images=0), "n_images"), (dict(max_rows=0), "max_rows"),
                    (dict(agnostic=2), "agnostic")):
        a = dict(good, **kw)
        rc = h.kodhip_merge_detections(*[a[k] for k in good], None)
        err = h.kodhip_last_error().decode()
        assert rc < 0 and "merge_detections" in err and msg in err, (kw, rc, err)
