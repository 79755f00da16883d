"""CPU checks of the tracker's plain reference (tests/track_reference.py): the per-coordinate fp32 Kalman filter against
ByteTrack's 8 x 8 fp64 matrix form, and every scenario of tests/test_hip_track.py reaching the branch it was built for - a
case that stops exercising its branch fails here instead of passing silently on the GPU.

Filter, 200 random 60-frame tracks (boxes up to 4000 px, h from 8 to 800, 20 % missed frames), measured: worst error of the
means 4.0e-5 of h, worst relative error of a covariance entry 5.0e-6, every entry outside the four 2 x 2 blocks of the fp64
form exactly 0.  The assertions stand at 4 times the measured figures.
"""
import numpy as np
import pytest

import track_reference as tr

MEAN_BOUND, COV_BOUND = 4 * 4.0e-5, 4 * 5.01e-6


def test_filter_equals_the_matrix_form():
    rng = np.random.default_rng(2024)
    worst_m = worst_c = worst_off = 0.0
    for _ in range(200):
        m, c, off = tr.filter_errors(tr.filter_track(rng))
        worst_m, worst_c, worst_off = max(worst_m, m), max(worst_c, c), max(worst_off, off)
    print(f"TRACK filter: worst mean error / h {worst_m:.3g}, worst relative covariance error {worst_c:.3g}, off-block {worst_off:g}")
    assert worst_off == 0.0
    assert worst_m <= MEAN_BOUND and worst_c <= COV_BOUND


def test_layout_and_parameters():
    assert tr.HEADER.itemsize == 16 and tr.TRACK.itemsize == 112 and tr.TRACK.itemsize % 16 == 0
    assert tr.TRACK.fields["kf"][1] == 24 and tr.TRACK.fields["pad"][1] == 104
    p = tr.params()
    assert p.high == float(np.float32(0.5)) and p.low == float(np.float32(0.1)) and p.new == float(np.float32(0.5 + 0.1))
    assert (p.sim1, p.sim2, p.sim3) == tuple(float(np.float32(1.0 - m)) for m in (0.8, 0.5, 0.7))
    assert (p.fuse_score, p.agnostic, p.max_lost) == (1, 1, 30)


def test_greedy_is_the_sorted_pass():
    """the literal pass on a crowded random matrix: accepted pairs are disjoint, in sorted order, and every rejected
    admissible pair has a side that an earlier pair took"""
    rng = np.random.default_rng(5)
    boxes = {t: [np.float32(v) for v in tr.box(*rng.uniform(80, 160, 2), 60, 60)[:4]] for t in range(10)}
    rows = np.asarray([tr.box(*rng.uniform(80, 160, 2), 60, 60, float(rng.uniform(0.5, 1))) for _ in range(12)], np.float32)
    info = []
    acc = tr.associate(list(range(10)), list(range(12)), boxes, {t: 0.0 for t in boxes}, rows, 0.1, True, True, info)
    pairs = info[0]["pairs"]
    assert len(pairs) > 40 and 5 <= len(acc) <= 10
    assert len({t for t, _ in acc}) == len(acc) == len({d for _, d in acc})
    order = {(t, d): i for i, (t, d, _) in enumerate(pairs)}
    assert [s for _, _, s in pairs] == sorted((s for _, _, s in pairs), reverse=True)
    for (t, d), i in order.items():
        if (t, d) not in acc:
            assert any((a == t or b == d) and order[(a, b)] < i for a, b in acc)
    first = {}
    for t, d, _ in pairs:
        first.setdefault(t, d)
    assert any(first[t] != d for t, d in acc)                # greedy is not "every track's own first choice"


@pytest.mark.parametrize("name", sorted(tr.SCENARIOS))
def test_scenario_reaches_its_branch(name):
    s = tr.scenario(name)
    assert s.cap == 64 and len(s.frames) <= 12 and (name == "overflow" or max(len(f) for f in s.frames) <= 12)
    run = tr.scenario_run(name)
    s.check(run)
    for o, i in zip(run.outs, run.ids):
        assert o.dtype == np.float32 and i.dtype == np.int32 and len(o) == len(i)


def test_fuse_score_and_classes_change_the_result():
    assert tr.scenario_run("fuse_on").ids[1].tolist() != tr.scenario_run("fuse_off").ids[1].tolist()
    assert tr.scenario_run("class_agnostic").states[-1] != tr.scenario_run("class_aware").states[-1]
    assert tr.scenario_run("threshold_at").states[-1] != tr.scenario_run("threshold_below").states[-1]


def test_random_case_is_busy():
    frames, run = tr.random_frames(), tr.random_run()
    assert len(frames) == 40 and max(len(f) for f in frames) <= 26
    log = run.log
    second = sum(len(e["assoc"][1]["matches"]) for e in log)
    third = sum(len(e["assoc"][2]["matches"]) for e in log)
    freed = sum(len(e["freed_new"]) for e in log)
    removed = sum(len(e["removed"]) for e in log)
    lost = sum(len(e["lost"]) for e in log)
    contested = sum(len(a["pairs"]) > len(a["matches"]) for e in log for a in e["assoc"])
    hdr = run.tracker.header
    revived = 0
    for f in range(2, 40):            # an id that is emitted again after a frame without it
        before, earlier = set(run.ids[f - 1][:, 0].tolist()), set().union(*(set(i[:, 0].tolist()) for i in run.ids[:f - 1]))
        revived += len((set(run.ids[f][:, 0].tolist()) - before) & earlier)
    print(f"TRACK random: ids {int(hdr['next_id']) - 1}, second-association matches {second}, third {third}, new freed {freed}, "
          f"lost {lost}, removed {removed}, revived {revived}, contested associations {contested}, dropped {int(hdr['dropped'])}")
    assert second >= 10 and third >= 5 and freed >= 3 and removed >= 3 and revived >= 5 and contested >= 3
    assert int(hdr["dropped"]) == 0 and 20 <= int(hdr["next_id"]) - 1
    assert max(len(o) for o in run.outs) >= 15
