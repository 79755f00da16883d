"""The tracker on the device: kodhip_track_reset / kodhip_track_update (csrc/tracking.hip) through the C ABI with the test's
own poisoned buffers, `ByteTracker`, and `TrackedDetector` end to end, against the plain reference of tests/track_reference.py.

Everything is compared exactly, on bit patterns - outputs, ids, counts and the whole published state after every frame: the
tracker is comparison logic and singly rounded fp32 arithmetic (the library is built without contraction; fp32 division is
correctly rounded).  That the scenarios reach what they were built for is asserted on the CPU (tests/test_track_reference.py);
the detector test asserts its own conditions before it compares.  Figures are printed before they are asserted (`pytest -s`).

Measured on an MI355X: every comparison exact; the detector scene gives 12 - 19 rows per frame between thresholds 0.815386 and
0.817303, 9 / 7 / 3 / 2 / 5 / 5 emitted tracks, 11 ids that live two or three frames and one second-association match, the same
eager, graphed and through clip(); the 25 tests take 1.6 s.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fusion_helpers as H  # noqa: E402
import track_reference as tr  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402
from object_detection_cib_amd.core.tracking import ByteTracker, Tracks, state_dtype  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo  # noqa: E402

ANCH = LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
GUARD, SENTINEL, POISON = 1024, -7.0, 0x5A


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def _stride(cap):
    return tr.HEADER.itemsize + cap * tr.TRACK.itemsize


class Direct:
    """S streams of kodhip_track_update with the test's own buffers: GUARD poisoned bytes behind the state, a poisoned
    workspace, poisoned outputs, NaN rows beyond the counts"""

    def __init__(self, S, cap, p, max_rows=12):
        self.S, self.cap, self.p, self.max_rows = S, cap, p, max_rows
        self.n = S * _stride(cap)
        self.state = torch.full((self.n + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        self.work = torch.full((GUARD,), POISON, dtype=torch.uint8, device="cuda")
        assert _lib.lib().kodhip_track_workspace_bytes(S, cap, max_rows) == 0
        _lib.check(_lib.lib().kodhip_track_reset(self.state.data_ptr(), S, cap, stream()), "track_reset")

    def state_bytes(self, s):
        b = self.state.cpu().numpy()
        assert (b[self.n:] == POISON).all(), "the state's guard was written"
        return b[s * _stride(self.cap):(s + 1) * _stride(self.cap)].tobytes()

    def call(self, frames, **over):
        """frames[s][f]: [n, 6] arrays -> (rc, per stream and frame (out, ids))"""
        S, cap, R, p = self.S, self.cap, self.max_rows, self.p
        F = len(frames[0])
        rows = np.full((S, F, R, 6), np.nan, np.float32)
        counts = np.zeros((S, F), np.int32)
        for s in range(S):
            for f in range(F):
                r = np.asarray(frames[s][f], np.float32).reshape(-1, 6)
                rows[s, f, :len(r)], counts[s, f] = r, len(r)
        rows_d, counts_d = torch.from_numpy(rows).cuda(), torch.from_numpy(counts).cuda()
        out = torch.full((S, F, cap, 6), SENTINEL, device="cuda")
        ids = torch.full((S, F, cap, 2), -77, dtype=torch.int32, device="cuda")
        nout = torch.full((S, F), -1, dtype=torch.int32, device="cuda")
        a = dict(state=self.state.data_ptr(), rows=rows_d.data_ptr(), counts=counts_d.data_ptr(), S=S, F=F, max_rows=R, cap=cap,
                 high=p.high, low=p.low, new=p.new, sim1=p.sim1, sim2=p.sim2, sim3=p.sim3, fuse_score=p.fuse_score, agnostic=p.agnostic,
                 max_lost=p.max_lost, out=out.data_ptr(), out_ids=ids.data_ptr(), nout=nout.data_ptr(), workspace=self.work.data_ptr())
        a.update(over)
        rc = _lib.lib().kodhip_track_update(*a.values(), stream())
        torch.cuda.synchronize()
        k, o, i = nout.cpu().numpy(), out.cpu().numpy(), ids.cpu().numpy()
        assert (self.work.cpu().numpy() == POISON).all(), "the workspace was written"
        if rc != 0:
            assert (k == -1).all() and (o == SENTINEL).all() and (i == -77).all(), "a refused call wrote its outputs"
            return rc, None
        assert ((0 <= k) & (k <= cap)).all(), k
        res = []
        for s in range(S):
            for f in range(F):                                        # nothing written behind the emitted rows
                assert (o[s, f, k[s, f]:] == SENTINEL).all() and (i[s, f, k[s, f]:] == -77).all()
            res.append([(o[s, f, :k[s, f]], i[s, f, :k[s, f]]) for f in range(F)])
        return rc, res


def _same_frame(got, want_out, want_ids, tag):
    o, i = got
    assert len(o) == len(want_out), (tag, len(o), len(want_out))
    np.testing.assert_array_equal(i, want_ids, err_msg=f"{tag} ids")
    np.testing.assert_array_equal(_bits(o), _bits(want_out), err_msg=f"{tag} rows")


def _same_state(got: bytes, want: bytes, cap, tag):
    if got != want:
        g, w = (np.frombuffer(b, state_dtype(cap))[0] for b in (got, want))
        for name in tr.HEADER.names:
            assert g[name] == w[name], (tag, name, g[name], w[name])
        for t in range(cap):
            assert g["tracks"][t].tobytes() == w["tracks"][t].tobytes(), (tag, "slot", t, g["tracks"][t], w["tracks"][t])
    assert got == want, tag


def _grow(state: bytes, cap_from, cap_to):
    """the reference's state at cap_from as the state of a tracker with cap_to slots that never used more"""
    return state + bytes((cap_to - cap_from) * tr.TRACK.itemsize)


# ------------------------------------------------------------------------------------------------------ hand scenarios
@pytest.mark.parametrize("name", sorted(tr.SCENARIOS))
def test_track_scenarios(name):
    s, want = tr.scenario(name), tr.scenario_run(name)
    d = Direct(1, s.cap, s.params, max_rows=max(12, max(len(f) for f in s.frames)))
    assert d.state_bytes(0) == tr.RefTracker(s.cap, s.params).state_bytes(), "reset"
    for f, rows in enumerate(s.frames):
        rc, got = d.call([[rows]])
        _lib.check(rc, "track_update")
        _same_frame(got[0][0], want.outs[f], want.ids[f], f"{name} frame {f + 1}")
        _same_state(d.state_bytes(0), want.states[f], s.cap, f"{name} frame {f + 1}")
    print(f"TRACK {name}: emitted {[len(o) for o in want.outs]}, ids {int(want.tracker.header['next_id']) - 1}, "
          f"dropped {int(want.tracker.header['dropped'])}")


# ------------------------------------------------------------------------------------------------------ the random case
@pytest.mark.parametrize("cap,max_rows", [(64, 32), (1024, 300)])
def test_track_random_case(cap, max_rows):
    frames, want = tr.random_frames(), tr.random_run()
    d = Direct(1, cap, tr.params(**tr.RANDOM_PARAMS), max_rows=max_rows)
    for f, rows in enumerate(frames):
        rc, got = d.call([[rows]])
        _lib.check(rc, "track_update")
        _same_frame(got[0][0], want.outs[f], want.ids[f], f"random cap {cap} frame {f + 1}")
        _same_state(d.state_bytes(0), _grow(want.states[f], 64, cap), cap, f"random cap {cap} frame {f + 1}")
    print(f"TRACK random cap {cap}: emitted {[len(o) for o in want.outs]}")


# ------------------------------------------------------------------------------------------------------ structure
def test_track_clip_equals_single_frames():
    frames, want = tr.random_frames()[:8], tr.random_run()
    d = Direct(1, 64, tr.params(**tr.RANDOM_PARAMS), max_rows=32)
    rc, got = d.call([frames])
    _lib.check(rc, "track_update")
    for f in range(8):
        _same_frame(got[0][f], want.outs[f], want.ids[f], f"F = 8 frame {f + 1}")
    _same_state(d.state_bytes(0), want.states[7], 64, "F = 8")


@functools.lru_cache(maxsize=None)
def _stream_runs():
    frames = tr.random_frames()
    sets = [frames[0:8], frames[10:18], frames[20:28]]
    return sets, [tr.run_ref(fs, tr.params(**tr.RANDOM_PARAMS), 64) for fs in sets]


def test_track_streams_are_independent_and_reset_is_per_stream():
    sets, want = _stream_runs()
    assert len({w.states[-1] for w in want}) == 3
    d = Direct(3, 64, tr.params(**tr.RANDOM_PARAMS), max_rows=32)
    for f0 in (0, 4):                                                 # two launches of F = 4
        rc, got = d.call([fs[f0:f0 + 4] for fs in sets])
        _lib.check(rc, "track_update")
        for s in range(3):
            for f in range(4):
                _same_frame(got[s][f], want[s].outs[f0 + f], want[s].ids[f0 + f], f"stream {s} frame {f0 + f + 1}")
    for s in range(3):
        _same_state(d.state_bytes(s), want[s].states[-1], 64, f"stream {s}")
    _lib.check(_lib.lib().kodhip_track_reset(d.state.data_ptr() + _stride(64), 1, 64, stream()), "track_reset")
    fresh = tr.RefTracker(64, d.p).state_bytes()
    assert d.state_bytes(1) == fresh and d.state_bytes(0) == want[0].states[-1] and d.state_bytes(2) == want[2].states[-1]


def test_track_argument_errors_launch_nothing():
    s = tr.scenario("birth")
    d = Direct(1, 64, s.params)
    rc, _ = d.call([[s.frames[0]]])
    _lib.check(rc, "track_update")
    before = d.state_bytes(0)
    h = _lib.lib()
    nan = float("nan")
    for kw, msg in ((dict(state=None), "null"), (dict(rows=None), "null"), (dict(counts=None), "null"), (dict(out=None), "null"),
                    (dict(out_ids=None), "null"), (dict(nout=None), "null"), (dict(S=0), "S must"), (dict(F=0), "F >= 1"),
                    (dict(max_rows=0), "max_rows"), (dict(max_rows=301), "max_rows"), (dict(cap=32), "cap"), (dict(cap=96), "cap"),
                    (dict(cap=2048), "cap"), (dict(high=1.5), "thresholds"), (dict(low=-0.1), "thresholds"), (dict(new=nan), "thresholds"),
                    (dict(sim1=1.25), "thresholds"), (dict(sim2=-1.0), "thresholds"), (dict(sim3=2.0), "thresholds"),
                    (dict(low=0.7, high=0.6), "low_thres"), (dict(fuse_score=2), "0 or 1"), (dict(agnostic=-1), "0 or 1"),
                    (dict(max_lost=-1), "max_lost")):
        rc, _ = d.call([[s.frames[1]]], **kw)
        assert rc < 0 and msg.encode() in h.kodhip_last_error(), (kw, rc, h.kodhip_last_error())
        assert d.state_bytes(0) == before, kw
    for args, msg in (((None, 1, 64), "null"), ((d.state.data_ptr(), 0, 64), "S must"), ((d.state.data_ptr(), 1, 48), "cap")):
        assert h.kodhip_track_reset(*args, stream()) < 0 and msg.encode() in h.kodhip_last_error()
    torch.cuda.synchronize()
    assert d.state_bytes(0) == before
    assert h.kodhip_version() >= 109 and h.kodhip_track_header_bytes() == 16 and h.kodhip_track_bytes() == 112


# ------------------------------------------------------------------------------------------------------ ByteTracker
def test_bytetracker_equals_the_direct_call():
    sets, want = _stream_runs()
    kw = dict(streams=3, capacity=64, **{k: v for k, v in tr.RANDOM_PARAMS.items()})
    trk = ByteTracker(**kw)
    assert trk.state().tobytes() == tr.RefTracker(64, tr.params()).state_bytes() * 3

    def pack(rows_list, shape):
        rows = np.full(shape + (32, 6), np.nan, np.float32).reshape(-1, 32, 6)
        counts = np.zeros(len(rows), np.int32)
        for k, r in enumerate(rows_list):
            rows[k, :len(r)], counts[k] = r, len(r)
        return torch.from_numpy(rows.reshape(shape + (32, 6))).cuda(), torch.from_numpy(counts.reshape(shape)).cuda()

    for f in range(4):                                                # one frame per stream
        res = trk.update(pack([fs[f] for fs in sets], (3,)))
        assert isinstance(res, Tracks) and len(res) == 3 and tuple(res.packed.shape) == (3, 1, 64, 6) and tuple(res.counts.shape) == (3, 1)
        for s in range(3):
            ids = np.stack([res.ids[s].cpu().numpy(), res.det_index[s].cpu().numpy()], 1)
            _same_frame((res[s].cpu().numpy(), ids), want[s].outs[f], want[s].ids[f], f"update stream {s} frame {f + 1}")
    res = trk.update(pack([fs[f] for fs in sets for f in range(4, 8)], (3, 4)))      # [S, F, ...]: stream-major entries
    assert len(res) == 12
    for s in range(3):
        for f in range(4):
            ids = np.stack([res.ids[s * 4 + f].cpu().numpy(), res.det_index[s * 4 + f].cpu().numpy()], 1)
            _same_frame((res[s * 4 + f].cpu().numpy(), ids), want[s].outs[4 + f], want[s].ids[4 + f], f"clip stream {s} frame {f + 5}")
    st = trk.state()
    assert st.shape == (3,) and st.tobytes() == b"".join(w.states[-1] for w in want)
    assert trk.dropped == [0, 0, 0]
    trk.reset(1)
    st = trk.state()
    assert st[1]["frame"] == 0 and st[1]["next_id"] == 1 and (st[1]["tracks"]["state"] == 0).all() and st[0]["frame"] == 8 and st[2]["frame"] == 8
    one = trk.update(pack(sets[1][:2], (2,)), stream=1)               # the frames of one stream
    assert len(one) == 2 and trk.state()[1]["frame"] == 2 and trk.state()[0].tobytes() == want[0].states[-1]
    _same_frame((one[1].cpu().numpy(), np.stack([one.ids[1].cpu().numpy(), one.det_index[1].cpu().numpy()], 1)), want[1].outs[1],
                want[1].ids[1], "one stream")
    for kwargs, msg in ((dict(capacity=100), "capacity"), (dict(streams=0), "streams"), (dict(track_thresh=1.5), "track_thresh"),
                        (dict(low_thresh=0.7), "low_thresh"), (dict(track_buffer=-1), "track_buffer"), (dict(match_thresh=-0.5), "match_thresh")):
        with pytest.raises(ValueError, match=msg):
            ByteTracker(**kwargs)
    with pytest.raises(ValueError, match="rows"):
        trk.update(pack([sets[0][0]], (1,)))                          # B != streams


# ------------------------------------------------------------------------------------------------------ TrackedDetector
S_IMG, BATCH, FRAMES = 128, 4, 6


@pytest.fixture(scope="module")
def net():
    n = H.network(5, 0.25)
    with torch.no_grad():                                             # boxes about half an anchor wide: neighbours in time overlap
        for name, p in n.named_parameters():
            if name.endswith("box_head.conv.bias"):
                p.copy_(torch.tensor([0.0, 0.0, -0.5, -0.5]).repeat(p.numel() // 4))
    n.fuse_eval(False)
    return n


@pytest.fixture(scope="module")
def scene(net):
    """(frames, conf_thres, track_thresh): a 96 x 128 window moving 2 px per frame over a blocky canvas; the thresholds sit
    between two scores, about 12 rows over conf_thres and 6 over track_thresh in the sparsest frame"""
    from object_detection_cib_amd.inference import Detector
    rng = np.random.default_rng(11)
    canvas = np.kron(rng.integers(0, 256, (12, 18, 3)), np.ones((8, 8, 1))) + rng.integers(-8, 9, (96, 144, 3))
    canvas = np.clip(canvas, 0, 255).astype(np.uint8)
    frames = [np.ascontiguousarray(canvas[:, 2 * f:2 * f + 128]) for f in range(FRAMES)]
    rows = [r.cpu().numpy() for r in Detector(net, ANCH, image_size=S_IMG, batch_size=BATCH, conf_thres=0.0, max_det=300)(frames)]
    scores = np.stack([np.sort(r[:, 4])[::-1][:20] for r in rows])
    assert scores.shape == (FRAMES, 20) and (scores[:, :14] > 0).all() and (scores < 1).all()
    conf = float(np.float32((scores[:, 11].min() + scores[:, 12].min()) / 2))
    track = float(np.float32((scores[:, 5].min() + scores[:, 6].min()) / 2))
    assert 0 < conf < track < 1
    return frames, conf, track


def _collect(res: Tracks):
    return [(r.cpu().numpy(), np.stack([i.cpu().numpy(), d.cpu().numpy()], 1)) for r, i, d in zip(res, res.ids, res.det_index)]


def _tracked(net, scene, **kw):
    from object_detection_cib_amd.inference import TrackedDetector
    _, conf, track = scene
    return TrackedDetector(net, ANCH, image_size=S_IMG, batch_size=BATCH, conf_thres=conf, capacity=64, track_thresh=track, low_thresh=conf,
                           new_thresh=track, match_thresh=0.9, match_thresh_low=0.9, match_thresh_new=0.9, fuse_score=False,
                           track_buffer=2, **kw)


@pytest.fixture(scope="module")
def eager_run(net, scene):
    """frame-by-frame TrackedDetector calls: per frame (rows, ids), and the final state"""
    det = _tracked(net, scene)
    got = [_collect(det([f]))[0] for f in scene[0]]
    return got, det.tracker.state().tobytes()


def test_tracked_detector_equals_the_composition(net, scene, eager_run):
    from object_detection_cib_amd.inference import Detector
    frames, conf, track = scene
    p = tr.params(track_thresh=track, low_thresh=conf, new_thresh=track, match_thresh=0.9, match_thresh_low=0.9, match_thresh_new=0.9,
                  fuse_score=False, track_buffer=2)
    plain = Detector(net, ANCH, image_size=S_IMG, batch_size=BATCH, conf_thres=conf)
    trk = ByteTracker(streams=1, capacity=64, track_thresh=track, low_thresh=conf, new_thresh=track, match_thresh=0.9, match_thresh_low=0.9,
                      match_thresh_new=0.9, fuse_score=False, track_buffer=2)
    ref = tr.RefTracker(64, p)
    counts, composed, want = [], [], []
    for f in frames:
        rows = plain([f])[0]
        counts.append(len(rows))
        packed = torch.full((1, 300, 6), float("nan"), device="cuda")
        packed[0, :len(rows)] = rows
        composed.append(_collect(trk.update((packed, torch.tensor([len(rows)], dtype=torch.int32, device="cuda"))))[0])
        want.append(ref.step(rows.cpu().numpy()))
    lives = {}
    for _, ids in want:
        for i in ids[:, 0].tolist():
            lives[i] = lives.get(i, 0) + 1
    print(f"TRACK detector: conf {conf:.6g}, track {track:.6g}, rows per frame {counts}, emitted {[len(o) for o, _ in want]}, "
          f"frames per id {lives}, second-association matches {sum(len(e['assoc'][1]['matches']) for e in ref.log)}")
    assert min(counts) >= 1 and max(lives.values(), default=0) >= 2
    got, state = eager_run
    for f in range(FRAMES):
        _same_frame(composed[f], *want[f], f"composition frame {f + 1}")
        _same_frame(got[f], *want[f], f"detector frame {f + 1}")
        o = got[f][0]                                                 # finite boxes (the filter's, so not clipped to the frame)
        assert np.isfinite(o).all()
    _same_state(state, ref.state_bytes(), 64, "detector")
    assert trk.state().tobytes() == state


def test_tracked_detector_graphed_and_clip(net, scene, eager_run):
    frames = scene[0]
    got, state = eager_run
    det = _tracked(net, scene, graphed=True)
    for f, frame in enumerate(frames):
        _same_frame(_collect(det([frame]))[0], *got[f], f"graphed frame {f + 1}")
    assert det.tracker.state().tobytes() == state
    det = _tracked(net, scene, streams=2)
    res = det.clip(frames, stream=1)                                  # chunks of 4 and 2 (padded to 4) frames
    assert len(res) == FRAMES and tuple(res.counts.shape) == (1, FRAMES)
    for f, pair in enumerate(_collect(res)):
        _same_frame(pair, *got[f], f"clip frame {f + 1}")
    st = det.tracker.state()
    assert st[1].tobytes() == state and st[0]["frame"] == 0


def test_tracked_detector_value_errors(net):
    from object_detection_cib_amd.inference import TrackedDetector
    with pytest.raises(ValueError, match="conf_thres"):
        TrackedDetector(net, ANCH, image_size=S_IMG, conf_thres=0.6, track_thresh=0.5)
    d = TrackedDetector(net, ANCH, image_size=S_IMG, batch_size=BATCH, streams=2, capacity=64)
    assert d.conf_thres == 0.1
    with pytest.raises(ValueError, match="one frame per stream"):
        d([np.zeros((64, 64, 3), np.uint8)])
    with pytest.raises(ValueError, match="stream"):
        d.clip([np.zeros((64, 64, 3), np.uint8)], stream=2)
