"""Plain reference of the tracker (kodhip_track_update, csrc/tracking.hip): numpy float32 scalars and Python loops, the
sorted-pair greedy pass written literally and the frame steps of include/kodhip.h one after the other.  Every operation is
one float32 operation, in the order the header gives, so the kernel is compared with it on bit patterns.

Also `MatrixFilter`: ByteTrack's Kalman filter in its usual form - 8-state mean, 8 x 8 fp64 covariance, F, H, diag Q / R,
K = P H^T S^-1, P - K S K^T - as a second, independent form of the per-coordinate filter.

The scenarios of the GPU tests are built here, each with a `check(run)` that asserts the branch it was built for was taken
(tests/test_track_reference.py runs them on the CPU)."""
from __future__ import annotations

import functools
from typing import Callable, List, NamedTuple, Optional

import numpy as np

F32 = np.float32
FREE, NEW, TRACKED, LOST = 0, 1, 2, 3
WP, WV = F32(0.05), F32(0.00625)

HEADER = np.dtype([("frame", "<i4"), ("next_id", "<i4"), ("dropped", "<i4"), ("pad", "<i4")])
TRACK = np.dtype([("state", "<i4"), ("id", "<i4"), ("last_frame", "<i4"), ("start_frame", "<i4"), ("score", "<f4"), ("cls", "<f4"),
                  ("kf", "<f4", (4, 5)), ("pad", "<i4", (2,))])
assert HEADER.itemsize == 16 and TRACK.itemsize == 112


class Params(NamedTuple):
    high: float
    low: float
    new: float
    sim1: float
    sim2: float
    sim3: float
    fuse_score: int
    agnostic: int
    max_lost: int


def params(track_thresh=0.5, low_thresh=0.1, new_thresh=None, match_thresh=0.8, match_thresh_low=0.5, match_thresh_new=0.7,
           fuse_score=True, agnostic=True, track_buffer=30, **over) -> Params:
    """ByteTracker's keywords -> the kernel's arguments (the sims are float32(1 - match_thresh), formed in double)"""
    new = float(track_thresh) + 0.1 if new_thresh is None else float(new_thresh)
    p = Params(float(F32(track_thresh)), float(F32(low_thresh)), float(F32(new)), float(F32(1.0 - float(match_thresh))),
               float(F32(1.0 - float(match_thresh_low))), float(F32(1.0 - float(match_thresh_new))), int(bool(fuse_score)),
               int(bool(agnostic)), int(track_buffer))
    return p._replace(**over)


# ------------------------------------------------------------------------------------------------ the fp32 filter
def measure(row):
    x1, y1, x2, y2 = (F32(v) for v in row[:4])
    w, h = x2 - x1, y2 - y1
    return [x1 + w / F32(2), y1 + h / F32(2), w / h, h]


def usable(row) -> bool:
    w, h = F32(row[2]) - F32(row[0]), F32(row[3]) - F32(row[1])
    return bool(w > 0 and h > 0 and not np.isnan(F32(row[4])))


def track_box(kf):
    cx, cy, a, h = (F32(kf[c][0]) for c in range(4))
    w = a * h
    x1, y1 = cx - w / F32(2), cy - h / F32(2)
    return [x1, y1, x1 + w, y1 + h]


def initiate(z):
    kf = np.zeros((4, 5), F32)
    h = F32(z[3])
    for c in range(4):
        sp = F32(1e-2) if c == 2 else F32(0.1) * h
        sv = F32(1e-5) if c == 2 else F32(0.0625) * h
        kf[c] = (z[c], F32(0), sp * sp, F32(0), sv * sv)
    return kf


def predict(kf):
    hh = F32(kf[3][0])
    out = np.zeros((4, 5), F32)
    for c in range(4):
        sp = F32(1e-2) if c == 2 else WP * hh
        sv = F32(1e-5) if c == 2 else WV * hh
        p, v, ppp, ppv, pvv = (F32(x) for x in kf[c])
        out[c] = (p + v, v, ((ppp + F32(2) * ppv) + pvv) + sp * sp, ppv + pvv, pvv + sv * sv)
    return out


def update(kf, z):
    hh = F32(kf[3][0])
    out = np.zeros((4, 5), F32)
    for c in range(4):
        sr = F32(1e-1) if c == 2 else WP * hh
        p, v, ppp, ppv, pvv = (F32(x) for x in kf[c])
        S = ppp + sr * sr
        kp, kv, y = ppp / S, ppv / S, F32(z[c]) - p
        out[c] = (p + kp * y, v + kv * y, ppp - (kp * kp) * S, ppv - (kp * kv) * S, pvv - (kv * kv) * S)
    return out


def similarity(A, B, score, fuse):
    """kodhip_fuse_detections' IoU of track box A and detection box B (fmaxf / fminf: a NaN operand is passed over), times
    the detection's score where fuse applies"""
    w = np.fmax(F32(0), np.fmin(A[2], B[2]) - np.fmax(A[0], B[0]))
    h = np.fmax(F32(0), np.fmin(A[3], B[3]) - np.fmax(A[1], B[1]))
    inter = w * h
    aa, ab = (A[2] - A[0]) * (A[3] - A[1]), (B[2] - B[0]) * (B[3] - B[1])
    iou = inter / ((aa + ab) - inter)
    return iou * F32(score) if fuse else iou


def associate(tracks, dets, boxes, tcls, rows, thr, fuse, agnostic, info=None):
    """tracks: slots, dets: rows, both still open -> [(t, d)] accepted: the admissible pairs with sim > thr, sorted by sim
    descending, then slot, then row; a pair is accepted iff neither side is taken"""
    pairs = []
    for t in tracks:
        for d in dets:
            if not agnostic and F32(tcls[t]) != F32(rows[d][5]):
                continue
            s = similarity(boxes[t], [F32(v) for v in rows[d][:4]], rows[d][4], fuse)
            if s > F32(thr):
                pairs.append((-float(s), t, d))
    pairs.sort()
    taken_t, taken_d, acc = set(), set(), []
    for _, t, d in pairs:
        if t not in taken_t and d not in taken_d:
            taken_t.add(t); taken_d.add(d); acc.append((t, d))
    if info is not None:
        info.append({"pairs": [(t, d, -s) for s, t, d in pairs], "matches": list(acc)})
    return acc


class RefTracker:
    """one stream of kodhip_track_update; `header` and `tracks` are the published state, bit for bit"""

    def __init__(self, cap: int, p: Params):
        self.cap, self.p = cap, p
        self.header = np.zeros((), HEADER)
        self.header["next_id"] = 1
        self.tracks = np.zeros(cap, TRACK)
        self.log = []                 # per frame: {"assoc": [phase 1, 2, 3], "created": [...], "freed_new": [...], "removed": [...]}

    def state_bytes(self) -> bytes:
        return self.header.tobytes() + self.tracks.tobytes()

    def step(self, rows):
        """rows [n, 6] float32 -> (out [k, 6] float32, ids [k, 2] int32)"""
        p, T = self.p, self.tracks
        rows = np.asarray(rows, F32).reshape(-1, 6)
        with np.errstate(all="ignore"):
            return self._step(p, T, rows)

    def _step(self, p, T, rows):
        self.header["frame"] += 1
        frame = int(self.header["frame"])
        n = len(rows)
        entry = {"assoc": [], "created": [], "freed_new": [], "removed": [], "lost": []}
        # 1. predict
        boxes, tcls = {}, {}
        for t in range(self.cap):
            st = int(T[t]["state"])
            if st == FREE:
                continue
            if st in (TRACKED, LOST):
                if st == LOST:
                    T[t]["kf"][3][1] = 0
                T[t]["kf"] = predict(T[t]["kf"])
            boxes[t], tcls[t] = track_box(T[t]["kf"]), T[t]["cls"]
        # 2. classes of detections
        ok = [usable(r) for r in rows]
        high = [d for d in range(n) if ok[d] and F32(rows[d][4]) > F32(p.high)]
        low = [d for d in range(n) if ok[d] and F32(p.low) < F32(rows[d][4]) <= F32(p.high)]
        matched = {}                  # slot -> row
        taken = set()

        def run(tracks, dets, thr, fuse):
            acc = associate(tracks, dets, boxes, tcls, rows, thr, fuse, p.agnostic, entry["assoc"])
            for t, d in acc:
                matched[t] = d; taken.add(d)

        start = {t: int(T[t]["state"]) for t in boxes}
        # 3. first association
        run([t for t in boxes if start[t] in (TRACKED, LOST)], high, p.sim1, p.fuse_score)
        # 4. second association
        run([t for t in boxes if start[t] == TRACKED and t not in matched], low, p.sim2, 0)
        # 6. third association (5. below: it touches only the states)
        run([t for t in boxes if start[t] == NEW], [d for d in high if d not in taken], p.sim3, p.fuse_score)
        for t in boxes:
            if t in matched:
                d = matched[t]
                T[t]["kf"] = update(T[t]["kf"], measure(rows[d]))
                T[t]["state"], T[t]["score"], T[t]["cls"], T[t]["last_frame"] = TRACKED, rows[d][4], rows[d][5], frame
            elif start[t] == TRACKED:
                T[t]["state"] = LOST; entry["lost"].append(t)
            elif start[t] == NEW:
                T[t]["state"] = FREE; entry["freed_new"].append(t)
        # 7. create
        free = [t for t in range(self.cap) if int(T[t]["state"]) == FREE]
        for d in high:
            if d in taken or not F32(rows[d][4]) >= F32(p.new):
                continue
            if not free:
                self.header["dropped"] += 1
                continue
            t = free.pop(0)
            T[t]["kf"] = initiate(measure(rows[d]))
            T[t]["state"] = TRACKED if frame == 1 else NEW
            T[t]["id"] = self.header["next_id"]
            self.header["next_id"] += 1
            T[t]["start_frame"] = T[t]["last_frame"] = frame
            T[t]["score"], T[t]["cls"] = rows[d][4], rows[d][5]
            matched[t] = d
            entry["created"].append(t)
        # 8. remove
        for t in range(self.cap):
            if int(T[t]["state"]) == LOST and frame - int(T[t]["last_frame"]) > p.max_lost:
                T[t]["state"] = FREE; entry["removed"].append(t)
        # 9. output
        out, ids = [], []
        for t in range(self.cap):
            if int(T[t]["state"]) == TRACKED:
                out.append(track_box(T[t]["kf"]) + [T[t]["score"], T[t]["cls"]])
                ids.append([int(T[t]["id"]), matched[t]])
        self.log.append(entry)
        return np.asarray(out, F32).reshape(-1, 6), np.asarray(ids, np.int32).reshape(-1, 2)


class Run(NamedTuple):
    outs: list                        # per frame [k, 6] float32
    ids: list                         # per frame [k, 2] int32
    states: list                      # per frame: the state's bytes
    log: list
    tracker: RefTracker


def run_ref(frames, p: Params, cap: int) -> Run:
    trk = RefTracker(cap, p)
    outs, ids, states = [], [], []
    for rows in frames:
        o, i = trk.step(rows)
        outs.append(o); ids.append(i); states.append(trk.state_bytes())
    return Run(outs, ids, states, trk.log, trk)


# ------------------------------------------------------------------------------------------------ the matrix form
class MatrixFilter:
    """ByteTrack's KalmanFilter (8 states: cx, cy, a, h and their velocities) in fp64 with full matrices"""

    def __init__(self, z):
        wp, wv = float(WP), float(WV)
        self.wp, self.wv = wp, wv
        h = float(z[3])
        self.F = np.eye(8); self.F[:4, 4:] = np.eye(4)
        self.H = np.eye(4, 8)
        self.mean = np.concatenate([np.asarray(z, np.float64), np.zeros(4)])
        std = [float(F32(0.1)) * h, float(F32(0.1)) * h, float(F32(1e-2)), float(F32(0.1)) * h,
               float(F32(0.0625)) * h, float(F32(0.0625)) * h, float(F32(1e-5)), float(F32(0.0625)) * h]
        self.cov = np.diag(np.square(std))

    def predict(self):
        h = self.mean[3]
        std = [self.wp * h, self.wp * h, float(F32(1e-2)), self.wp * h, self.wv * h, self.wv * h, float(F32(1e-5)), self.wv * h]
        self.mean = self.F @ self.mean
        self.cov = self.F @ self.cov @ self.F.T + np.diag(np.square(std))

    def update(self, z):
        h = self.mean[3]
        R = np.diag(np.square([self.wp * h, self.wp * h, float(F32(1e-1)), self.wp * h]))
        S = self.H @ self.cov @ self.H.T + R
        K = self.cov @ self.H.T @ np.linalg.inv(S)
        self.mean = self.mean + K @ (np.asarray(z, np.float64) - self.H @ self.mean)
        self.cov = self.cov - K @ S @ K.T

    def blocks(self):
        """-> (p [4], v [4], Ppp [4], Ppv [4], Pvv [4]) and the largest |entry| outside the four 2 x 2 blocks"""
        c = self.cov
        idx = np.arange(4)
        mask = np.ones((8, 8), bool)
        mask[idx, idx] = mask[idx + 4, idx + 4] = mask[idx, idx + 4] = mask[idx + 4, idx] = False
        return (self.mean[:4], self.mean[4:], c[idx, idx], c[idx, idx + 4], c[idx + 4, idx + 4]), float(np.abs(c[mask]).max())


def filter_track(rng, frames=60):
    """one random track: boxes up to 4000 px, h from 8 to 800, 20 % missed frames -> [(z or None)] per frame"""
    h = float(np.exp(rng.uniform(np.log(8.0), np.log(800.0))))
    a = float(rng.uniform(0.3, 2.5))
    cx, cy = rng.uniform(0.0, 4000.0, 2)
    vx, vy = rng.uniform(-0.2, 0.2, 2) * h
    zs = []
    for f in range(frames):
        cx, cy = cx + vx, cy + vy
        h *= float(rng.uniform(0.98, 1.02))
        w = a * h * float(rng.uniform(0.97, 1.03))
        row = np.asarray([cx - w / 2 + rng.normal(0, 0.02 * h), cy - h / 2 + rng.normal(0, 0.02 * h),
                          cx + w / 2 + rng.normal(0, 0.02 * h), cy + h / 2 + rng.normal(0, 0.02 * h), 0.9, 0.0], F32)
        zs.append(None if (f > 0 and rng.random() < 0.2) else measure(row))
    return zs


def filter_errors(zs):
    """both forms over one track -> (worst |mean error| / h, worst relative covariance error, worst off-block |entry|)"""
    kf = initiate(zs[0])
    mf = MatrixFilter([float(v) for v in zs[0]])
    worst_m = worst_c = worst_off = 0.0
    missed = False
    with np.errstate(all="ignore"):
        for z in zs[1:]:
            if missed:                # (a lost track's height velocity is zeroed before the predict)
                kf[3][1] = 0; mf.mean[7] = 0.0
            kf = predict(kf); mf.predict()
            missed = z is None
            if not missed:
                kf = update(kf, z); mf.update([float(v) for v in z])
            (p, v, ppp, ppv, pvv), off = mf.blocks()
            h = abs(p[3])
            worst_off = max(worst_off, off)
            for c in range(4):
                worst_m = max(worst_m, abs(float(kf[c][0]) - p[c]) / h, abs(float(kf[c][1]) - v[c]) / h)
                for got, want in ((kf[c][2], ppp[c]), (kf[c][3], ppv[c]), (kf[c][4], pvv[c])):
                    worst_c = max(worst_c, abs(float(got) - want) / abs(want) if want != 0 else (0.0 if float(got) == 0 else np.inf))
    return worst_m, worst_c, worst_off


# ------------------------------------------------------------------------------------------------ scenarios
def box(cx, cy, w, h, score=0.9, cls=0.0):
    return [cx - w / 2.0, cy - h / 2.0, cx + w / 2.0, cy + h / 2.0, score, cls]


class Scenario(NamedTuple):
    frames: List[np.ndarray]          # per frame [n, 6] float32
    params: Params
    cap: int
    check: Callable[[Run], None]      # asserts that the case reaches what it was built for


def _frames(*lists):
    return [np.asarray(rows, F32).reshape(-1, 6) for rows in lists]


def _ids(run, f):
    return run.ids[f][:, 0].tolist()


def _birth():
    A, B, C = box(100, 100, 40, 80), box(300, 120, 50, 90), box(500, 300, 60, 60)

    def check(run):
        assert [len(o) for o in run.outs] == [2, 2, 3], [len(o) for o in run.outs]      # frame-1 tracks at once, C after its second match
        assert _ids(run, 0) == [1, 2] and _ids(run, 2) == [1, 2, 3]
        assert run.log[1]["created"] == [2] and run.log[2]["assoc"][2]["matches"] == [(2, 2)]
    return Scenario(_frames([A, B], [A, B, C], [A, B, C]), params(), 64, check)


def _new_freed_reuse():
    A, B, C = box(100, 100, 40, 80), box(300, 120, 50, 90), box(500, 300, 60, 60)

    def check(run):
        assert run.log[2]["freed_new"] == [1] and run.log[2]["created"] == [1]          # freed and reused in the same frame
        assert int(run.tracker.tracks[1]["id"]) == 3 and int(run.tracker.tracks[1]["state"]) == NEW
    return Scenario(_frames([A], [A, B], [A, C]), params(), 64, check)


def _cross():
    frames = []
    for f in range(12):
        frames.append([box(100 + 11 * f, 200, 40, 80, 0.9), box(221 - 11 * f, 206, 40, 80, 0.85)])

    def check(run):
        assert all(_ids(run, f) == [1, 2] for f in range(12))
        # while they overlap a track has more than one admissible detection, and at least once the greedy result is not
        # what every track would have picked for itself
        assert any(len(e["assoc"][0]["pairs"]) > 2 for e in run.log)
    return Scenario(_frames(*frames), params(match_thresh=0.9), 64, check)


def _greedy_not_first_choice():
    # T0 and T1 both prefer row 0; T0 has the larger sim and takes it, T1 gets row 1, its second choice
    f1 = [box(100, 100, 40, 80), box(124, 100, 40, 80)]
    f2 = [box(110, 100, 40, 80), box(150, 100, 40, 80)]

    def check(run):
        a = run.log[1]["assoc"][0]
        first = {}
        for t, d, s in a["pairs"]:
            first.setdefault(t, d)
        assert first[0] == 0 and first[1] == 0, first
        assert a["matches"] == [(0, 0), (1, 1)], a["matches"]
    return Scenario(_frames(f1, f2), params(match_thresh=0.95), 64, check)


def _gap():
    A, B, K = box(100, 100, 40, 80), box(300, 120, 50, 90), box(500, 300, 60, 60)
    L = 3                             # max_lost: A is away for L frames, B for L + 1
    frames = [[A, B, K]] * 3 + [[K]] * L + [[A, K]] + [[A, B, K]] * 2

    def check(run):
        fa = 3 + L                    # the frame (0-based) at which A is back
        assert 1 in _ids(run, fa) and 1 not in _ids(run, fa - 1)                         # A returns with its id
        assert int(run.tracker.tracks[0]["start_frame"]) == 1
        assert run.log[fa]["removed"] == [1]                                             # B was removed one frame before it returns
        assert sorted(_ids(run, fa + 2)) == [1, 3, 4] and int(run.tracker.tracks[1]["id"]) == 4
    return Scenario(_frames(*frames), params(track_buffer=L), 64, check)


def _low():
    A, B = box(100, 100, 40, 80), box(300, 120, 50, 90)
    Al, Bl, Cl = box(100, 100, 40, 80, 0.3), box(300, 120, 50, 90, 0.3), box(500, 300, 60, 60, 0.3)
    frames = [[A, B], [A, B], [Al, Cl], [Al, Bl, Cl]]

    def check(run):
        assert run.log[2]["assoc"][1]["matches"] == [(0, 0)] and run.log[3]["assoc"][1]["matches"] == [(0, 0)]    # step 4 carries A
        assert run.log[2]["lost"] == [1] and int(run.tracker.tracks[1]["state"]) == LOST                          # B is not revived
        assert int(run.tracker.header["next_id"]) == 3 and _ids(run, 3) == [1]                                    # and C never starts
    return Scenario(_frames(*frames), params(), 64, check)


def _fuse(fuse):
    # row 0 overlaps the track more, row 1 has the higher score: IoU alone picks row 0, IoU * score row 1
    f1 = [box(100, 100, 40, 80, 0.995)]
    f2 = [box(102, 100, 40, 80, 0.55), box(107, 100, 40, 80, 0.95)]

    def check(run):
        (t, d0, s0), (_, d1, s1) = run.log[1]["assoc"][0]["pairs"]
        assert (d0, d1) == ((1, 0) if fuse else (0, 1)) and s0 > s1
        assert run.ids[1].tolist() == [[1, 1 if fuse else 0]]
    return Scenario(_frames(f1, f2), params(fuse_score=fuse, new_thresh=0.99), 64, check)


def _ties():
    A, A1 = box(100, 100, 40, 80), box(100, 100, 40, 80, 0.995)

    def check(run):
        a = run.log[1]["assoc"][0]
        assert len(a["pairs"]) == 4 and len({s for _, _, s in a["pairs"]}) == 1          # four equal sims
        assert a["matches"] == [(0, 0), (1, 1)]                                          # by slot, then row
        assert run.log[2]["assoc"][0]["matches"] == [(0, 0)] and run.log[2]["lost"] == [1]   # one row, two equal tracks: the lower slot
        assert run.log[3]["assoc"][0]["matches"] == [(0, 0)]                             # one track, two equal rows: the lower row
    return Scenario(_frames([A1, A1], [A, A], [A], [A, A]), params(new_thresh=0.99, track_buffer=0), 64, check)


def _threshold(at):
    f1 = [box(100, 100, 40, 80)]
    f2 = [box(113, 104, 40, 80)]
    probe = run_ref(_frames(f1, f2), params(fuse_score=False, match_thresh=0.99), 64)
    (_, _, sim), = probe.log[1]["assoc"][0]["pairs"]
    thr = F32(sim) if at else np.nextafter(F32(sim), F32(0))
    assert 0.2 < float(thr) < 0.8

    def check(run):
        assert run.log[1]["assoc"][0]["matches"] == ([] if at else [(0, 0)])             # strict: a sim AT the threshold is no match
        assert (run.log[1]["lost"] == [0]) == bool(at)
    return Scenario(_frames(f1, f2), params(fuse_score=False, sim1=float(thr)), 64, check)


def _classes(agnostic):
    f1 = [box(100, 100, 40, 80, 0.9, 2.0)]
    f2 = [box(101, 100, 40, 80, 0.9, 5.0)]

    def check(run):
        assert run.log[1]["assoc"][0]["matches"] == ([(0, 0)] if agnostic else [])
        assert int(run.tracker.header["next_id"]) == (2 if agnostic else 3)
        if agnostic:
            assert float(run.tracker.tracks[0]["cls"]) == 5.0                             # the class follows the detection
    return Scenario(_frames(f1, f2), params(agnostic=agnostic), 64, check)


def _degenerate():
    nan = float("nan")
    A = box(100, 100, 40, 80)
    bad = [[50, 50, 50, 90, 0.9, 0], [60, 60, 90, 40, 0.9, 0], [200, 200, 240, 280, nan, 0], [nan, 10, 40, 80, 0.9, 0],
           [10, 10, 40, nan, 0.9, 0]]
    frames = [bad[:2] + [A] + bad[2:], [bad[3], A, bad[0], [98, 98, 142, 142, nan, 0]]]

    def check(run):
        assert int(run.tracker.header["next_id"]) == 2 and int(run.tracker.header["dropped"]) == 0
        assert run.ids[0].tolist() == [[1, 2]] and run.ids[1].tolist() == [[1, 1]]
        assert np.isfinite(run.outs[1]).all()
    return Scenario(_frames(*frames), params(), 64, check)


def _overflow():
    rows = [box(30 + 60 * (i % 10), 30 + 60 * (i // 10), 40, 40, 0.9, float(i % 3)) for i in range(70)]

    def check(run):
        assert int(run.tracker.header["dropped"]) == 6 and int(run.tracker.header["next_id"]) == 65
        assert len(run.outs[0]) == 64
    return Scenario(_frames(rows), params(), 64, check)


def _drain():
    rows = [box(100, 100, 40, 80), box(300, 120, 50, 90), box(500, 300, 60, 60)]
    frames = [rows, rows] + [[]] * 5

    def check(run):
        assert (run.tracker.tracks["state"] == FREE).all() and int(run.tracker.header["frame"]) == 7
        assert run.log[5]["removed"] == [0, 1, 2] and [len(o) for o in run.outs] == [3, 3, 0, 0, 0, 0, 0]
    return Scenario(_frames(*frames), params(track_buffer=3), 64, check)


SCENARIOS = {
    "birth": _birth, "new_freed_reuse": _new_freed_reuse, "cross": _cross, "greedy_not_first_choice": _greedy_not_first_choice,
    "gap": _gap, "low": _low, "fuse_on": lambda: _fuse(True), "fuse_off": lambda: _fuse(False), "ties": _ties,
    "threshold_at": lambda: _threshold(True), "threshold_below": lambda: _threshold(False),
    "class_agnostic": lambda: _classes(True), "class_aware": lambda: _classes(False), "degenerate": _degenerate,
    "overflow": _overflow, "drain": _drain,
}


@functools.lru_cache(maxsize=None)
def scenario(name) -> Scenario:
    return SCENARIOS[name]()


@functools.lru_cache(maxsize=None)
def scenario_run(name) -> Run:
    s = scenario(name)
    return run_ref(s.frames, s.params, s.cap)


@functools.lru_cache(maxsize=None)
def random_frames(seed=7, objects=20, frames=40):
    """20 objects on slow straight paths with jitter, a tenth of the detections missed, scores on both sides of the
    thresholds, up to three false positives per frame"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(60, 900, (objects, 2))
    vel = rng.uniform(-6, 6, (objects, 2))
    size = rng.uniform(30, 90, (objects, 2))
    cls = rng.integers(0, 3, objects)
    first = [0] * objects
    last = [frames] * objects
    first[:3], last[3:7] = (8, 14, 20), (10, 16, 22, 28)     # three objects enter late, four leave for good
    out = []
    for f in range(frames):
        pos = pos + vel
        rows = []
        for o in range(objects):
            if rng.random() < 0.1 or not first[o] <= f < last[o]:
                continue
            j = rng.normal(0, 1.5, 4)
            score = float(rng.choice([rng.uniform(0.6, 0.95), rng.uniform(0.15, 0.5)], p=[0.8, 0.2]))
            rows.append(box(pos[o, 0] + j[0], pos[o, 1] + j[1], size[o, 0] + j[2], size[o, 1] + j[3], score, float(cls[o])))
        for _ in range(int(rng.integers(0, 4))):
            rows.append(box(*rng.uniform(60, 900, 2), *rng.uniform(20, 80, 2), float(rng.uniform(0.12, 0.8)), float(rng.integers(0, 3))))
        order = rng.permutation(len(rows))
        out.append(np.asarray(rows, F32).reshape(-1, 6)[order])
    return out


RANDOM_PARAMS = dict(agnostic=False, track_buffer=5)


@functools.lru_cache(maxsize=None)
def random_run(cap=64) -> Run:
    return run_ref(random_frames(), params(**RANDOM_PARAMS), cap)
