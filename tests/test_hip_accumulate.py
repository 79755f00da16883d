"""Gradient accumulation on the device: kodhip_grad_accumulate (csrc/accumulate.hip) through the C ABI on the test's own guarded
buffers, GraphedTrainStep / MultiScaleTrainStep(accumulate_grad_batches=N) and DefaultYolov5Experiment(accumulate_grad_batches=N).

Everything is compared bit for bit (int32 / uint32 views):
* the kernel against the numpy reference of tests/accumulate_reference.py - modes 0, 1 and 2 with the flag 0 and non-zero, sizes
  around the 4-element quad and the 4096-element block chunk, bases off the 16-byte boundary on either side; canaries and the
  whole gradient side must be unchanged; every refused call leaves both buffers as they were;
* a captured step with N = 3 over 7 batches (two full windows and a flushed partial one), SGD and AdamW, with and without
  clipping, against a comparator that never accumulates through `.grad`: per micro-batch one train_step at the scale B / 3 and a
  snapshot of the gradient arena, the snapshots summed by the numpy reference, the sum copied into the gradient arena, opt.step();
* N = 1 against the plain captured step; the experiment's eager and graphed routes against each other and the comparator;
  multi-scale with a size first met inside a window; the guards.

yv5n width, nc 3, B = 2, 64 px; per image a small, a medium and a large box so that every pyramid level gets a match.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import accumulate_reference as R  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.data.detection import DetectionTarget  # noqa: E402

GUARD = 64                                   # canary elements on both sides of a buffer (a multiple of 4: 16 bytes)
CANARY = 0x5A5A5A5A
NC, B, S, CAP, STEPS, N = 3, 2, 64, 64, 7, 3
WINDOWS = [(0, 3), (3, 6), (6, 7)]           # 7 batches, N = 3: two full windows and the partial one flush() closes
CLIP = 0.1


# ------------------------------------------------------------------------------------------------------------- the kernel
class _Buf:
    """n values on the device inside a canary-filled buffer: [GUARD canaries | off canaries | n values | GUARD canaries]"""

    def __init__(self, values, off):
        self.n, self.off = len(values), off
        host = np.full(self.n + 2 * GUARD + off, CANARY, dtype=np.uint32)
        host[GUARD + off:GUARD + off + self.n] = np.asarray(values, dtype=np.float32).view(np.uint32)
        self.buf = torch.from_numpy(host.view(np.int32).copy()).cuda()
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr() + 4 * (GUARD + self.off)

    def words(self):
        return self.buf.cpu().numpy().view(np.uint32)

    def values(self):
        return self.words()[GUARD + self.off:GUARD + self.off + self.n]

    def canaries_intact(self):
        w = self.words()
        return bool((w[:GUARD + self.off] == CANARY).all() and (w[GUARD + self.off + self.n:] == CANARY).all())


MODES = [(0, None), (1, None), (2, 0.0), (2, 1.0), (2, -3.5)]      # (mode, ctl[0]); the copy is mode 1 and mode 2 with ctl[0] != 0


@pytest.mark.parametrize("mode,flag", MODES, ids=["add", "copy", "ctl_add", "ctl_copy", "ctl_copy_neg"])
@pytest.mark.parametrize("offsets", R.OFFSETS)
@pytest.mark.parametrize("n", R.SIZES)
def test_kernel_bits(n, offsets, mode, flag):
    a, g = R.values(n, seed=n + 7)
    acc, grad = _Buf(a, offsets[0]), _Buf(g, offsets[1])
    ctl = None if flag is None else torch.tensor([flag, 7.0, 7.0, 7.0], dtype=torch.float32).cuda()
    first = mode == 1 or (mode == 2 and flag != 0.0)
    want = R.accumulate_ref(a, g, first)
    rc = _lib.lib().kodhip_grad_accumulate(acc.ptr(), grad.ptr(), n, mode, None if ctl is None else ctl.data_ptr(), stream())
    _lib.check(rc, "grad_accumulate")
    torch.cuda.synchronize()
    got = acc.values().view(np.float32)
    differ = int(((R.bits(got) != R.bits(want)) & ~(np.isnan(got) & np.isnan(want))).sum())
    print(f"grad_accumulate n {n} offsets {offsets} mode {mode} flag {flag}: {differ} of {n} values differ")
    assert acc.canaries_intact() and grad.canaries_intact(), "wrote outside the buffers"
    np.testing.assert_array_equal(grad.values(), R.bits(g))                          # the gradient side is read only
    assert np.array_equal(np.isnan(got), np.isnan(want))
    if first:
        np.testing.assert_array_equal(R.bits(got), R.bits(g))                        # a copy: all 32 bits, NaN payloads included
    else:
        assert R.same_bits_or_both_nan(got, want)
    if ctl is not None:
        assert ctl.cpu().tolist() == [flag, 7.0, 7.0, 7.0]                           # the flag is only read


def test_kernel_running_sum():
    """three launches through one control block, as a window of a captured step does: copy, add, add"""
    n = 8193
    gs = [R.mixed(n, 40 + k) for k in range(3)]
    acc = _Buf(R.mixed(n, 39), 0)
    ctl = torch.zeros(4, dtype=torch.float32).cuda()
    want = None
    for k, g in enumerate(gs):
        ctl[0] = 1.0 if k == 0 else 0.0
        grad = _Buf(g, 0)
        _lib.check(_lib.lib().kodhip_grad_accumulate(acc.ptr(), grad.ptr(), n, 2, ctl.data_ptr(), stream()), "grad_accumulate")
        want = R.accumulate_ref(want, g, k == 0)
    torch.cuda.synchronize()
    assert acc.canaries_intact()
    assert R.same_bits_or_both_nan(acc.values().view(np.float32), want)


def test_error_returns_leave_the_buffers_untouched():
    lib = _lib.lib()
    a, g = R.values(1023, 3)
    acc, grad = _Buf(a, 0), _Buf(g, 0)
    ctl = torch.ones(4, dtype=torch.float32).cuda()
    before = [b.words().copy() for b in (acc, grad)]
    cases = [("negative n", (acc.ptr(), grad.ptr(), -1, 0, None)),
             ("null acc", (None, grad.ptr(), 8, 0, None)),
             ("null grad", (acc.ptr(), None, 8, 1, None)),
             ("mode 3", (acc.ptr(), grad.ptr(), 8, 3, ctl.data_ptr())),
             ("mode -1", (acc.ptr(), grad.ptr(), 8, -1, ctl.data_ptr())),
             ("mode 2 with NULL ctl", (acc.ptr(), grad.ptr(), 8, 2, None)),
             ("acc not 4-byte aligned", (acc.ptr() + 2, grad.ptr(), 8, 0, None)),
             ("grad not 4-byte aligned", (acc.ptr(), grad.ptr() + 1, 8, 1, None)),
             ("acc is grad", (acc.ptr(), acc.ptr(), 1023, 0, None)),
             ("acc begins inside grad", (grad.ptr() + 4 * 1000, grad.ptr(), 1023, 0, None)),
             ("grad begins inside acc", (acc.ptr(), acc.ptr() + 4 * 1022, 1023, 1, None))]
    for what, args in cases:
        rc = lib.kodhip_grad_accumulate(*args, stream())
        msg = lib.kodhip_last_error()
        print(f"grad_accumulate {what}: rc {rc} {msg!r}")
        assert rc < 0 and b"grad_accumulate" in msg, (what, rc)
    assert lib.kodhip_grad_accumulate(None, None, 0, 0, None, stream()) == 0         # n == 0: nothing to do, NULLs allowed
    torch.cuda.synchronize()
    for b, w in zip((acc, grad), before):
        np.testing.assert_array_equal(b.words(), w)


# ------------------------------------------------------------------------------------------------------------ the fixtures
def _net(seed=5):
    from bench import build
    torch.manual_seed(seed)
    return build(NC, torch.device("cuda", 0), seed=seed, widen=0.25)


def _anchors():
    from object_detection_cib_amd.core.anchors.info import voc_anchor_info
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo
    return LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))


def _batch(seed):
    """(images [B, 3, S, S] on the device, one DetectionTarget per image): a small, a medium and a large box (8, 22 and 50 px,
    jittered) for the stride-8, -16 and -32 anchors"""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.random((B, 3, S, S), dtype=np.float32)).cuda()
    tg = []
    for _ in range(B):
        rows = []
        for side in (8.0, 22.0, 50.0):
            wh = side * rng.uniform(0.9, 1.1, 2)
            c = rng.uniform(wh / 2 + 1, S - 1 - wh / 2)
            rows.append(np.concatenate((c - wh / 2, c + wh / 2)))
        tg.append(DetectionTarget(torch.from_numpy(np.stack(rows).astype(np.float64)), torch.from_numpy(rng.integers(0, NC, 3).astype(np.int64))))
    return x, tuple(tg), None


@pytest.fixture(scope="module")
def batches():
    return [_batch(s) for s in range(STEPS)]


def _ibits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


ARENAS = ("p_arena", "m_arena", "rm_arena", "rv_arena", "nbt_arena")


def _arenas(net, adam=False, norm=False):
    torch.cuda.synchronize()
    eng = net.engine()
    out = {n: getattr(eng, n).clone() for n in ARENAS + (("v_arena",) if adam else ())}
    if norm:
        out["grad_norm"] = eng.clip[0:4].clone()
    return out


def _assert_same(got, want, what):
    assert list(got) == list(want), what
    for k, v in want.items():
        same = torch.equal(_ibits(got[k]), _ibits(v))
        if not same:
            print(f"{what}: {k}: {int((_ibits(got[k]) != _ibits(v)).sum())} of {v.numel()} words differ")
        assert same, (what, k)


def _optimizer(net, kind, clip):
    from object_detection_cib_amd.nn.optim.smart import SmartAdamW, SmartSGD
    opt = SmartSGD(net, lr=0.01) if kind == "sgd" else SmartAdamW(net, lr=1e-3)
    opt.gradient_clip_val, opt.track_grad_norm = clip, True
    return opt


def _comparator_window(net, loss, opt, window):
    """one window without `.grad` accumulation: per micro-batch a train_step at B / N and a snapshot of the gradient arena; the
    numpy sum of the snapshots goes into the gradient arena that opt.step() reads"""
    eng = net.engine()
    acc = None
    for k, (x, tg, _) in enumerate(window):
        for p in net.parameters():
            p.grad = None
        net.train_step(x, loss, FeatureShape(width=S, height=S), tg, B / N)
        eng.wait_grads()
        torch.cuda.synchronize()
        acc = R.accumulate_ref(acc, eng.current_grad_arena().cpu().numpy(), k == 0)
    assert np.isfinite(acc).all() and np.abs(acc).max() > 0
    eng.current_grad_arena().copy_(torch.from_numpy(acc))
    opt.step()


class _HandRun:
    """7 batches, N = 3, driven by hand: the comparator (graphed=False) or GraphedTrainStep(accumulate_grad_batches=3)"""

    def __init__(self, graphed, kind, clip, batches):
        from object_detection_cib_amd.engine.graphed import GraphedTrainStep
        self.net, self.loss = _net()
        net, eng = self.net, self.net.engine()
        opt = _optimizer(net, kind, clip)
        adam = kind == "adam"
        self.snaps, self.stepped, self.coefs = [], [], []
        if not graphed:
            for lo, hi in WINDOWS:
                _comparator_window(net, self.loss, opt, batches[lo:hi])
                self.snaps.append(_arenas(net, adam, True))
                self.coefs.append(float(eng.clip[4]))
            return
        initial = _arenas(net)
        step = GraphedTrainStep(net, self.loss, B, S, S, CAP, gradient_clip_val=clip, track_grad_norm=True, optimizer=kind,
                                accumulate_grad_batches=N)
        assert step.scale == B / N
        step.capture(batches[0][0], batches[0][1], adam=opt.hyper() if adam else None)
        _assert_same(_arenas(net), initial, "capture() moved the state")
        assert eng.acc_arena is not None and eng.acc_arena.numel() == eng.p_arena.numel() and eng.accumulation.n == N
        assert not eng.accumulation.flush_needed
        self.step = step

        def hyper():
            return dict(adam=opt.hyper()) if adam else dict(zip(("lr", "momentum", "weight_decay"), opt.hyper()))

        def after():
            self.stepped.append(step.stepped)
            if step.stepped:
                opt.steps_taken += 1
                self.snaps.append(_arenas(net, adam, True))
        versions = []
        for x, tg, _ in batches:
            before = eng.freshness_key()
            step(x, tg, **hyper())
            versions.append((before, eng.freshness_key()))
            after()
        self.versions = versions
        assert eng.accumulation.flush_needed
        assert step.flush(**hyper()) is True
        after()
        assert step.flush(**hyper()) is False and step.stepped is False


@pytest.fixture(scope="module")
def hand(batches):
    cache = {}

    def get(graphed, kind, clip):
        key = (graphed, kind, clip)
        if key not in cache:
            cache[key] = _HandRun(graphed, kind, clip, batches)
        return cache[key]
    return get


@pytest.mark.parametrize("clip", [None, CLIP], ids=["noclip", "clip"])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_window_equals_the_comparator(hand, kind, clip):
    want, got = hand(False, kind, clip), hand(True, kind, clip)
    assert got.stepped == [False, False, True, False, False, True, False, True]      # calls 3, 6 and the flush
    assert len(got.snaps) == len(want.snaps) == 3
    print(f"{kind} clip {clip}: comparator clip coefficients {want.coefs}, grad norms "
          f"{[float(s['grad_norm'][0]) for s in want.snaps]}")
    if clip is not None:
        assert all(c < 1.0 for c in want.coefs), "the clip value never bites: nothing is tested"
    for w, (g, c) in enumerate(zip(got.snaps, want.snaps)):
        _assert_same(g, c, f"{kind} clip {clip} window {w}")
    moved = int((_ibits(want.snaps[0]["p_arena"]) != _ibits(want.snaps[2]["p_arena"])).sum())
    assert moved > 0
    # a non-closing replay moved running statistics and no parameter; a closing one moved both
    for (b, a), stepped in zip(got.versions, got.stepped):
        assert a[1] > b[1] and (a[0] > b[0]) == stepped, (b, a, stepped)


def test_eval_constants_follow_a_non_closing_replay(hand, batches):
    """after a micro-batch that moved only running statistics the eval forward must see them (engine/freshness.py)"""
    from object_detection_cib_amd.engine.graphed import GraphedTrainStep
    net, loss = _net(9)
    step = GraphedTrainStep(net, loss, B, S, S, CAP, accumulate_grad_batches=N).capture(batches[0][0], batches[0][1])
    x = batches[0][0]

    def eval_forward(m):
        m.eval()
        with torch.no_grad():
            out = [o.clone() for o in m.forward_raw(x)]
        m.train()
        return out
    eval_forward(net)                                   # (the constants exist and are fresh before the replay)
    step(x, batches[0][1], (0.01,) * 3, (0.9,) * 3, (0.0, 5e-4, 0.0))
    assert step.stepped is False
    twin, _ = _net(10)
    twin.load_state_dict(net.state_dict())
    got, want = eval_forward(net), eval_forward(twin)
    assert all(torch.equal(_ibits(a), _ibits(b)) for a, b in zip(got, want))
    net.engine().accumulation.reset()


# ------------------------------------------------------------------------------------------------------------------ N = 1
def test_accumulate_1_is_the_plain_step(batches):
    from object_detection_cib_amd.engine.graphed import GraphedTrainStep
    runs = []
    for kw in ({}, {"accumulate_grad_batches": 1}):
        net, loss = _net()
        eng = net.engine()
        step = GraphedTrainStep(net, loss, B, S, S, CAP, track_grad_norm=True, **kw).capture(batches[0][0], batches[0][1])
        assert step.scale == float(B)
        snaps = []
        for x, tg, _ in batches[:4]:
            total, _ = step(x, tg, (0.01,) * 3, (0.9,) * 3, (0.0, 5e-4, 0.0))
            assert step.stepped is True
            snaps.append(dict(_arenas(net, norm=True), total=total.clone()))
        assert eng.acc_arena is None and eng.acc_ctl is None and eng.accumulation is None
        assert step.flush() is False
        runs.append(snaps)
    for k, (a, b) in enumerate(zip(*runs)):
        _assert_same(b, a, f"step {k}")


# -------------------------------------------------------------------------------------------------------------- experiment
def _experiment(graphed, seed=5, **kw):
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.warmup import OptimizerWarmupUpdater
    net, loss = _net(seed)
    return DefaultYolov5Experiment(net, loss, _anchors(), optimizer_warmup_updater=OptimizerWarmupUpdater(3, 0.1, 0.8, 0.937),
                                   max_epochs=4, graphed=graphed, max_targets=CAP, **kw)


@pytest.fixture(scope="module")
def exp_runs(batches):
    out = {}
    for graphed in (False, True):
        exp = _experiment(graphed, ema=True, accumulate_grad_batches=N)
        losses = exp.fit_epoch(batches)
        out[graphed] = (exp, losses.cpu(), _arenas(exp.net))
    return out


def test_experiment_routes_agree(exp_runs):
    (eager, l0, a0), (graphed, l1, a1) = exp_runs[False], exp_runs[True]
    for exp in (eager, graphed):
        assert exp.global_step == 3 and exp.optimizer.steps_taken == 3 and exp.ema.updates == 3 and exp.current_epoch == 1
    print(f"fit_epoch N = {N}: eager losses {l0.tolist()} graphed {l1.tolist()}")
    assert torch.isfinite(l0).all() and torch.equal(_ibits(l0), _ibits(l1))          # the scaled totals, (B / N) * (...)
    _assert_same(a1, a0, "graphed against eager")
    for k in ("p", "rm", "rv", "nbt"):
        assert torch.equal(_ibits(graphed.ema._shadow[k]), _ibits(eager.ema._shadow[k])), k
    assert not eager._window.flush_needed and not graphed.net.engine().accumulation.flush_needed
    assert eager.step_accumulated() is False and graphed.step_accumulated() is False
    assert eager.global_step == 3 and graphed.global_step == 3


def test_experiment_equals_the_comparator(exp_runs, batches):
    """the hand-driven comparator with the experiment's own hyper sequence (warm-up hook before every optimizer step)"""
    ref = _experiment(False, accumulate_grad_batches=N)
    ref.configure_optimizers()
    for lo, hi in WINDOWS:
        ref._warmup(STEPS)
        _comparator_window(ref.net, ref.loss, ref.optimizer, batches[lo:hi])
        ref.global_step += 1
    want = _arenas(ref.net)
    for graphed in (False, True):
        _assert_same(exp_runs[graphed][2], want, f"experiment graphed={graphed} against the comparator")


def test_the_scaled_total_is_one_product(exp_runs, batches):
    """`total` is (B / N) * (...) in fp32, not (B * (...)) / N"""
    exp = _experiment(False, seed=5, accumulate_grad_batches=N)
    plain = _experiment(False, seed=5)
    t3, t1 = exp.training_step(batches[0]), plain.training_step(batches[0])
    s = (exp.logged["box"] + exp.logged["cls"]) + exp.logged["obj"]
    assert torch.equal(_ibits(t3), _ibits((B / N) * s)) and torch.equal(_ibits(t1), _ibits(B * s))
    assert torch.equal(_ibits(exp_runs[False][1][0]), _ibits(t3.cpu()))


# ------------------------------------------------------------------------------------------------------------- multi-scale
def _ms_seed():
    """a schedule seed whose draws begin 64, 96: the second size is first met as the second micro-batch of a window"""
    from object_detection_cib_amd.engine.multiscale import MultiScaleSchedule
    for seed in range(200):
        sch = MultiScaleSchedule(S, S, seed, gs=32, interval=1, sizes=[64, 96])
        if [sch.next() for _ in range(2)] == [(64, 64), (96, 96)]:
            return seed
    raise AssertionError("no seed draws 64, 96")


def test_multiscale_size_first_met_inside_a_window(batches):
    from object_detection_cib_amd.engine.multiscale import MultiScaleTrainStep
    seed = _ms_seed()
    hyper = ((0.01,) * 3, (0.9,) * 3, (0.0, 5e-4, 0.0))
    results = []
    for precapture in (False, True):
        net, loss = _net()
        eng = net.engine()
        ms = MultiScaleTrainStep(net, loss, B, S, S, CAP, sizes=[64, 96], interval=1, seed=seed, accumulate_grad_batches=2)
        if precapture:
            # both sizes met, and captured, before the compared windows start: one window, then everything back to the start
            initial = _arenas(net)
            for x, tg, _ in batches[:2]:
                ms(x, tg, *hyper)
            assert ms.captures == 2 and ms.stepped
            torch.cuda.synchronize()
            with torch.no_grad():
                for k, v in initial.items():
                    getattr(eng, k).copy_(v)
            eng.invalidate_eval_constants()
            eng.sgd_steps = 0
            ms.load_state_dict({"seed": seed, "draws": 0, "steps": 0})
        snaps, sizes, captures, stepped = [], [], [], []
        for x, tg, _ in batches[:4]:
            ms(x, tg, *hyper)
            sizes.append(ms.size)
            captures.append(ms.captures)
            stepped.append(ms.stepped)
            if ms.stepped:
                snaps.append(_arenas(net))
        assert sizes[:2] == [(64, 64), (96, 96)] and stepped == [False, True, False, True]
        assert captures == ([2] * 4 if precapture else [1, 2, 2, 2]), captures
        assert ms.flush() is False
        results.append(snaps)
    for w, (a, b) in enumerate(zip(*results)):
        _assert_same(a, b, f"multi-scale window {w}: captured inside the window against captured before")


# ------------------------------------------------------------------------------------------------------------------ guards
class _CountingLib:
    """the ABI handle with every call counted (what reaches the library launches or refuses; nothing else launches)"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted


def test_guards(hand, exp_runs, batches):
    run = hand(True, "sgd", None)
    step, eng = run.step, run.net.engine()
    hyper = ((0.01,) * 3, (0.9,) * 3, (0.0, 5e-4, 0.0))
    # flush() with nothing open: no ABI call, no upload, nothing moves
    assert not eng.accumulation.flush_needed
    before, key, slot = _arenas(run.net), eng.freshness_key(), (eng._hyper_ring.slot, eng._clip_ring.slot, eng._acc_ring.slot)
    real, eng.lib = eng.lib, _CountingLib(eng.lib)
    try:
        assert step.flush(*hyper) is False
        calls = eng.lib.calls
    finally:
        eng.lib = real
    assert calls == [] and eng.freshness_key() == key
    assert slot == (eng._hyper_ring.slot, eng._clip_ring.slot, eng._acc_ring.slot)
    _assert_same(_arenas(run.net), before, "flush() with nothing open")
    # a changed N after capture
    step.accumulate = 2
    try:
        with pytest.raises(RuntimeError, match=r"capture\(\) again"):
            step(batches[0][0], batches[0][1], *hyper)
    finally:
        step.accumulate = N
    _assert_same(_arenas(run.net), before, "a refused call")
    for bad in (0, 2.5, "2"):
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            _experiment(False, accumulate_grad_batches=bad)
    # optimize() under ema.applied() still raises, on both routes, and moves no counter
    for graphed in (False, True):
        exp = exp_runs[graphed][0]
        counters = (exp.global_step, exp.ema.updates, exp.optimizer.steps_taken)
        with exp.ema.applied():
            with pytest.raises(RuntimeError, match="applied"):
                exp.optimize(batches[0], STEPS)
        assert counters == (exp.global_step, exp.ema.updates, exp.optimizer.steps_taken)
