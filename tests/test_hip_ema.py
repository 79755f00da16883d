"""Weight EMA on the device: kodhip_ema_update / kodhip_ema_swap (csrc/ema.hip) through the C ABI on the test's own guarded
buffers, ModelEMA (engine/ema.py), DefaultYolov5Experiment(ema=True) and the checkpoint key.

Everything is compared bit for bit (uint32 / int32 views, so NaN payloads count):
* the update against the numpy reference of tests/ema_reference.py - one and several segments, odd sizes, sizes around the
  4096-element block chunk, bases off the 16-byte boundary on either side, a zero-length segment in the middle; the canaries
  around every segment and the whole model side must be unchanged;
* the swap against a plain exchange, twice = identity;
* every refused call leaves both buffers as they were;
* ModelEMA after four training steps (eager train_step + FusedSGD, and GraphedTrainStep) against the reference applied to
  snapshots of net.state_dict(); the same seeded experiment with and without ema=True; applied(); a checkpoint resume; validate().

yv5n width, nc 3, B = 2, 64 px; per image a small, a medium and a large box so that every pyramid level gets a match.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ema_reference as R  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.data.detection import DetectionTarget  # noqa: E402

GUARD = 64                                   # canary elements on both sides of every segment (a multiple of 4: 16 bytes)
CANARY = 0x5A5A5A5A
NC, B, S, CAP, STEPS = 3, 2, 64, 64, 4
HYPER = ((0.01, 0.01, 0.01), (0.9, 0.9, 0.9), (0.0, 5e-4, 0.0))
OFFSETS = [(0, 0), (1, 1), (1, 0), (0, 2)]   # (model, shadow) base offsets in elements from a 16-byte boundary
CHUNK_SIZES = (4095, 4096, 4097, 8193)       # around the 4096-element chunk one block owns


# ------------------------------------------------------------------------------------------------------- the two kernels
class _Seg:
    """one segment on the device inside a canary-filled buffer: [GUARD canaries | off canaries | n values | GUARD canaries]"""

    def __init__(self, values, off):
        self.n, self.off = len(values), off
        host = np.full(self.n + 2 * GUARD + off, CANARY, dtype=np.uint32)
        host[GUARD + off:GUARD + off + self.n] = np.asarray(values, dtype=np.float32).view(np.uint32)
        self.host = host
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


def _tables(ms, es, numels=None):
    k = len(ms)
    return ((C.c_void_p * k)(*[s.ptr() if s is not None else None for s in ms]),
            (C.c_void_p * k)(*[s.ptr() if s is not None else None for s in es]),
            (C.c_long * k)(*(numels if numels is not None else [s.n for s in ms])))


def _segments(sizes, offsets, seed):
    ms = [_Seg(R.mixed(n, seed + 11 * i, specials=True), om) for i, (n, (om, _)) in enumerate(zip(sizes, offsets))]
    es = [_Seg(R.mixed(n, seed + 11 * i + 5, specials=True), oe) for i, (n, (_, oe)) in enumerate(zip(sizes, offsets))]
    return ms, es


def _check_update(sizes, offsets, updates, seed):
    ms, es = _segments(sizes, offsets, seed)
    m0 = [s.values().copy() for s in ms]
    want = [s.values().view(np.float32).copy() for s in es]
    for u in updates:
        d = R.decay_ref(u)
        c0, c1 = np.float32(d), np.float32(1.0 - d)
        rc = _lib.lib().kodhip_ema_update(*_tables(ms, es), len(ms), float(c0), float(c1), stream())
        _lib.check(rc, "ema_update")
        want = [R.ema_update_ref(w, m.view(np.float32), d) for w, m in zip(want, m0)]
    torch.cuda.synchronize()
    for k, (m, e) in enumerate(zip(ms, es)):
        diff = int((e.values() != R.bits(want[k])).sum())
        print(f"ema_update sizes {sizes} offsets {offsets} updates {updates}: segment {k}: {diff} of {m.n} values differ")
        assert m.canaries_intact() and e.canaries_intact(), ("wrote outside segment", k)
        np.testing.assert_array_equal(m.values(), m0[k])                              # the model side is read only
        np.testing.assert_array_equal(e.values(), R.bits(want[k]))


@pytest.mark.parametrize("offsets", OFFSETS)
@pytest.mark.parametrize("n", R.SIZES)
def test_update_one_segment_bits(n, offsets):
    _check_update([n], [offsets], R.UPDATES, seed=n)                                  # all six d, applied one after the other


@pytest.mark.parametrize("sizes,offsets", [
    ((65, 1, 1023), [(0, 0)] * 3),
    ((65, 1, 1023), [(1, 1), (0, 0), (3, 2)]),
    ((65, 0, 1023), [(0, 0)] * 3),                                                    # a zero-length segment in the middle
    ((0, 5, 0), [(0, 0)] * 3),
    (CHUNK_SIZES, [(0, 0), (0, 0), (1, 0), (0, 0)]),
    ((70001, 3, 4096, 12289), [(0, 0), (1, 1), (0, 0), (0, 1)]),
])
def test_update_several_segments_bits(sizes, offsets):
    _check_update(list(sizes), offsets, (1, 2000, 10 ** 7), seed=sum(sizes))


def test_update_with_all_segments_empty_launches_nothing():
    ms, es = _segments([0, 0], [(0, 0)] * 2, 1)
    assert _lib.lib().kodhip_ema_update(*_tables(ms, es), 2, 0.5, 0.5, stream()) == 0
    z = (C.c_void_p * 1)(None)
    assert _lib.lib().kodhip_ema_update(z, z, (C.c_long * 1)(0), 1, 0.5, 0.5, stream()) == 0      # null pointers with numel 0
    torch.cuda.synchronize()
    assert all(s.canaries_intact() for s in ms + es)


def _check_swap(sizes, offsets, seed):
    ms, es = _segments(sizes, offsets, seed)
    a0, b0 = [s.values().copy() for s in ms], [s.values().copy() for s in es]
    lib = _lib.lib()
    _lib.check(lib.kodhip_ema_swap(*_tables(ms, es), len(ms), stream()), "ema_swap")
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(ms, es)):
        assert a.canaries_intact() and b.canaries_intact(), ("wrote outside segment", k)
        np.testing.assert_array_equal(a.values(), b0[k])
        np.testing.assert_array_equal(b.values(), a0[k])
    _lib.check(lib.kodhip_ema_swap(*_tables(ms, es), len(ms), stream()), "ema_swap")
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(ms, es)):
        assert a.canaries_intact() and b.canaries_intact()
        np.testing.assert_array_equal(a.values(), a0[k])                              # twice: the identity
        np.testing.assert_array_equal(b.values(), b0[k])


@pytest.mark.parametrize("offsets", OFFSETS)
@pytest.mark.parametrize("n", R.SIZES)
def test_swap_one_segment_bits(n, offsets):
    _check_swap([n], [offsets], seed=n)


@pytest.mark.parametrize("sizes,offsets", [
    ((65, 1, 1023), [(1, 1), (0, 0), (3, 2)]),
    ((65, 0, 1023, 7), [(0, 0)] * 4),
    (CHUNK_SIZES, [(0, 0), (0, 0), (1, 0), (0, 0)]),
    ((70001, 3, 4096, 12289), [(0, 0), (1, 1), (0, 0), (0, 1)]),
])
def test_swap_several_segments_bits(sizes, offsets):
    _check_swap(list(sizes), offsets, seed=sum(sizes))


def test_error_returns_leave_the_buffers_untouched():
    lib = _lib.lib()
    ms, es = _segments([65, 9, 1023, 5, 5], [(0, 0)] * 5, 3)
    before = [s.words().copy() for s in ms + es]

    def both(tm, te, tn, nseg, what):
        for fn, call in (("ema_update", lambda: lib.kodhip_ema_update(tm, te, tn, nseg, 0.5, 0.5, stream())),
                         ("ema_swap", lambda: lib.kodhip_ema_swap(tm, te, tn, nseg, stream()))):
            rc = call()
            msg = lib.kodhip_last_error()
            print(f"{fn} {what}: rc {rc} {msg!r}")
            assert rc < 0 and fn.encode() in msg, (fn, what, rc)

    tm, te, tn = _tables(ms, es)
    both(tm, te, tn, 0, "nseg 0")
    both(tm, te, tn, 5, "nseg 5")
    both(tm, te, tn, -1, "nseg -1")
    both(None, te, tn, 3, "null model table")
    both(tm, None, tn, 3, "null shadow table")
    both(tm, te, None, 3, "null numel table")
    both(*_tables([ms[0], None, ms[2]], es[:3], [65, 9, 1023]), 3, "null model pointer with numel > 0")
    both(*_tables(ms[:3], [es[0], es[1], None], [65, 9, 1023]), 3, "null shadow pointer with numel > 0")
    both(*_tables(ms[:3], es[:3], [65, -1, 1023]), 3, "negative numel")
    both(*_tables(ms[:3], [es[0], ms[1], es[2]], [65, 9, 1023]), 3, "a shadow segment is its model segment")
    both(*_tables([ms[0], es[2], ms[2]], es[:3], [65, 9, 1023]), 3, "a model segment inside another pair's shadow segment")
    # partial overlap: the shadow begins inside the model segment
    tmo = (C.c_void_p * 1)(ms[2].ptr())
    teo = (C.c_void_p * 1)(ms[2].ptr() + 4 * 1000)
    both(tmo, teo, (C.c_long * 1)(1023), 1, "partial overlap")
    both((C.c_void_p * 1)(ms[2].ptr() + 2), (C.c_void_p * 1)(es[2].ptr()), (C.c_long * 1)(8), 1, "base not 4-byte aligned")
    torch.cuda.synchronize()
    for s, w in zip(ms + es, before):
        np.testing.assert_array_equal(s.words(), w)


# ------------------------------------------------------------------------------------------------------------ ModelEMA
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


def _state(net):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def _assert_same_state(got, want, what):
    assert list(got) == list(want), what
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, (what, k)
        assert torch.equal(_ibits(got[k]), _ibits(v)), (what, k)


def _arenas(net):
    torch.cuda.synchronize()
    eng = net.engine()
    return {n: getattr(eng, n).clone() for n in ("p_arena", "m_arena", "rm_arena", "rv_arena", "nbt_arena")}


class _HandRun:
    """four training steps driven by hand, ModelEMA.update() after each; snapshots of net.state_dict() after every step"""

    def __init__(self, graphed, batches):
        from object_detection_cib_amd.engine.ema import ModelEMA
        from object_detection_cib_amd.engine.graphed import GraphedTrainStep
        from object_detection_cib_amd.nn.optim.smart import SmartSGD
        self.net, self.loss = _net()
        net, eng = self.net, self.net.engine()
        self.ema = ModelEMA(net)
        self.initial = _state(net)
        self.snaps, self.losses = [], []
        if graphed:
            step = GraphedTrainStep(net, self.loss, B, S, S, CAP).capture(batches[0][0], batches[0][1])
            _assert_same_state(_state(net), self.initial, "capture() moved the state")
        else:
            opt = SmartSGD(net, lr=0.01)
        for x, tg, _ in batches:
            if graphed:
                total = step(x, tg, *HYPER)[0]
            else:
                for p in net.parameters():
                    p.grad = None
                total, _ = net.train_step(x, self.loss, FeatureShape(width=S, height=S), tg, float(B))
                opt.step()
            self.losses.append(float(total))
            self.ema.update()
            self.snaps.append(_state(net))
        self.eng = eng


@pytest.fixture(scope="module")
def hand(batches):
    return {g: _HandRun(g, batches) for g in (False, True)}


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_model_ema_equals_the_reference_on_snapshots(hand, graphed):
    run = hand[graphed]
    assert all(np.isfinite(run.losses)), run.losses
    assert run.ema.updates == STEPS
    got = run.ema.state_dict()
    assert list(got) == list(run.initial) and len(got) == len(run.net.state_dict())
    n_float = n_int = differ = moved = 0
    for k, v0 in run.initial.items():
        if v0.is_floating_point():
            e = v0.cpu().numpy()
            for t, snap in enumerate(run.snaps, 1):
                e = R.ema_update_ref(e, snap[k].cpu().numpy(), R.decay_ref(t))
            g = got[k].cpu().numpy()
            differ += int((R.bits(g) != R.bits(e)).sum())
            moved += int((R.bits(g) != R.bits(v0.cpu().numpy())).sum())
            assert g.shape == e.shape and np.array_equal(R.bits(g), R.bits(e)), k
            n_float += 1
        else:
            assert got[k].dtype == v0.dtype and torch.equal(got[k], v0), k                    # as at construction ...
            assert not torch.equal(run.snaps[-1][k], v0), k                                   # ... while the network's moved on
            n_int += 1
    print(f"ModelEMA graphed={graphed}: {n_float} float keys, {n_int} integer keys, {differ} values differ from the reference, "
          f"{moved} values moved away from their initial bits; losses {run.losses}")
    assert n_float and n_int and moved > 0


def test_model_ema_needs_the_hip_network():
    from object_detection_cib_amd.engine.ema import ModelEMA
    with pytest.raises(TypeError, match="engine"):
        ModelEMA(torch.nn.Conv2d(3, 8, 1).cuda())


# -------------------------------------------------------------------------------------------------------- experiment
def _experiment(graphed, seed=5, **kw):
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.warmup import OptimizerWarmupUpdater
    net, loss = _net(seed)
    return DefaultYolov5Experiment(net, loss, _anchors(), optimizer_warmup_updater=OptimizerWarmupUpdater(3, 0.1, 0.8, 0.937),
                                   max_epochs=4, graphed=graphed, max_targets=CAP, **kw)


class _ExpRun:
    """the experiment over the four batches; with ema=True a checkpoint is written after the second step"""

    def __init__(self, graphed, ema, batches, path=None):
        from object_detection_cib_amd.lightning.checkpoint import save_checkpoint
        self.exp = exp = _experiment(graphed, ema=ema)
        self.losses = []
        self.ckpt = None
        for i, b in enumerate(batches):
            self.losses.append(exp.optimize(b, STEPS).item())
            if i == 1 and path is not None:
                self.ckpt = save_checkpoint(path, exp.net, exp.optimizer, epoch=0, global_step=exp.global_step,
                                            ema_state=exp.ema_state_dict())
        self.arenas = _arenas(exp.net)


@pytest.fixture(scope="module")
def exp_runs(batches, tmp_path_factory):
    d = tmp_path_factory.mktemp("ema")
    return {(g, e): _ExpRun(g, e, batches, str(d / f"ema_{int(g)}.ckpt") if e else None) for g in (False, True) for e in (False, True)}, d


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_ema_never_writes_the_model(exp_runs, graphed):
    runs, _ = exp_runs
    on, off = runs[(graphed, True)], runs[(graphed, False)]
    assert off.exp.ema is None and on.exp.ema is not None and on.exp.ema.updates == STEPS
    print(f"experiment graphed={graphed}: losses with ema {on.losses} without {off.losses}")
    assert all(np.isfinite(on.losses)) and on.losses == off.losses
    for k, v in off.arenas.items():
        assert torch.equal(_ibits(on.arenas[k]), _ibits(v)), k
    assert not torch.equal(on.exp.ema._shadow["p"], on.arenas["p_arena"])             # (and the average is not the model)


def test_experiment_ema_arguments():
    import inspect
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
    sig = inspect.signature(DefaultYolov5Experiment.__init__).parameters
    for name, default in (("ema", False), ("ema_decay", 0.9999), ("ema_tau", 2000.0)):
        assert sig[name].default == default and sig[name].kind is inspect.Parameter.KEYWORD_ONLY


def _eval_forward(net, x, fused=False):
    net.eval()
    net.fuse_eval(fused)
    with torch.no_grad():
        out = [o.clone() for o in net.forward_raw(x)]
    net.fuse_eval(False)
    net.train()
    torch.cuda.synchronize()
    return out


def _same_tensors(a, b):
    return len(a) == len(b) and all(torch.equal(_ibits(p), _ibits(q)) for p, q in zip(a, b))


def test_applied(hand, exp_runs, batches):
    from object_detection_cib_amd.engine.graphed import GraphedEvalForward
    run = hand[False]
    net, ema = run.net, run.ema
    x = batches[0][0]
    ema_sd = ema.state_dict()
    before_sd = _state(net)
    before_fwd = _eval_forward(net, x)
    geval = GraphedEvalForward(net, _anchors(), B, S, S)                               # captured before the swap
    before_graphed = geval(x).clone()
    # a second network that holds the EMA weights, twice: load_state_dict(ema.state_dict()) and copy_to
    twin, _ = _net(77)
    twin.load_state_dict(ema_sd)
    twin2, _ = _net(78)
    assert ema.copy_to(twin2) is twin2
    _assert_same_state(_state(twin2), _state(twin), "copy_to")
    want = {f: _eval_forward(twin, x, fused=f) for f in (False, True)}
    want_graphed = GraphedEvalForward(twin, _anchors(), B, S, S)(x).clone()
    assert not _same_tensors(want[False], before_fwd), "the EMA weights compute what the raw ones do: nothing is tested"
    with ema.applied() as inside:
        assert inside is net and ema.is_applied
        _assert_same_state(_state(net), ema_sd, "state_dict() while applied")
        for fused in (False, True):
            assert _same_tensors(_eval_forward(net, x, fused=fused), want[fused]), f"eval forward while applied, fused={fused}"
        assert torch.equal(_ibits(geval(x)), _ibits(want_graphed)), "captured eval forward while applied"
        with pytest.raises(RuntimeError, match="applied"):
            ema.update()
        with pytest.raises(RuntimeError, match="applied"):
            with ema.applied():
                pass
        assert ema.is_applied and ema.updates == STEPS
    assert not ema.is_applied
    _assert_same_state(_state(net), before_sd, "state after applied()")
    assert _same_tensors(_eval_forward(net, x), before_fwd)
    assert torch.equal(_ibits(geval(x)), _ibits(before_graphed))
    _assert_same_state(ema.state_dict(), ema_sd, "the EMA after applied()")
    # an exception inside still swaps back
    with pytest.raises(KeyError):
        with ema.applied():
            raise KeyError("x")
    _assert_same_state(_state(net), before_sd, "state after a raising applied() block")
    # a training step through the experiment while applied
    runs, _ = exp_runs
    for graphed in (False, True):
        exp = runs[(graphed, True)].exp
        step0, upd0 = exp.global_step, exp.ema.updates
        with exp.ema.applied():
            with pytest.raises(RuntimeError, match="applied"):
                exp.optimize(batches[0], STEPS)
        assert (exp.global_step, exp.ema.updates) == (step0, upd0)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_checkpoint_resume(exp_runs, batches, graphed):
    from object_detection_cib_amd.engine.ema import ModelEMA
    from object_detection_cib_amd.lightning.checkpoint import EMA_KEY, load_checkpoint, save_checkpoint
    runs, d = exp_runs
    full = runs[(graphed, True)]
    path = str(d / f"ema_{int(graphed)}.ckpt")
    assert EMA_KEY == "ema" and set(full.ckpt[EMA_KEY]) == {"updates", "decay", "tau", "state_dict"}
    assert (full.ckpt[EMA_KEY]["updates"], full.ckpt[EMA_KEY]["decay"], full.ckpt[EMA_KEY]["tau"]) == (2, 0.9999, 2000.0)
    assert list(full.ckpt[EMA_KEY]["state_dict"]) == list(full.exp.net.state_dict())
    want = full.exp.ema.state_dict()

    resumed = _experiment(graphed, seed=40, ema=True)              # other initial weights: everything comes from the file
    meta = load_checkpoint(path, resumed.net, None, ema=resumed)   # (before the EMA exists: the state waits)
    assert resumed.ema is None and EMA_KEY in meta
    resumed.configure_optimizers()
    load_checkpoint(path, resumed.net, resumed.optimizer, ema=resumed)
    resumed.global_step = meta["global_step"]
    assert resumed.ema.updates == 2
    losses = [resumed.optimize(b, STEPS).item() for b in batches[2:]]
    print(f"EMA resume graphed={graphed}: losses {full.losses[2:]} resumed {losses}")
    assert losses == full.losses[2:]
    _assert_same_state(resumed.ema.state_dict(), want, f"resumed EMA graphed={graphed}")
    for k, v in full.arenas.items():
        assert torch.equal(_ibits(_arenas(resumed.net)[k]), _ibits(v)), k
    # the EMA's own state dict, saved on its own, is a weight file load_checkpoint reads as a bare state dict
    bare = str(d / f"bare_{int(graphed)}.pt")
    torch.save({"state_dict": {k: v.cpu() for k, v in want.items()}}, bare)
    other, _ = _net(41)
    load_checkpoint(bare, other)
    _assert_same_state(_state(other), want, "bare EMA weight file")
    # a file written without ema_state has no key, and leaves a passed EMA untouched
    plain = str(d / f"plain_{int(graphed)}.ckpt")
    assert EMA_KEY not in save_checkpoint(plain, full.exp.net, full.exp.optimizer)
    assert EMA_KEY not in torch.load(plain, map_location="cpu", weights_only=False)
    alone = ModelEMA(other, updates=7)
    kept = alone.state_dict()
    assert EMA_KEY not in load_checkpoint(plain, other, None, ema=alone)
    assert alone.updates == 7
    _assert_same_state(alone.state_dict(), kept, "an EMA passed with a file that has no key")
    load_checkpoint(path, other, None, ema=alone)                  # and a ModelEMA takes the key itself
    assert alone.updates == 2
    _assert_same_state(alone.state_dict(), {k: v.cuda() for k, v in full.ckpt[EMA_KEY]["state_dict"].items()}, "ModelEMA from the file")


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_validate_runs_the_averaged_weights(exp_runs, batches, graphed):
    runs, _ = exp_runs
    exp = runs[(graphed, True)].exp
    before = _arenas(exp.net)
    twin = _experiment(graphed, seed=90)
    exp.ema.copy_to(twin.net)
    want = [twin.validation_step(b)[1] for b in batches[:2]]
    want = [[t.clone() for t in dets] for dets in want]
    raw = [[t.clone() for t in exp.validation_step(b)[1]] for b in batches[:2]]
    seen = []
    orig = exp.validation_step

    def recording(batch, batch_idx=0):
        targets, dets = orig(batch, batch_idx)
        assert exp.ema.is_applied
        seen.append([t.clone() for t in dets])
        return targets, dets
    exp.validation_step = recording
    try:
        report = exp.validate(batches[:2], NC)
    finally:
        del exp.validation_step
    assert isinstance(report, dict) and len(seen) == 2 and not exp.ema.is_applied
    rows = [sum(int(t.shape[0]) for t in dets) for dets in seen]
    print(f"validate() graphed={graphed} with ema=True: detections per batch {rows}")
    assert sum(rows) > 0
    for got, w in zip(seen, want):
        assert _same_tensors(got, w)
    assert not all(_same_tensors(g, r) for g, r in zip(seen, raw)), "the raw weights give the same detections: nothing is tested"
    for k, v in before.items():
        assert torch.equal(_ibits(_arenas(exp.net)[k]), _ibits(v)), k
