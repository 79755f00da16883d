"""Multi-scale training without a GPU: the size schedule (engine/multiscale.py) against the restatement of YOLOv5's draw in
tests/multiscale_reference.py, the resize arithmetic against torch's CPU F.interpolate, and the argument checks of
kodhip_multiscale_batch (made before any launch, so they run here like those of tests/test_abi.py).

Resize anchor: `resize_ref` (the arithmetic the device kernel is held to bit for bit) against F.interpolate(mode="bilinear",
align_corners=False) on pixels in [0, 1] stays within ulp32(H - 1) + ulp32(W - 1) of the source size H x W - the bound
tests/tta_reference.py derives (the source coordinate of each axis is rounded once more than torch's).  Measured over the
whole plans of the five bases, up- and down-scaling: at most 0.33 of the bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multiscale_reference as M

BASES = [(640, 640), (416, 416), (128, 128), (64, 128), (96, 160)]


def _schedule(*a, **k):
    from object_detection_cib_amd.engine.multiscale import MultiScaleSchedule
    return MultiScaleSchedule(*a, **k)


@pytest.mark.parametrize("base", BASES)
def test_draws_equal_the_restatement(base):
    H, W = base
    want = M.draw_ref(H, W, 0, 1000)
    s = _schedule(H, W, 0, (0.5, 1.5), 32)
    got = []
    for _ in range(1000):
        size = s.next()
        got.append((s.sz, size))
    assert got == want
    from object_detection_cib_amd.engine.multiscale import multiscale_sizes
    assert set(multiscale_sizes(H, W)) == {c for _, c in want} == set(s.canvases())
    assert all(h % 32 == 0 and w % 32 == 0 for _, (h, w) in want)


def test_size_sets():
    d640 = [sz for sz, _ in M.draw_ref(640, 640, 0, 1000)]
    assert sorted(set(d640)) == list(range(320, 961, 32)) and len(set(d640)) == 21
    counts = np.bincount(np.array(d640) // 32)[10:]
    assert counts.min() > 1000 / 21 * 0.5 and counts.max() < 1000 / 21 * 1.6, counts            # each about 1/21
    d416 = [sz for sz, _ in M.draw_ref(416, 416, 0, 1000)]
    assert sorted(set(d416)) == list(range(192, 641, 32))
    c = {sz: d416.count(sz) for sz in set(d416)}
    inner = np.mean([v for k, v in c.items() if k not in (192, 640)])
    assert 0.25 * inner < c[192] < 0.8 * inner and 0.25 * inner < c[640] < 0.8 * inner, c         # the end sizes at half weight
    assert sorted({sz for sz, _ in M.draw_ref(128, 128, 0, 1000)}) == [64, 96, 128, 160, 192]
    from object_detection_cib_amd.engine.multiscale import multiscale_sizes
    assert multiscale_sizes(128, 128) == [(64, 64), (96, 96), (128, 128), (160, 160), (192, 192)]
    assert (32, 64) in multiscale_sizes(64, 128) and (96, 192) in multiscale_sizes(64, 128)
    assert (160, 224) in multiscale_sizes(96, 160)


def test_interval_sizes_and_resume():
    s = _schedule(128, 128, 5, (0.5, 1.5), 32, interval=3)
    got = [s.next() for _ in range(30)]
    assert got == [c for _, c in M.draw_ref(128, 128, 5, 30, interval=3)]
    assert all(got[3 * i] == got[3 * i + 1] == got[3 * i + 2] for i in range(10)) and len(set(got)) > 1
    assert s.state_dict() == {"seed": 5, "draws": 10, "steps": 30}
    # explicit sizes: rng.choice over the list
    s = _schedule(128, 128, 2, (0.5, 1.5), 32, sizes=[64, 128, 192])
    got = [s.next() for _ in range(200)]
    assert got == [c for _, c in M.draw_ref(128, 128, 2, 200, sizes=[64, 128, 192])]
    assert set(got) == {(64, 64), (128, 128), (192, 192)} == set(s.canvases())
    # a resume after k draws continues the sequence; the global generator is never touched
    import random
    random.seed(123)
    before = random.getstate()
    for interval, k in ((1, 17), (3, 17)):
        full = _schedule(96, 160, 9, (0.5, 1.5), 32, interval=interval)
        seq = [full.next() for _ in range(60)]
        part = _schedule(96, 160, 9, (0.5, 1.5), 32, interval=interval)
        for _ in range(k):
            part.next()
        resumed = _schedule(96, 160, 77, (0.5, 1.5), 32, interval=interval)
        resumed.load_state_dict(part.state_dict())
        assert [resumed.next() for _ in range(60 - k)] == seq[k:]
    assert random.getstate() == before
    # the k-th draw depends on (seed, k) only
    assert [_schedule(640, 640, 4).next() for _ in range(3)] == [_schedule(640, 640, 4).next() for _ in range(3)]


def test_refused_at_construction():
    with pytest.raises(ValueError, match="grid size"):
        _schedule(32, 32, 0, (0.5, 1.5), 32)                   # sz = 0 can be drawn
    with pytest.raises(ValueError, match="grid size"):
        _schedule(128, 128, 0, (0.5, 1.5), 32, sizes=[16, 128])
    with pytest.raises(ValueError, match="interval"):
        _schedule(128, 128, 0, (0.5, 1.5), 32, interval=0)


# ---------------------------------------------------------------------------------------------------- resize anchor
@pytest.mark.parametrize("base", [(64, 64), (128, 128), (64, 128), (96, 160), (640, 640)])
def test_resize_ref_against_torch_interpolate(base):
    H, W = base
    x = M.image_batch(1 if H == 640 else 2, H, W, seed=H + 3 * W)
    bound = float(np.spacing(np.float32(H - 1))) + float(np.spacing(np.float32(W - 1)))
    worst, seen_up, seen_down = 0.0, False, False
    for sz in sorted({sz for sz, _ in M.draw_ref(H, W, 0, 2000)}):
        h, w = M.canvas_ref(H, W, sz)
        want = F.interpolate(torch.from_numpy(x), size=(h, w), mode="bilinear", align_corners=False).numpy()
        got = M.resize_ref(x, h, w)
        assert got.shape == want.shape == (x.shape[0], 3, h, w)
        worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max()))
        seen_up, seen_down = seen_up or h > H, seen_down or h < H
        if (h, w) == (H, W):
            np.testing.assert_array_equal(got.view(np.uint32), x.view(np.uint32))           # identity: the pixels themselves
    print(f"multi-scale resize {H}x{W}: worst |resize_ref - F.interpolate| = {worst:.3e} = {worst / bound:.3f} of the bound {bound:.3e}")
    assert seen_up and seen_down
    assert worst <= bound


def test_pairs_and_boxes_restatement():
    x = M.image_batch(2, 64, 64, seed=1)
    p = M.to_pairs_ref(x)
    assert p.shape == (2, 64, 64, 4) and not p[..., 3].any()
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)     # torch rounds to nearest even too
    np.testing.assert_array_equal(p[..., :3], want.transpose(0, 2, 3, 1))
    wide = M.widen_pairs_ref(p)
    np.testing.assert_array_equal(wide, torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    f, q = M.resize_pairs_ref(p, 64, 64)
    np.testing.assert_array_equal(q, p)                                                   # identity returns the source pairs
    b = np.array([[1.5, 2.25, 100.125, 60.0], [0, 0, 0, 0]])
    s = M.scale_boxes_ref(b, 64, 128, 96, 192)
    np.testing.assert_array_equal(s, b * 1.5)
    assert not s[1].any()


# ------------------------------------------------------------------------------------------------ argument refusal
def test_multiscale_batch_refuses_bad_arguments_without_a_launch():
    from object_detection_cib_amd import _lib
    h = _lib.lib()
    assert h.kodhip_version() >= 112
    X, P, O, Fo, BI, BO = 0x100000, 0x200000, 0x4000000, 0x8000000, 0xC000000, 0xD000000       # never dereferenced: every call is refused

    def call(x=X, xp=None, out=O, f32=None, B=2, H=64, W=64, hh=96, ww=96, bi=None, bo=None, n=0):
        return h.kodhip_multiscale_batch(x, xp, out, f32, B, H, W, hh, ww, bi, bo, n, None)
    cases = [(dict(xp=P), "exactly one source"), (dict(x=None), "exactly one source"), (dict(out=None), "null out_pairs"),
             (dict(W=63), "even"), (dict(ww=95), "even"), (dict(B=0), "bad sizes"), (dict(H=0), "bad sizes"), (dict(hh=-32), "bad sizes"),
             (dict(ww=0), "bad sizes"), (dict(B=1 << 14, hh=1 << 10, ww=1 << 10), "too large"), (dict(out=X), "overlaps the source"),
             (dict(out=X + 64 * 64 * 12), "overlaps the source"), (dict(f32=X + 16), "overlaps the source"),
             (dict(x=None, xp=P, out=P + 2 * 64 * 64 * 8 - 16), "overlaps the source"), (dict(n=-1), "negative box count"),
             (dict(bi=BI, bo=None, n=3), "without boxes_out"), (dict(bi=BI, bo=BI + 32, n=3), "boxes_out must be"),
             (dict(out=O + 8), "misaligned")]
    for kw, msg in cases:
        rc = call(**kw)
        err = h.kodhip_last_error().decode()
        assert rc < 0 and "multiscale_batch" in err and msg in err, (kw, rc, err)
