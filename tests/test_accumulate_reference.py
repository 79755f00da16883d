"""The numpy reference of the accumulate launch against CPU torch, and the host side of gradient accumulation
(engine/accumulate.py: AccumulationWindow, yolov5_accumulate).  No GPU."""
import inspect

import numpy as np
import pytest
import torch

import accumulate_reference as R
from object_detection_cib_amd.engine.accumulate import AccumulationWindow, yolov5_accumulate


def _torch_add(a, b):
    t = torch.from_numpy(np.array(a, dtype=np.float32, copy=True))
    t.add_(torch.from_numpy(np.array(b, dtype=np.float32, copy=True)))
    return t.numpy()


def test_add_equals_torch_on_the_edge_pairs():
    a, b = R.edge_pairs()
    got, want = R.accumulate_ref(a, b, False), _torch_add(a, b)
    for x, y, g, w in zip(R.bits(a), R.bits(b), R.bits(got), R.bits(want)):
        print(f"{x:08x} + {y:08x} -> numpy {g:08x} torch {w:08x}")
    assert np.array_equal(np.isnan(got), np.isnan(want))             # NaN positions; payloads are not compared
    assert R.same_bits_or_both_nan(got, want)
    # the cases are what their comments say
    r = dict(zip(zip(R.bits(a).tolist(), R.bits(b).tolist()), R.bits(got).tolist()))
    assert r[(0x007FFFFF, 0x00000001)] == 0x00800000 and r[(0x00800000, 0x807FFFFF)] == 0x00000001
    assert r[(0x00000000, 0x80000000)] == 0x00000000 and r[(0x80000000, 0x80000000)] == 0x80000000
    assert r[(0x7F7FFFFF, 0x7F7FFFFF)] == 0x7F800000 and r[(0xFF7FFFFF, 0xFF7FFFFF)] == 0xFF800000
    assert r[(0x7F7FFFFF, 0x73000000)] == 0x7F800000 and r[(0x7F7FFFFF, 0x72FFFFFF)] == 0x7F7FFFFF
    assert r[(0x3F800000, 0x33800000)] == 0x3F800000 and r[(0x3F800001, 0x33800000)] == 0x3F800002
    assert np.isnan(got[(R.bits(a) == 0x7F800000) & (R.bits(b) == 0xFF800000)]).all()


@pytest.mark.parametrize("n", [n for n in R.SIZES if n] + [70001])
def test_add_equals_torch_on_the_shared_values(n):
    a, g = R.values(n, seed=n)
    got, want = R.accumulate_ref(a, g, False), _torch_add(a, g)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert R.same_bits_or_both_nan(got, want)
    if n >= 4096:
        sub = (np.abs(got) < np.float32(1.1754944e-38)) & (got != 0)
        assert sub.any() and np.isinf(got).any() and np.isnan(got).any()          # the value set reaches every class


def test_running_sum_is_torch_grad_accumulation():
    """((g1 + g2) + g3) + g4, the first one copied: what `.grad +=` leaves"""
    gs = [R.mixed(4097, s) for s in range(4)]
    acc = None
    t = None
    for k, g in enumerate(gs):
        acc = R.accumulate_ref(acc, g, k == 0)
        t = torch.from_numpy(g.copy()) if k == 0 else t.add_(torch.from_numpy(g.copy()))
    assert R.same_bits_or_both_nan(acc, t.numpy())


def test_the_copy_keeps_the_words():
    g = R.mixed(300, 7)
    junk = R.mixed(300, 8)
    out = R.accumulate_ref(junk, g, True)
    assert np.array_equal(R.bits(out), R.bits(g))                     # -0.0, NaN payloads: all 32 bits
    assert (R.bits(g) == 0x80000000).any() and (R.bits(g) == 0xFFC12345).any()
    zero = np.zeros(300, dtype=np.float32)
    assert not np.array_equal(R.bits(R.accumulate_ref(zero, g, False)), R.bits(g))      # an add to zero would lose -0.0
    before = R.bits(g).copy()
    out[:] = 1.0
    assert np.array_equal(R.bits(g), before)                          # a new array, not a view


# ------------------------------------------------------------------------------------------------------------- the window
def test_window_n1_closes_every_call():
    w = AccumulationWindow(1)
    for _ in range(4):
        assert w.first and not w.flush_needed
        assert w.advance() is True
    assert AccumulationWindow().n == 1


def test_window_n3_over_seven_calls():
    w = AccumulationWindow(3)
    closes, firsts = [], []
    for _ in range(7):
        firsts.append(w.first)
        closes.append(w.advance())
    assert closes == [False, False, True, False, False, True, False]
    assert firsts == [True, False, False, True, False, False, True]
    assert w.flush_needed and not w.first
    w.reset()
    assert not w.flush_needed and w.first
    w.reset()                                                         # a flush on a closed window does nothing
    assert not w.flush_needed and w.first and w.advance() is False


@pytest.mark.parametrize("bad", [0, -1, 2.0, 1.5, "3", None, True])
def test_window_refuses_bad_n(bad):
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        AccumulationWindow(bad)


def test_window_takes_integer_types():
    assert AccumulationWindow(np.int64(4)).n == 4


@pytest.mark.parametrize("batch_size,want", [(64, (1, 1.0)), (16, (4, 1.0)), (24, (3, 1.125)), (128, (1, 2.0))])
def test_yolov5_accumulate(batch_size, want):
    assert yolov5_accumulate(batch_size) == want
    assert yolov5_accumulate(batch_size, nbs=64) == want


def test_keywords():
    from object_detection_cib_amd.engine.graphed import GraphedTrainStep
    from object_detection_cib_amd.engine.multiscale import MultiScaleTrainStep
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
    for cls in (GraphedTrainStep, MultiScaleTrainStep, DefaultYolov5Experiment):
        assert inspect.signature(cls.__init__).parameters["accumulate_grad_batches"].default == 1
    assert callable(DefaultYolov5Experiment.step_accumulated) and callable(GraphedTrainStep.flush) and callable(MultiScaleTrainStep.flush)


def test_the_entry_refuses_bad_arguments_before_any_launch():
    """argument validation happens before any launch, so it is testable without a GPU"""
    from object_detection_cib_amd import _lib
    h = _lib.lib()
    a = np.zeros(64, dtype=np.float32)
    g = np.zeros(64, dtype=np.float32)
    pa, pg = a.ctypes.data, g.ctypes.data
    for what, args in (("negative n", (pa, pg, -1, 0, None)), ("null acc", (None, pg, 8, 0, None)), ("null grad", (pa, None, 8, 1, None)),
                       ("mode 3", (pa, pg, 8, 3, None)), ("mode -1", (pa, pg, 8, -1, None)), ("mode 2 without ctl", (pa, pg, 8, 2, None)),
                       ("misaligned acc", (pa + 2, pg, 8, 0, None)), ("misaligned grad", (pa, pg + 1, 8, 0, None)),
                       ("acc is grad", (pa, pa, 8, 0, None)), ("partial overlap", (pa, pa + 16, 8, 0, None))):
        rc = h.kodhip_grad_accumulate(*args, None)
        assert rc < 0 and b"grad_accumulate" in h.kodhip_last_error(), (what, rc, h.kodhip_last_error())
    assert h.kodhip_grad_accumulate(None, None, 0, 0, None, None) == 0               # n == 0 launches nothing
    assert h.kodhip_grad_accumulate(pa, pg, 0, 1, None, None) == 0
