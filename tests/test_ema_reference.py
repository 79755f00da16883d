"""The weight EMA's host side (engine/ema.py) and its numpy reference (tests/ema_reference.py), without a GPU.

The reference is pinned bit for bit against the literal YOLOv5 loop (utils/torch_utils.py ModelEMA.update) on torch CPU tensors,
`v *= d; v += (1 - d) * m` with d a Python double: 10 sizes x 6 update counts, magnitudes from 1e-42 (subnormal) to 1e4.
"""
import math

import numpy as np
import pytest
import torch

import ema_reference as R
from object_detection_cib_amd.engine.ema import ema_coefficients, ema_decay


@pytest.mark.parametrize("updates", R.UPDATES)
@pytest.mark.parametrize("n", R.SIZES)
def test_reference_equals_the_yolov5_loop(n, updates):
    d = R.decay_ref(updates)
    e, m = R.mixed(n, 3 * n + 1), R.mixed(n, 5 * n + 2)
    want = R.ema_update_ref(e, m, d)
    v, msd = torch.from_numpy(e.copy()), torch.from_numpy(m.copy())
    v *= d
    v += (1 - d) * msd
    mismatches = int((R.bits(v.numpy()) != R.bits(want)).sum())
    print(f"n {n} updates {updates} d {d!r}: {mismatches} of {n} values differ from torch")
    np.testing.assert_array_equal(R.bits(v.numpy()), R.bits(want))
    np.testing.assert_array_equal(msd.numpy().view(np.uint32), m.view(np.uint32))


def test_inputs_reach_subnormals_and_1e4():
    x = np.abs(R.mixed(70001, 1))
    tiny = np.finfo(np.float32).tiny
    assert ((x > 0) & (x < tiny)).sum() > 1000 and x.max() > 5e3 and (x == 0).any()
    assert np.isnan(R.mixed(64, 1, specials=True)).sum() == 3


def test_reference_specials():
    """NaN stays NaN, Inf stays Inf, a subnormal result is not flushed"""
    e = np.array([np.nan, np.inf, -np.inf, 1e-42, 0.0, 1.0], dtype=np.float32)
    m = np.array([1.0, 1.0, np.inf, 1e-42, -0.0, np.nan], dtype=np.float32)
    out = R.ema_update_ref(e, m, R.decay_ref(2000))
    assert np.isnan(out[0]) and out[1] == np.inf and np.isnan(out[2]) and np.isnan(out[5])
    assert 0 < out[3] < np.finfo(np.float32).tiny and out[4] == 0.0


@pytest.mark.parametrize("updates", R.UPDATES + (0,))
def test_ema_decay_is_the_formula(updates):
    assert ema_decay(updates) == 0.9999 * (1 - math.exp(-updates / 2000.0))
    assert ema_decay(updates, 0.999, 500.0) == 0.999 * (1 - math.exp(-updates / 500.0))
    assert ema_decay(updates) == R.decay_ref(updates)
    assert isinstance(ema_decay(updates), float) and 0.0 <= ema_decay(updates) < 1.0


def test_ema_coefficients_round_one_minus_d_in_double():
    d = ema_decay(2000)
    c0, c1 = ema_coefficients(2000, 0.9999, 2000.0)
    assert c0.dtype == np.float32 and c1.dtype == np.float32
    assert c0 == np.float32(d) and c1 == np.float32(1 - d)
    assert c1 != np.float32(1) - np.float32(d)                 # 0.36794266 against 0.36794263
    assert repr(float(c1))[:10] == "0.36794266" and repr(float(np.float32(1) - np.float32(d)))[:10] == "0.36794263"
    for u in R.UPDATES:
        a, b = ema_coefficients(u)
        assert a == np.float32(ema_decay(u)) and b == np.float32(1.0 - ema_decay(u))


def test_model_ema_refuses_a_network_without_engine():
    from object_detection_cib_amd.engine.ema import ModelEMA
    with pytest.raises(TypeError, match="engine"):
        ModelEMA(torch.nn.Conv2d(3, 8, 1))
