"""Plain numpy restatement of the weight EMA update (csrc/ema.hip, engine/ema.py) and the inputs its tests share.

    e <- (e * float32(d)) + (float32(1 - d) * m)          numpy float32: every operation rounded on its own

`d` is the Python double of YOLOv5's ramp; `1 - d` is formed in double and rounded once.  tests/test_ema_reference.py pins this
against the literal YOLOv5 loop on torch CPU tensors; tests/test_hip_ema.py pins the kernel against it, bit for bit.
"""
import math

import numpy as np

SIZES = (1, 3, 4, 5, 63, 64, 65, 1023, 1025, 70001)
UPDATES = (1, 2, 17, 2000, 10 ** 5, 10 ** 7)


def decay_ref(updates, decay=0.9999, tau=2000.0):
    return decay * (1 - math.exp(-updates / tau))


def ema_update_ref(e, m, d):
    """e, m: float32 arrays; d: Python double -> the new e (float32)"""
    e, m = np.asarray(e, dtype=np.float32), np.asarray(m, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (e * np.float32(d)) + (np.float32(1 - d) * m)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def mixed(n, seed, specials=False):
    """n float32 values of both signs whose magnitudes run from 1e-42 (subnormal) to 1e4, log-uniform, with exact zeros among
    them; specials: NaN (two payloads), +-Inf, -0.0 and the largest subnormal at fixed places where n allows"""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-42.0, 4.0, n)
    x = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    x[rng.random(n) < 0.02] = 0.0
    if specials:
        words = (0x7FC00000, 0x7FA00001, 0x7F800000, 0xFF800000, 0x80000000, 0x007FFFFF, 0xFFC12345)
        u = x.view(np.uint32)
        for k, w in enumerate(words):
            if 7 * k + 2 < n:
                u[7 * k + 2] = w
    return x
