"""Plain numpy restatement of the gradient accumulation launch (csrc/accumulate.hip, engine/accumulate.py) and the inputs its
tests share.

    first:  acc <- grad                 a copy of the 32-bit words (-0.0 stays -0.0, a NaN keeps its payload)
    else:   acc <- acc + grad           numpy float32: one rounding per element, what torch's `a.add_(b)` gives

tests/test_accumulate_reference.py pins this against CPU torch; tests/test_hip_accumulate.py pins the kernel against it.
"""
import numpy as np

SIZES = (0, 1, 3, 4, 5, 63, 4095, 4096, 4097, 8193)
OFFSETS = [(0, 0), (1, 1), (1, 0), (0, 2)]   # (acc, grad) base offsets in elements from a 16-byte boundary


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def accumulate_ref(acc, grad, first):
    """acc, grad: float32 arrays -> the new acc (float32, a new array)"""
    grad = np.ascontiguousarray(np.asarray(grad, dtype=np.float32))
    if first:
        return grad.view(np.uint32).copy().view(np.float32)
    with np.errstate(all="ignore"):
        return np.asarray(acc, dtype=np.float32) + grad


def same_bits_or_both_nan(a, b):
    """bit equality except where both are NaN (the payload of a NaN that an add produces is not compared)"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | nan).all())


# pairs (a, b) at the edges of fp32 addition, as 32-bit words
_EDGE_WORDS = [
    (0x00000001, 0x00000001),      # subnormal + subnormal -> subnormal
    (0x007FFFFF, 0x00000001),      # largest subnormal + smallest -> smallest normal
    (0x00800000, 0x80000001),      # smallest normal - smallest subnormal -> subnormal result
    (0x00800000, 0x807FFFFF),      # -> smallest subnormal
    (0x00000000, 0x80000000),      # +0 + -0 -> +0
    (0x80000000, 0x80000000),      # -0 + -0 -> -0
    (0x80000000, 0x00000000),
    (0x3F800000, 0xBF800000),      # 1 - 1 -> +0
    (0x7F7FFFFF, 0x7F7FFFFF),      # overflow to +Inf
    (0xFF7FFFFF, 0xFF7FFFFF),      # overflow to -Inf
    (0x7F7FFFFF, 0x73000000),      # max + half an ulp of max: ties to even -> Inf
    (0x7F7FFFFF, 0x72FFFFFF),      # just below the tie: stays max
    (0x7F800000, 0x3F800000),      # Inf + 1
    (0x7F800000, 0xFF800000),      # Inf - Inf -> NaN
    (0xFF800000, 0xFF800000),
    (0x7FC00000, 0x3F800000),      # NaN + 1
    (0x3F800000, 0x7FA00001),      # 1 + signalling NaN
    (0xFFC12345, 0x7FC00001),      # NaN + NaN
    (0x3F800000, 0x33800000),      # 1 + 2^-24: tie to even -> 1
    (0x3F800001, 0x33800000),      # odd + tie -> rounds up
    (0x4B800000, 0x3F000000),      # 2^24 + 0.5
]


def edge_pairs():
    """(a, b): float32 arrays of the edge operands above, both orders"""
    w = np.array(_EDGE_WORDS + [(y, x) for x, y in _EDGE_WORDS], dtype=np.uint32)
    return w[:, 0].copy().view(np.float32), w[:, 1].copy().view(np.float32)


def mixed(n, seed):
    """n float32 values of both signs, magnitudes log-uniform from 1e-42 (subnormal) to 1e38 (sums overflow), exact zeros among
    them, and - where n allows - NaN (two payloads), +-Inf, -0.0, the largest subnormal and +-max at fixed places"""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-42.0, 38.4, n)
    with np.errstate(all="ignore"):
        x = (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    x[rng.random(n) < 0.02] = 0.0
    words = (0x7FC00000, 0x7FA00001, 0x7F800000, 0xFF800000, 0x80000000, 0x007FFFFF, 0xFFC12345, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000001)
    u = x.view(np.uint32)
    for k, w in enumerate(words):
        if 5 * k + 2 < n:
            u[5 * k + 2] = w
    return x


def values(n, seed):
    """(acc, grad) of n elements: the edge pairs in front where they fit, `mixed` behind them"""
    a, g = mixed(n, seed), mixed(n, seed + 1)
    ea, eg = edge_pairs()
    k = min(n, len(ea))
    if n >= 64:                      # (the small sizes keep mixed()'s specials)
        a[-k:], g[-k:] = ea[:k], eg[:k]
    return a, g
