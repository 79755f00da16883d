"""Plain numpy references for the video-frame input path (csrc/video.hip, data/frames.py): the 4:2:0 YUV -> RGB conversion in
20-bit fixed point as OpenCV's color_yuv.simd.hpp states it (int64 here: no accumulator can wrap), the colour matrices in
Python floats, and packers that lay planes out the way a decoder or a camera leaves them - rows `pitch` bytes apart, the bytes
between them filled with whatever the caller's generator gives."""
import numpy as np

SHIFT = 20
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def matrix_real(name):
    """(yoff, cy, cvr, cvg, cug, cub) of a matrix name as Python floats: the exact coefficients, no fixed point"""
    kr, kb = KR_KB[name.split("-")[0]]
    kg = 1.0 - kr - kb
    s, cy, yoff = (1.0, 1.0, 0) if name.endswith("-full") else (255.0 / 224.0, 255.0 / 219.0, 16)
    return yoff, cy, 2.0 * (1.0 - kr) * s, -2.0 * kr * (1.0 - kr) / kg * s, -2.0 * kb * (1.0 - kb) / kg * s, 2.0 * (1.0 - kb) * s


def matrix_coeffs_ref(name):
    """the six integers: round(c * 2^20) of `matrix_real`"""
    m = matrix_real(name)
    return (m[0],) + tuple(int(round(c * (1 << SHIFT))) for c in m[1:])


def yuv_to_rgb_sums(Y, U, V, coeffs):
    """the three accumulators before the shift, int64, for arrays of equal shape"""
    yoff, cy, cvr, cvg, cug, cub = (int(c) for c in coeffs)
    Y, uu, vv = np.asarray(Y, np.int64), np.asarray(U, np.int64) - 128, np.asarray(V, np.int64) - 128
    y = np.maximum(0, Y - yoff) * cy + (1 << (SHIFT - 1))
    return y + cvr * vv, y + cvg * vv + cug * uu, y + cub * uu


def yuv420_to_rgb(y, u, v, coeffs):
    """y [h, w], u and v [h/2, w/2] uint8 -> RGB uint8 [h, w, 3]: pixel (r, c) takes chroma sample (r >> 1, c >> 1);
    >> is numpy's arithmetic shift (floor on negative sums)"""
    h, w = y.shape
    assert h % 2 == 0 and w % 2 == 0 and u.shape == v.shape == (h // 2, w // 2)
    U, V = (np.repeat(np.repeat(p, 2, axis=0), 2, axis=1) for p in (u, v))
    return np.stack([np.clip(s >> SHIFT, 0, 255) for s in yuv_to_rgb_sums(y, U, V, coeffs)], axis=-1).astype(np.uint8)


def yuv_to_rgb_real(Y, U, V, name):
    """the real-valued conversion of matrix `name` in float64, clipped to 0..255 (luma below the offset counts as the offset,
    as in the fixed-point form)"""
    yoff, cy, cvr, cvg, cug, cub = matrix_real(name)
    Y, uu, vv = np.maximum(0.0, np.asarray(Y, np.float64) - yoff) * cy, np.asarray(U, np.float64) - 128, np.asarray(V, np.float64) - 128
    return tuple(np.clip(c, 0.0, 255.0) for c in (Y + cvr * vv, Y + cvg * vv + cug * uu, Y + cub * uu))


# ---------------------------------------------------------------------------------------------------------------- packers
def pitched(plane, pitch, rng):
    """a [rows, row bytes] uint8 plane -> (1-D buffer of exactly (rows - 1) * pitch + row bytes, its padding from rng): the last
    row's last byte is the buffer's last byte"""
    rows, nb = plane.shape
    assert pitch >= nb
    buf = rng.integers(0, 256, (rows - 1) * pitch + nb, dtype=np.uint8)
    for r in range(rows):
        buf[r * pitch:r * pitch + nb] = plane[r]
    return buf


def nv12_surface(y, u, v, pitch, uv_offset, rng):
    """one decoder surface: Y rows at 0, interleaved UV rows at uv_offset, both `pitch` apart; everything else from rng"""
    h, w = y.shape
    assert uv_offset >= (h - 1) * pitch + w
    uv = np.stack([u, v], axis=-1).reshape(h // 2, w)
    buf = rng.integers(0, 256, uv_offset + (h // 2 - 1) * pitch + w, dtype=np.uint8)
    buf[:(h - 1) * pitch + w] = pitched(y, pitch, rng)
    buf[uv_offset:] = pitched(uv, pitch, rng)
    return buf


def packed_yuv(y, u, v, fmt):
    """cv2's [h * 3 / 2, w] layout: fmt "nv12" (Y, interleaved UV rows) or "i420" (Y, U plane, V plane)"""
    h, w = y.shape
    tail = np.stack([u, v], axis=-1).reshape(-1) if fmt == "nv12" else np.concatenate((u.reshape(-1), v.reshape(-1)))
    return np.concatenate((y.reshape(-1), tail)).reshape(h * 3 // 2, w)
