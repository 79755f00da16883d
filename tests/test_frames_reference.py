"""CPU checks of the video-frame input path (data/frames.py, csrc/video.hip's launcher): the colour matrices against their
definitions and over all 2^24 (Y, U, V) triples, `frame_table`'s addresses, pitches and geometry on CPU tensors, every
ValueError a bad frame raises (by index, from host arithmetic alone) and the launcher's argument checks, which run before any
launch and so without a GPU.

Bounds: a coefficient rounded to 2^-20 is off by at most 2^-21, times at most 255 + 2 * 128 levels of input: 2.4e-4 of a level
on top of the 0.5 of rounding the result - 0.51 holds the derived tables.  OpenCV's BT.601 integers are not round(c * 2^20) of
the exact coefficients (CUB 2116026 against 2115867: 1.5e-4 * 128 = 0.02 level, the others less): within 1.0.
Measured here: derived tables 0.5002, OpenCV's against exact BT.601 0.690, largest accumulator 5.74e8."""
import numpy as np
import pytest
import torch

import frames_reference as R
from object_detection_cib_amd.data.frames import (BGR24, FRAME_DESC, I420, MATRICES, NV12, RGB24, Frame, frame_table,
                                                  matrix_coeffs)

OPENCV_BT601 = (16, 1220542, 1673527, -852492, -409993, 2116026)


def test_matrix_coefficients():
    assert matrix_coeffs("bt601") == OPENCV_BT601
    for name in ("bt709", "bt601-full", "bt709-full"):
        assert matrix_coeffs(name) == R.matrix_coeffs_ref(name), name
    assert set(MATRICES) == {"bt601", "bt709", "bt601-full", "bt709-full"}
    assert matrix_coeffs("bt709-full")[:2] == (0, 1 << 20)
    with pytest.raises(ValueError, match="bt2020"):
        matrix_coeffs("bt2020")


def test_all_triples_error_and_accumulator_bounds():
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst, acc = {}, 0
    tables = [(n, matrix_coeffs(n), n) for n in ("bt709", "bt601-full", "bt709-full")] + [("opencv bt601", OPENCV_BT601, "bt601")]
    for tag, coeffs, real in tables:
        err = 0.0
        for Y in range(256):
            sums = R.yuv_to_rgb_sums(np.full_like(U, Y), U, V, coeffs)
            want = R.yuv_to_rgb_real(np.full_like(U, Y), U, V, real)
            for s, wv in zip(sums, want):
                acc = max(acc, int(np.abs(s).max()))
                err = max(err, float(np.abs(np.clip(s >> 20, 0, 255) - wv).max()))
        worst[tag] = err
    print(f"FRAMES all triples: worst error {worst}, largest accumulator {acc:.4g}")
    assert acc < 2 ** 31
    for tag in ("bt709", "bt601-full", "bt709-full"):
        assert worst[tag] <= 0.51, worst
    assert worst["opencv bt601"] <= 1.0, worst


def test_reference_conversion_by_hand():
    # one 2 x 2 block, BT.601 limited: Y 16 / 235 with neutral chroma are black / white, Y below 16 is black too
    y = np.array([[16, 235], [0, 128]], np.uint8)
    rgb = R.yuv420_to_rgb(y, np.array([[128]], np.uint8), np.array([[128]], np.uint8), OPENCV_BT601)
    assert rgb[0, 0].tolist() == [0, 0, 0] and rgb[0, 1].tolist() == [255, 255, 255] and rgb[1, 0].tolist() == [0, 0, 0]
    assert rgb[1, 1].tolist() == [130, 130, 130]                   # (128 - 16) * 255 / 219 = 130.4
    # chroma is per 2 x 2 block; a strong V saturates red and floors green through a negative sum
    y = np.full((2, 4), 128, np.uint8)
    rgb = R.yuv420_to_rgb(y, np.array([[128, 0]], np.uint8), np.array([[255, 128]], np.uint8), OPENCV_BT601)
    assert (rgb[:, :2] == rgb[0, 0]).all() and (rgb[:, 2:] == rgb[0, 2]).all()
    assert rgb[0, 0].tolist() == [255, 27, 130] and rgb[0, 2].tolist() == [130, 180, 0]


# -------------------------------------------------------------------------------------------------------------- frame_table
def _planes(h, w, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))


def test_frame_table_addresses_and_pitches():
    assert FRAME_DESC.itemsize == 104 and FRAME_DESC.fields["scale_x"][1] == 64
    big = torch.zeros((90, 200, 3), dtype=torch.uint8)
    crop = big[10:70, 20:120]
    f = Frame.rgb(crop)
    assert f.shape == (60, 100, 3) and f.format == RGB24 and Frame.rgb(crop, bgr=True).format == BGR24
    d, _ = frame_table([f], 128)
    assert d["plane0"][0] == big.data_ptr() + 10 * 600 + 20 * 3 == crop.data_ptr() and d["pitch0"][0] == 600
    assert (d["h"][0], d["w"][0], d["format"][0]) == (60, 100, RGB24) and d["plane1"][0] == 0 and d["cy"][0] == 0
    # a numpy image is described in place as well (the call uploads it)
    img = np.zeros((8, 6, 3), np.uint8)
    d, _ = frame_table([Frame.rgb(img)], 128)
    assert d["plane0"][0] == img.ctypes.data and d["pitch0"][0] == 18
    # one decoder surface: UV behind the Y plane, or where the decoder says
    y, u, v = _planes(36, 64)
    rng = np.random.default_rng(1)
    for pitch, off in ((70, None), (256, None), (70, 70 * 48)):
        buf = torch.from_numpy(R.nv12_surface(y, u, v, pitch, pitch * 36 if off is None else off, rng))
        f = Frame.nv12_surface(buf, 36, 64, pitch, off, matrix="bt709")
        d, _ = frame_table([f], 128)
        assert d["plane0"][0] == buf.data_ptr() and d["plane1"][0] == buf.data_ptr() + (pitch * 36 if off is None else off)
        assert (d["pitch0"][0], d["pitch12"][0], d["format"][0]) == (pitch, pitch, NV12)
        assert tuple(d[k][0] for k in ("yoff", "cy", "cvr", "cvg", "cug", "cub")) == matrix_coeffs("bt709")
        np.testing.assert_array_equal(f.planes[0].numpy(), y)
        np.testing.assert_array_equal(f.planes[1].numpy().reshape(18, 32, 2)[..., 1], v)
    # separate planes with pitches of their own; uv as [h/2, w/2, 2] or [h/2, w]
    yb, cb = torch.zeros((36, 80), dtype=torch.uint8), torch.zeros((18, 96), dtype=torch.uint8)
    for uv in (cb[:, :64], cb[:, :64].unflatten(1, (32, 2))):
        d, _ = frame_table([Frame.nv12(yb[:, 8:72], uv)], 128)
        assert (d["plane0"][0], d["plane1"][0], d["pitch0"][0], d["pitch12"][0]) == (yb.data_ptr() + 8, cb.data_ptr(), 80, 96)
    ub, vb = torch.zeros((18, 40), dtype=torch.uint8), torch.zeros((18, 40), dtype=torch.uint8)
    d, _ = frame_table([Frame.i420(yb[:, :64], ub[:, 3:35], vb[:, :32])], 128)
    assert (d["plane1"][0], d["plane2"][0], d["pitch12"][0], d["format"][0]) == (ub.data_ptr() + 3, vb.data_ptr(), 40, I420)
    # cv2's packed host layouts
    for fmt in ("nv12", "i420"):
        arr = R.packed_yuv(y, u, v, fmt)
        f = Frame.from_host_yuv(arr, fmt)
        d, _ = frame_table([f], 128)
        assert d["plane0"][0] == arr.ctypes.data and d["plane1"][0] == arr.ctypes.data + 36 * 64 and f.nbytes == 36 * 64 * 3 // 2
        if fmt == "i420":
            assert d["plane2"][0] == arr.ctypes.data + 36 * 64 + 18 * 32 and d["pitch12"][0] == 32
            np.testing.assert_array_equal(f.planes[2].numpy(), v)


def test_frame_table_geometry_is_letterbox_tables():
    from object_detection_cib_amd.engine.rect import rect_canvas
    from object_detection_cib_amd.inference import letterbox_table
    shapes = [(72, 128), (36, 64), (300, 172), (128, 128), (2, 20), (42, 2)]
    frames = [Frame.nv12(torch.zeros((h, w), dtype=torch.uint8), torch.zeros((h // 2, w), dtype=torch.uint8)) for h, w in shapes]
    for canvas in (None, rect_canvas(shapes[:2], 128), (128, 128)):
        part = frames[:2] if canvas == (96, 128) else frames
        assert canvas in (None, (96, 128), (128, 128))
        want_d, want_b = letterbox_table([f.shape[:2] for f in part], 128, 3, canvas)
        got_d, got_b = frame_table(part, 128, 3, canvas)
        for k in ("h", "w", "nh", "nw", "top", "left", "scale_x", "scale_y"):
            np.testing.assert_array_equal(got_d[k], want_d[k], err_msg=k)
        np.testing.assert_array_equal(got_b, want_b)
    with pytest.raises(ValueError, match="image 5"):               # letterbox_table's own errors keep the index
        frame_table([Frame.rgb(np.zeros((1, 400, 3), np.uint8))], 128, 5)


def test_bad_frames_raise_by_index():
    from object_detection_cib_amd.inference import _check_images
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    bad = {
        "dtype": Frame.rgb(torch.zeros((4, 4, 3))),
        "int16": Frame.nv12(np.zeros((4, 4), np.int16), np.zeros((2, 4), np.uint8)),
        r"\[h, w, 3\]": Frame.rgb(u8(4, 4, 4)),
        "strides": Frame.rgb(u8(4, 3, 4).permute(0, 2, 1)),
        "even": Frame.nv12(u8(5, 4), u8(2, 4)),
        "even height and width": Frame.i420(u8(4, 6)[:, :5], u8(2, 2), u8(2, 2)),
        "uv: shape": Frame.nv12(u8(4, 4), u8(2, 2)),
        r"uv: shape \(2, 2, 3\)": Frame.nv12(u8(4, 4), u8(2, 2, 3)),
        "u: shape": Frame.i420(u8(4, 4), u8(4, 2), u8(2, 2)),
        "one pitch": Frame.i420(u8(8, 8), u8(4, 4), u8(4, 6)[:, :4]),
        "last-dimension stride": Frame.nv12(u8(4, 8)[:, ::2], u8(2, 4)),
        "pitch 3 below": Frame.nv12_surface(u8(100), 4, 4, 3),
        "pitch 0 below": Frame.nv12(u8(1, 4).expand(4, 4), u8(2, 4)),
        "uv_offset": Frame.nv12_surface(u8(100), 4, 4, 8, uv_offset=16),
        "bytes": Frame.nv12_surface(u8(43), 4, 4, 8),
        "bt2020": Frame.nv12(u8(4, 4), u8(2, 4), matrix="bt2020"),
        "fmt": Frame.from_host_yuv(np.zeros((6, 4), np.uint8), "yuy2"),
        r"h \* 3 / 2": Frame.from_host_yuv(np.zeros((7, 4), np.uint8), "nv12"),
        "numpy": Frame.from_host_yuv(u8(6, 4), "nv12"),
    }
    good = Frame.nv12_surface(u8(44), 4, 4, 8)
    assert good.error is None and Frame.nv12_surface(u8(100), 4, 4, 8, uv_offset=30).error is None
    for what, f in bad.items():
        with pytest.raises(ValueError, match=f"image 4: .*{what}"):
            frame_table([good, f], 128, 3)
        with pytest.raises(ValueError, match="image 1: "):
            _check_images([np.zeros((4, 4, 3), np.uint8), f, good])
    with pytest.raises(ValueError, match="image 2: expected an HWC uint8 array"):
        _check_images([good, np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8)])
    # device frames must lie on the detector's device; planes in host memory are the call's to upload
    _check_images([good], torch.device("cuda", 0))
    meta = Frame.rgb(torch.zeros((4, 4, 3), dtype=torch.uint8, device="meta"))
    with pytest.raises(ValueError, match="image 0: frame on meta, the detector on cuda:0"):
        _check_images([meta], torch.device("cuda", 0))
    with pytest.raises(ValueError, match="image 0: planes on different devices"):
        Frame(NV12, 4, 4, (u8(4, 4), torch.zeros((2, 4), dtype=torch.uint8, device="meta"))).check(0)


def test_launcher_argument_checks_need_no_gpu():
    from object_detection_cib_amd import _lib
    h = _lib.lib()
    assert h.kodhip_version() >= 111 and h.kodhip_frame_desc_bytes() == FRAME_DESC.itemsize
    for args in ((None, 64, None, 1, 64, 64), (64, None, None, 1, 64, 64), (64, 64, None, 0, 64, 64), (64, 64, None, 65536, 64, 64),
                 (64, 64, None, 1, 64, 63), (64, 64, None, 1, 0, 64), (64, 64, None, 1, 1 << 16, 1 << 15), (64, 68, None, 1, 64, 64),
                 (64, None, 72, 1, 64, 64)):
        assert h.kodhip_letterbox_frames(*args, None) < 0, args
        assert b"letterbox_frames" in h.kodhip_last_error(), args
