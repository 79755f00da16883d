"""CPU checks of the second-stage crops: the numpy reference (tests/crops_reference.py) on cases worked out by hand, the crop
record's size, and the argument checks of kodhip_crop_plan / kodhip_crop_batch (refused before any launch, so testable without
a GPU; the pointers are never dereferenced)."""
import ctypes as C

import numpy as np
import pytest

import crops_reference as R

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------------------ rectangle
def test_apply_classifier_numbers_by_hand():
    # 100 x 60 box centred on (150, 120) in a 300 x 400 image: square -> 100; 100 * fp32(1.3) = 129.999995..., 4.8e-6 below 130
    # with fp32 steps of 1.5e-5 there -> 130; + 30 = 160; half of it to each side of the centre
    rects, valid = R.crop_rects([[100, 90, 200, 150, 0.9, 3]], (300, 400))
    assert valid.tolist() == [True] and rects.tolist() == [[70, 40, 160, 160]]
    # the same box in a 190 x 210 image is clipped right and below: x 70..210, y 40..190
    assert R.crop_rects([[100, 90, 200, 150]], (190, 210))[0].tolist() == [[70, 40, 140, 150]]
    # save_one_box's options keep the aspect: 100 * fp32(1.02) = 101.99999809..., a quarter step below 102 -> 102; + 10 = 112 wide,
    # 60 * fp32(1.02) = 61.199998... (the fp32 next to 61.2) + 10 = 71.2 high: x 94..206, y 84.4..155.6 -> int() 84 and 155
    rects, valid = R.crop_rects([[100, 90, 200, 150]], (300, 400), square=False, gain=1.02, pad=10)
    assert valid.tolist() == [True] and rects.tolist() == [[94, 84, 112, 71]]
    # fractions are cut toward zero on both edges: x 10.7..20.9 -> 10 and 20
    assert R.crop_rects([[10.7, 5.2, 20.9, 9.9]], (50, 50), square=False, gain=1.0, pad=0)[0].tolist() == [[10, 5, 10, 4]]


def test_borders_outside_and_nan():
    rows = [[-10.5, 20, 30.7, 40], [10, -5, 20, 9.9], [150.2, 10, 250, 30], [10, 90.9, 20, 130],       # left, top, right, bottom
            [210, 10, 230, 30], [10, -40, 20, -1], [NAN, 10, 20, 30], [10, 10, INF, 30], [30, 30, 10, 10],
            [-3e38, 0, 3e38, 50]]
    rects, valid = R.crop_rects(rows, (100, 200), square=False, gain=1.0, pad=0)
    assert rects[:4].tolist() == [[0, 20, 30, 20], [10, 0, 10, 9], [150, 10, 50, 20], [10, 90, 10, 10]]
    # wholly outside (right of, above), NaN, inf, a reversed box: empty, the rectangle zeroed
    assert valid.tolist() == [True] * 4 + [False] * 5 + [True]
    assert (rects[4:9] == 0).all()
    # a width that overflows fp32 around a finite centre is -inf .. inf, clipped to the image; around an overflowed centre the
    # edge is inf - inf: empty
    assert rects[9].tolist() == [0, 0, 200, 50]
    assert R.crop_rects([[2e38, 0, 3e38, 50]], (100, 200), square=False, gain=10.0, pad=0)[1].tolist() == [False]
    # pad alone can make an inverted box non-empty, as in YOLOv5
    assert R.crop_rects([[30, 30, 28, 28]], (100, 200), square=False, gain=1.0, pad=10)[0].tolist() == [[25, 25, 8, 8]]     # centre 29, width -2 + 10
    # one shape per row
    rects, valid = R.crop_rects([[0, 0, 500, 500], [0, 0, 500, 500]], [(10, 20), (30, 40)], square=False, gain=1.0, pad=0)
    assert rects.tolist() == [[0, 0, 20, 10], [0, 0, 40, 30]]


# ------------------------------------------------------------------------------------------------------------- geometry
def test_letterbox_geometry_by_hand():
    g = lambda cw, ch, mode="letterbox": R.crop_geometry(cw, ch, 8, 16, mode)
    assert g(30, 10)[:4] == (5, 16, 1, 0)            # 3:1: r = 16/30, 10 r = 5.33 -> 5 rows, one grey row above, two below
    assert g(10, 30)[:4] == (8, 3, 0, 6)             # 1:3: r = 8/30, 10 r = 2.67 -> 3 columns, 6 grey ones to the left, 7 right
    assert g(5, 16)[:4] == (8, 2, 0, 7)              # r = 1/2: 2.5 columns -> 2 (half to even)
    assert g(7, 16)[:4] == (8, 4, 0, 6)              # 3.5 -> 4
    assert g(1000, 1)[:4] == (1, 16, 3, 0)           # 0.016 rows -> at least one
    assert g(30, 10)[4:] == (1.0 / (16 / 30.0), 1.0 / (5 / 10.0))
    assert g(30, 10, "stretch") == (8, 16, 0, 0, 1.0 / (16 / 30.0), 1.0 / (8 / 10.0))


def test_crop_ref_slices_pastes_and_normalises():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    # a stretch at the crop's own size returns the slice
    x, u8 = R.crop_ref(img, (5, 7, 16, 8), True, 8, 16)
    np.testing.assert_array_equal(u8, img[7:15, 5:21])
    np.testing.assert_array_equal(x, (img[7:15, 5:21].astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
    # an empty crop is all pad; bgr swaps the channels, mean / std apply in the output's order
    x, u8 = R.crop_ref(img, (0, 0, 0, 0), False, 4, 4)
    assert (u8 == 114).all() and (x == np.float32(114) / np.float32(255)).all()
    mean, std = (0.5, 0.25, 0.125), (0.5, 2.0, 4.0)
    xb, ub = R.crop_ref(img, (5, 7, 16, 8), True, 8, 16, bgr=True, mean=mean, std=std)
    np.testing.assert_array_equal(ub, img[7:15, 5:21, ::-1])
    plain = ub.astype(np.float32) / np.float32(255)
    np.testing.assert_array_equal(xb[2], (plain[..., 2] - np.float32(0.125)) / np.float32(4.0))
    # letterbox of a 3:1 cutout: the resize of the cutout alone between grey rows
    x, u8 = R.crop_ref(img, (0, 0, 30, 10), True, 8, 16, mode="letterbox")
    assert (u8[0] == 114).all() and (u8[6:] == 114).all()
    np.testing.assert_array_equal(u8[1:6], R.resize_linear_u8(img[:10], 16, 5))
    # a tap outside the cutout would change the result: the cutout's last column is resized without its neighbour
    wide = R.crop_ref(img, (0, 0, 12, 10), True, 4, 5)[1]
    other = img.copy()
    other[:, 12:] ^= 255
    np.testing.assert_array_equal(R.crop_ref(other, (0, 0, 12, 10), True, 4, 5)[1], wide)


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_crop_record_size():
    from object_detection_cib_amd import _lib
    from object_detection_cib_amd.core.crops import CROP_DESC
    h = _lib.lib()
    assert h.kodhip_version() >= 117
    assert h.kodhip_crop_desc_bytes() == CROP_DESC.itemsize == 56


def test_launchers_refuse_bad_arguments_without_a_gpu():
    from object_detection_cib_amd import _lib
    h = _lib.lib()
    p = 4096                                                                 # (never dereferenced: every call is refused)
    good = dict(frames=p, B=2, rows=p, row_stride=6, row_index=p, frame_index=p, N=3, out_h=8, out_w=16, mode=0, square=1, gain=1.3,
                pad=30.0, crops=p, rects=None)
    bad = [(dict(frames=None), "null"), (dict(rows=None), "null"), (dict(row_index=None), "null"), (dict(frame_index=None), "null"),
           (dict(crops=None), "null"), (dict(out_h=0), "out_h"), (dict(out_h=1025), "out_h"), (dict(out_w=0), "out_w"),
           (dict(out_w=1025), "out_w"), (dict(N=0), "N "), (dict(N=65536), "N "), (dict(B=0), "B "), (dict(B=65536), "B "),
           (dict(row_stride=3), "row_stride"), (dict(gain=0.0), "gain"), (dict(gain=-1.0), "gain"), (dict(gain=NAN), "gain"),
           (dict(gain=INF), "gain"), (dict(pad=-1.0), "pad"), (dict(pad=NAN), "pad"), (dict(pad=INF), "pad"), (dict(mode=2), "mode"),
           (dict(mode=-1), "mode")]
    for kw, msg in bad:
        a = dict(good, **kw)
        rc = h.kodhip_crop_plan(*[a[k] for k in good], None)
        err = h.kodhip_last_error().decode()
        assert rc < 0 and "crop_plan" in err and msg in err, (kw, rc, err)

    def norm(*v):
        return (C.c_float * 6)(*v)
    good = dict(frames=p, B=2, crops=p, N=3, out_f32=p, out_u8=None, out_h=8, out_w=16, bgr=0, mean_std=None)
    bad = [(dict(frames=None), "null"), (dict(crops=None), "null"), (dict(out_f32=None), "at least one output"), (dict(out_h=0), "out_h"),
           (dict(out_h=1025), "out_h"), (dict(out_w=0), "out_w"), (dict(out_w=1025), "out_w"), (dict(N=0), "N "),
           (dict(N=65536), "N "), (dict(B=0), "B "), (dict(B=65536), "B "),
           (dict(mean_std=norm(0, 0, 0, 1, 0, 1)), "std[1]"), (dict(mean_std=norm(0, 0, 0, 1, 1, NAN)), "std[2]"),
           (dict(mean_std=norm(0, 0, 0, INF, 1, 1)), "std[0]"), (dict(mean_std=norm(0, NAN, 0, 1, 1, 1)), "mean[1]")]
    for kw, msg in bad:
        a = dict(good, **kw)
        rc = h.kodhip_crop_batch(*[a[k] for k in good], None)
        err = h.kodhip_last_error().decode()
        assert rc < 0 and "crop_batch" in err and msg in err, (kw, rc, err)


def test_options_name_the_bad_argument():
    from object_detection_cib_amd.core.crops import CropOptions
    for kw, name in ((dict(size=(0, 8)), "size"), (dict(size=(8, 1025)), "size"), (dict(size=(8,)), "size"), (dict(size="ab"), "size"),
                     (dict(mode="fit"), "mode"), (dict(gain=0), "gain"), (dict(gain=NAN), "gain"), (dict(pad=-1), "pad"),
                     (dict(pad=INF), "pad"), (dict(max_crops=0), "max_crops"), (dict(mean=(0, 0, 0)), "std"), (dict(std=(1, 1, 1)), "mean"),
                     (dict(mean=(0, 0), std=(1, 1, 1)), "mean"), (dict(mean=(0, 0, 0), std=(1, 0, 1)), "std"),
                     (dict(mean=(0, 0, 0), std=(1, NAN, 1)), "std")):
        with pytest.raises(ValueError, match=f"^{name}"):
            CropOptions(**kw)
    o = CropOptions(16, mode="letterbox", mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
    assert (o.h, o.w, o.mode, o.square, o.gain, o.pad) == (16, 16, 1, True, 1.3, 30.0) and list(o.mean_std)[3] == np.float32(0.229)
