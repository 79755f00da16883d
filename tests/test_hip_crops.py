"""Second-stage crops on the device: kodhip_crop_plan / kodhip_crop_batch (csrc/crops.hip) through the C ABI, `crop_detections`,
`Detector.detect_crops` and `ClassifiedDetector` against tests/crops_reference.py - the rectangle in np.float32, the cutout of
the RGB image (for 4:2:0 sources: `frames_reference.yuv420_to_rgb` of the whole frame), oracle resize_linear_u8 of the cutout
alone, 114 around it, / 255, normalise.

Everything is compared exactly: rectangles, valid flags and uint8 crops with np.array_equal, the fp32 crops on their bit
patterns.  The rectangle is a handful of fp32 operations rounded once each, the resize is integer arithmetic, and the two or
four fp32 operations behind it are correctly rounded on both sides.  Figures are printed before they are asserted (`pytest -s`).

Measured on an MI355X: every comparison exact; the seven detector images keep 13 - 54 rows each (17 - 74 augmented); the stub
classifier sees 188 crops, none empty, and agrees with the detector's class on 45 of them; at gain 0.02 50 of the 188 crops are
empty; the 31 tests take about 3 s.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import crops_reference as C  # noqa: E402
import frames_reference as R  # noqa: E402
import fusion_helpers as F  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core import crops as K  # noqa: E402
from object_detection_cib_amd.core.crops import CROP_DESC, crop_detections  # noqa: E402
from object_detection_cib_amd.core.nms import PackedDetections  # noqa: E402
from object_detection_cib_amd.data.frames import FRAME_DESC, Frame, frame_records, matrix_coeffs  # noqa: E402
from test_hip_frames import SIZES, _kth_score, _make_frame, _surface, _yuv  # noqa: E402
from test_hip_rect import ANCH, BATCH, IOU, S, _bits, _np, _same_rows  # noqa: E402

DEV = "cuda"
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ----------------------------------------------------------------------------------------------------------------- kernel
SRC_SIZES = ((38, 54), (64, 48))               # h x w, even: 4:2:0 frames
# (frame, left edge, top edge, width, height) of the rectangle BEFORE the clip, edges at .5 so that int() is far from a tie:
VIRTUAL = (
    (0, 10.5, 8.5, 20, 14),                    # interior
    (0, -6.5, 10.5, 16, 12), (0, 20.5, -5.5, 12, 16), (1, 40.5, 20.5, 16, 10), (1, 10.5, 55.5, 10, 16),   # left, top, right, bottom
    (0, 60.5, 10.5, 8, 8), (1, 5.5, -30.5, 8, 8),                                                        # outside: empty
    (0, 53.5, 12.5, 10, 10), (1, 14.5, 63.5, 10, 10),                  # one column / one row is left inside the frame
    (0, 25.5, 5.5, 1, 12), (1, 6.5, 30.5, 12, 1),                      # 1 pixel wide / high by itself (square: 12 x 12)
    (0, 11.5, 9.5, 16, 16), (1, 7.5, 13.5, 8, 8),                      # exactly 16 x 16 and 8 x 8, odd origins: the copy path
    (1, 9.5, 21.5, 16, 8), (0, 5.5, -7.5, 16, 16),                     # 16 x 8 (the second one through the clip, also when squared)
    (0, 30.5, 20.5, 5, 7),                                             # upscale
    (0, 2.5, 4.5, 50, 30),                                             # downscale
)
OUTS = ((16, 16), (8, 8), (8, 16))             # out_h x out_w


def _rows_for(gain, pad):
    """the detection rows whose rectangles (before clip and square) are VIRTUAL under (gain, pad): [N, 6] fp32, frame per row"""
    rows = []
    for k, ax, ay, w, h in VIRTUAL:
        cx, cy, bw, bh = ax + w / 2.0, ay + h / 2.0, (w - pad) / gain, (h - pad) / gain
        rows.append([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2, 0.5, 1.0])
    rows.append([float("nan"), 1.0, 5.0, 9.0, 0.5, 1.0])
    return np.float32(rows), np.int32([v[0] for v in VIRTUAL] + [1])


def _launch(frames, rows, stride, row_index, frame_index, out, mode, square, gain, pad, bgr=False, norm=None, f32=True, u8=True):
    """kodhip_crop_plan + kodhip_crop_batch -> (crop records, rects [N, 4], fp32 [N, 3, h, w] | None, uint8 [N, h, w, 3] | None)"""
    h = _lib.lib()
    assert h.kodhip_crop_desc_bytes() == CROP_DESC.itemsize and h.kodhip_frame_desc_bytes() == FRAME_DESC.itemsize
    N, (oh, ow) = len(row_index), out
    f_dev = torch.from_numpy(frame_records(frames).view(np.uint8)).to(DEV)
    ri, fi = torch.from_numpy(np.int32(row_index)).to(DEV), torch.from_numpy(np.int32(frame_index)).to(DEV)
    recs = torch.full((N * CROP_DESC.itemsize,), 0xEE, dtype=torch.uint8, device=DEV)
    rects = torch.full((N, 4), -7, dtype=torch.int32, device=DEV)
    x = torch.full((N, 3, oh, ow), -7.0, device=DEV) if f32 else None
    b = torch.full((N, oh, ow, 3), 7, dtype=torch.uint8, device=DEV) if u8 else None
    ms = (_lib.f32 * 6)(*norm[0], *norm[1]) if norm is not None else None
    _lib.check(h.kodhip_crop_plan(f_dev.data_ptr(), len(frames), rows.data_ptr(), stride, ri.data_ptr(), fi.data_ptr(), N, oh, ow, mode,
                                  int(square), gain, pad, recs.data_ptr(), rects.data_ptr(), stream()), "crop_plan")
    _lib.check(h.kodhip_crop_batch(f_dev.data_ptr(), len(frames), recs.data_ptr(), N, x.data_ptr() if f32 else None,
                                   b.data_ptr() if u8 else None, oh, ow, int(bgr), ms, stream()), "crop_batch")
    torch.cuda.synchronize()
    return (recs.cpu().numpy().view(CROP_DESC), rects.cpu().numpy(), x.cpu().numpy() if f32 else None, b.cpu().numpy() if u8 else None)


@pytest.fixture(scope="module")
def src_yuvs():
    rng = np.random.default_rng(31)
    return [_yuv(h, w, rng) for h, w in SRC_SIZES]


@pytest.mark.parametrize("square", [False, True])
@pytest.mark.parametrize("mode", ["stretch", "letterbox"])
@pytest.mark.parametrize("fmt", ["rgb", "bgr", "nv12", "i420"])
def test_kernel_equals_numpy_bit_for_bit(src_yuvs, fmt, mode, square):
    made = [[_make_frame(fmt, "bt601", yuv, k + 1, np.random.default_rng(fill)) for k, yuv in enumerate(src_yuvs)] for fill in (1, 2)]
    frames, rgbs = [m[0] for m in made[0]], [m[1] for m in made[0]]
    assert all(f.pitches[0] > (3 * f.w if fmt in ("rgb", "bgr") else f.w) for f in frames)
    assert rgbs[0].std() > 80                                           # high contrast: a tap outside the cutout shows
    # (norm, bgr, rows in a gapped [B, max_det, 6] buffer | dense [N, 6])
    variants = ((None, False, True), ((MEAN, STD), False, False), (None, True, False), ((MEAN, STD), True, True))
    seen, m = set(), {"stretch": 0, "letterbox": 1}[mode]
    for gain, pad in ((1.3, 30.0), (1.02, 10.0)):
        rows, fidx = _rows_for(gain, pad)
        order = np.argsort(fidx, kind="stable")                          # image-major, as a packed buffer holds them
        rows, fidx = rows[order], fidx[order]
        N, counts = len(rows), np.bincount(fidx, minlength=2)
        max_det = int(counts.max()) + 3
        gapped = np.full((2, max_det, 6), 1e30, np.float32)
        gidx = []
        for k in range(2):
            gapped[k, :counts[k]] = rows[fidx == k]
            gidx += [k * max_det + j for j in range(counts[k])]
        g_dev, d_dev = torch.from_numpy(gapped).to(DEV), torch.from_numpy(rows).to(DEV)
        want_rects, want_valid = C.crop_rects(rows, [SRC_SIZES[k] for k in fidx], square, gain, pad)
        nonempty = [tuple(r[2:]) for r, v in zip(want_rects, want_valid) if v]
        print(f"CROPS kernel {fmt} {mode} square {square} gain {gain} pad {pad}: rects {want_rects.tolist()}")
        # the conditions on the hand-made rows: empty and non-empty crops, 1-pixel crops, odd origins, every copy path
        assert (~want_valid).sum() >= 3 and len(nonempty) >= 6
        assert any(w == 1 for w, h in nonempty) and any(h == 1 for w, h in nonempty)
        assert any(v and r[0] % 2 and r[1] % 2 for r, v in zip(want_rects, want_valid))
        assert all((ow, oh) in nonempty for oh, ow in OUTS)
        assert any(w < 8 and h < 8 for w, h in nonempty) and any(w > 16 and h > 16 for w, h in nonempty)
        assert any(r[0] == 0 for r in want_rects[want_valid]) and any(r[1] == 0 for r in want_rects[want_valid])
        assert any(r[0] + r[2] == SRC_SIZES[k][1] for r, k in zip(want_rects[want_valid], fidx[want_valid]))
        assert any(r[1] + r[3] == SRC_SIZES[k][0] for r, k in zip(want_rects[want_valid], fidx[want_valid]))
        for out in OUTS:
            for norm, bgr, gap in variants:
                args = (g_dev, 6, gidx) if gap else (d_dev, 6, np.arange(N))
                recs, rects, x, u8 = _launch(frames, *args, fidx, out, m, square, gain, pad, bgr, norm)
                np.testing.assert_array_equal(rects, want_rects)
                np.testing.assert_array_equal(recs["valid"] != 0, want_valid)
                np.testing.assert_array_equal(recs["frame"], fidx)
                for rec, (x0, y0, cw, ch), v in zip(recs, want_rects, want_valid):
                    if v:
                        nh, nw, top, left, sx, sy = C.crop_geometry(cw, ch, *out, mode)
                        got = tuple(int(rec[n]) for n in ("x0", "y0", "w", "h", "nh", "nw", "top", "left"))
                        assert got == (x0, y0, cw, ch, nh, nw, top, left)
                        assert (float(rec["scale_x"]), float(rec["scale_y"])) == (sx, sy)
                        seen.add("copy" if (nh, nw) == (ch, cw) else "up" if nh > ch else "down")
                wx, wu = [np.stack(a) for a in zip(*[C.crop_ref(rgbs[k], r, v, *out, mode, bgr, *(norm or (None, None)))
                                                     for k, r, v in zip(fidx, want_rects, want_valid)])]
                np.testing.assert_array_equal(u8, wu)
                np.testing.assert_array_equal(_bits(x), _bits(wx))
                assert (u8[~want_valid] == 114).all()
        # each output alone, and the padding between the rows (another fill) does not reach the output
        recs, rects, x1, _ = _launch(frames, d_dev, 6, np.arange(N), fidx, (8, 16), m, square, gain, pad, u8=False)
        _, _, _, u1 = _launch([f for f, _ in made[1]], d_dev, 6, np.arange(N), fidx, (8, 16), m, square, gain, pad, f32=False)
        recs, rects, x2, u2 = _launch(frames, d_dev, 6, np.arange(N), fidx, (8, 16), m, square, gain, pad)
        np.testing.assert_array_equal(_bits(x1), _bits(x2))
        np.testing.assert_array_equal(u1, u2)
    assert seen == {"copy", "up", "down"}


def test_rows_with_stride_four_and_frames_in_any_order(src_yuvs):
    """a dense [N, 4] buffer (the smallest stride), crops of the two frames interleaved, a frame index outside the table"""
    made = [_make_frame("nv12", "bt709", yuv, k, np.random.default_rng(4)) for k, yuv in enumerate(src_yuvs)]
    rgbs = [R.yuv420_to_rgb(*yuv, matrix_coeffs("bt709")) for yuv in src_yuvs]
    rows, fidx = _rows_for(1.02, 10.0)
    d_dev = torch.from_numpy(np.ascontiguousarray(rows[:, :4])).to(DEV)
    ridx = np.arange(len(rows))[::-1].copy()
    fi = fidx[::-1].copy()
    recs, rects, x, u8 = _launch([m[0] for m in made], d_dev, 4, ridx, fi, (16, 16), 1, False, 1.02, 10.0)
    want_rects, want_valid, wx, wu = C.crops_ref(rgbs, rows[ridx], fi, 16, 16, "letterbox", False, 1.02, 10.0)
    np.testing.assert_array_equal(rects, want_rects)
    np.testing.assert_array_equal(_bits(x), _bits(wx))
    np.testing.assert_array_equal(u8, wu)
    bad = fi.copy()
    bad[0], bad[1] = 2, -1
    recs, rects, x, u8 = _launch([m[0] for m in made], d_dev, 4, ridx, bad, (16, 16), 1, False, 1.02, 10.0)
    assert (recs["valid"][:2] == 0).all() and (rects[:2] == 0).all() and (u8[:2] == 114).all()
    np.testing.assert_array_equal(u8[2:], wu[2:])


def test_launchers_refuse_bad_arguments_and_launch_nothing():
    x = torch.full((2, 3, 8, 8), -7.0, device=DEV)
    recs = torch.full((2 * CROP_DESC.itemsize,), 0xEE, dtype=torch.uint8, device=DEV)
    h = _lib.lib()
    p = recs.data_ptr()
    for args in ((p, 1, p, 3, p, p, 2, 8, 8, 0, 1, 1.3, 30.0, p, None), (p, 1, p, 6, p, p, 2, 8, 8, 2, 1, 1.3, 30.0, p, None),
                 (p, 1, p, 6, p, p, 2, 8, 8, 0, 1, 0.0, 30.0, p, None), (p, 1, p, 6, p, p, 2, 8, 2000, 0, 1, 1.3, 30.0, p, None)):
        assert h.kodhip_crop_plan(*args, stream()) < 0 and b"crop_plan" in h.kodhip_last_error()
    for args in ((p, 1, p, 2, None, None, 8, 8, 0, None), (p, 1, p, 0, x.data_ptr(), None, 8, 8, 0, None),
                 (p, 1, p, 2, x.data_ptr(), None, 8, 8, 0, (_lib.f32 * 6)(0, 0, 0, 1, 0, 1))):
        assert h.kodhip_crop_batch(*args, stream()) < 0 and b"crop_batch" in h.kodhip_last_error()
    torch.cuda.synchronize()
    assert bool((x == -7.0).all()) and bool((recs == 0xEE).all())


# ---------------------------------------------------------------------------------------------------------------- wrapper
def _dets(rows, fidx, n):
    return [torch.from_numpy(np.ascontiguousarray(rows[fidx == k])).to(DEV) for k in range(n)]


def _check_result(res, rgbs, dets, size, tag, limit=None, u8=True, **kw):
    for i, (im, d) in enumerate(zip(rgbs, dets)):
        rows = d.cpu().numpy()[:limit]
        wr, wv, wx, wu = C.crops_ref([im], rows, [0] * len(rows), *size, **kw)
        np.testing.assert_array_equal(res.rects[i].cpu().numpy(), wr, err_msg=f"{tag} rects {i}")
        np.testing.assert_array_equal(res.valid[i].cpu().numpy(), wv, err_msg=f"{tag} valid {i}")
        np.testing.assert_array_equal(_bits(res.crops[i].cpu().numpy()), _bits(wx), err_msg=f"{tag} crops {i}")
        if u8:
            np.testing.assert_array_equal(res.u8[i].cpu().numpy(), wu, err_msg=f"{tag} u8 {i}")


def test_crop_detections_mixed_sources(src_yuvs):
    rgbs = [R.yuv420_to_rgb(*yuv, matrix_coeffs("bt601")) for yuv in src_yuvs]
    rows, fidx = _rows_for(1.3, 30.0)
    # four sources: a numpy image, an NV12 surface on the device, a host I420 frame, a BGR tensor on the device; then numpy again
    images = [rgbs[0], rgbs[1], rgbs[0], rgbs[1], rgbs[1]]
    sources = [rgbs[0], _surface(src_yuvs[1], 1), Frame.from_host_yuv(R.packed_yuv(*src_yuvs[0], "i420"), "i420"),
               Frame.rgb(torch.from_numpy(np.ascontiguousarray(rgbs[1][..., ::-1])).to(DEV), bgr=True), rgbs[1]]
    two = _dets(rows, fidx, 2)
    dets = [two[0], two[1], two[0][:3], two[1], torch.zeros((0, 6), device=DEV)]
    res = crop_detections(sources, dets, size=(8, 16), out_u8=True)
    assert [len(c) for c in res.crops] == [len(d) for d in dets] and res.crops[4].shape == (0, 3, 8, 16)
    _check_result(res, images, dets, (8, 16), "mixed")
    # the per-image results are views of one buffer
    base = res.crops[0].data_ptr()
    assert res.crops[1].data_ptr() == base + len(dets[0]) * 3 * 8 * 16 * 4
    # options; [n, 4] rows; max_crops takes each image's first rows
    kw = dict(mode="letterbox", square=False, gain=1.02, pad=10, bgr=True, mean=MEAN, std=STD)
    res = crop_detections(sources, [d[:, :4] for d in dets], size=(16, 16), max_crops=2, **kw)
    assert res.u8 is None and [len(c) for c in res.crops] == [2, 2, 2, 2, 0]
    _check_result(res, images, dets, (16, 16), "options", limit=2, u8=False, **kw)
    # a PackedDetections is read where it lies: rows beyond the counts are never looked at
    max_det = max(len(d) for d in dets) + 2
    packed = torch.full((5, max_det, 6), float("nan"), device=DEV)
    for b, d in enumerate(dets):
        packed[b, :len(d)] = d
    pd = PackedDetections([packed[b, :len(d)] for b, d in enumerate(dets)], packed, torch.tensor([len(d) for d in dets], dtype=torch.int32, device=DEV))
    res = crop_detections(sources, pd, size=(8, 16), out_u8=True)
    _check_result(res, images, dets, (8, 16), "packed")


def test_crop_detections_without_rows_launches_nothing(src_yuvs, monkeypatch):
    rgb = R.yuv420_to_rgb(*src_yuvs[0], matrix_coeffs("bt601"))

    def refuse(*a, **k):
        raise AssertionError("a call without rows uploads and launches nothing")
    monkeypatch.setattr(K, "launch_crops", refuse)
    monkeypatch.setattr(K, "ImagePool", refuse)
    monkeypatch.setattr(K, "upload_frames", refuse)
    res = crop_detections([rgb, rgb], [torch.zeros((0, 6), device=DEV)] * 2, size=(8, 16), out_u8=True)
    assert [tuple(t.shape) for t in res.crops] == [(0, 3, 8, 16)] * 2 and res.crops[0].dtype == torch.float32
    assert [tuple(t.shape) for t in res.u8] == [(0, 8, 16, 3)] * 2 and res.u8[0].dtype == torch.uint8
    assert [tuple(t.shape) for t in res.rects] == [(0, 4)] * 2 and res.rects[0].dtype == torch.int32
    assert [tuple(t.shape) for t in res.valid] == [(0,)] * 2 and res.valid[0].dtype == torch.bool
    res = crop_detections([], [])
    assert res.crops == [] and res.rects == [] and res.valid == []


def test_more_rows_than_one_launch_takes(src_yuvs):
    rgb = R.yuv420_to_rgb(*src_yuvs[0], matrix_coeffs("bt601"))
    n = K.MAX_LAUNCH + 9
    rows = torch.tensor([[10.0, 8.0, 30.0, 20.0, 0.5, 0.0]], device=DEV).repeat(n, 1)
    rows[K.MAX_LAUNCH - 1] = torch.tensor([200.0, 8.0, 230.0, 20.0, 0.5, 0.0])          # (an empty one on each side of the seam)
    rows[K.MAX_LAUNCH] = torch.tensor([2.0, 3.0, 7.0, 9.0, 0.5, 0.0])
    whole = crop_detections([rgb], [rows], size=(2, 2), out_u8=True)
    half = n // 2
    a = crop_detections([rgb], [rows[:half]], size=(2, 2), out_u8=True)
    b = crop_detections([rgb], [rows[half:]], size=(2, 2), out_u8=True)
    assert len(whole.crops[0]) == n
    for name in ("crops", "u8", "rects", "valid"):
        assert torch.equal(getattr(whole, name)[0], torch.cat((getattr(a, name)[0], getattr(b, name)[0]))), name
    wr, wv, wx, wu = C.crops_ref([rgb], rows[K.MAX_LAUNCH - 2:K.MAX_LAUNCH + 2].cpu().numpy(), [0] * 4, 2, 2)
    assert wv.tolist() == [True, False, True, True]
    np.testing.assert_array_equal(whole.rects[0][K.MAX_LAUNCH - 2:K.MAX_LAUNCH + 2].cpu().numpy(), wr)
    np.testing.assert_array_equal(_bits(whole.crops[0][K.MAX_LAUNCH - 2:K.MAX_LAUNCH + 2].cpu().numpy()), _bits(wx))


def test_crop_detections_value_errors(src_yuvs, monkeypatch):
    rgb = R.yuv420_to_rgb(*src_yuvs[0], matrix_coeffs("bt601"))
    d = torch.tensor([[10.0, 8.0, 30.0, 20.0, 0.5, 0.0]], device=DEV)

    def refuse(*a, **k):
        raise AssertionError("a refused call uploads and launches nothing")
    for name in ("launch_crops", "ImagePool", "upload_frames"):
        monkeypatch.setattr(K, name, refuse)
    bad_frame = Frame.nv12(torch.zeros((5, 4), dtype=torch.uint8, device=DEV), torch.zeros((2, 4), dtype=torch.uint8, device=DEV))
    for args, kw, match in ((([rgb, rgb], [d]), {}, "^detections: 1 entries for 2 sources"), (([rgb], [d]), dict(size=(0, 8)), "^size"),
                            (([rgb], [d]), dict(size=(8, 2000)), "^size"), (([rgb], [d]), dict(size=(8,)), "^size"),
                            (([rgb], [d]), dict(mean=MEAN), "^std"), (([rgb], [d]), dict(std=STD), "^mean"),
                            (([rgb], [d]), dict(mean=MEAN, std=(1, 0, 1)), "^std"), (([rgb], [d]), dict(mode="fit"), "^mode"),
                            (([rgb], [d]), dict(gain=0), "^gain"), (([rgb], [d]), dict(pad=-1), "^pad"),
                            (([rgb], [d]), dict(max_crops=0), "^max_crops"), (([rgb, bad_frame], [d, d]), {}, "^image 1: .*even"),
                            (([rgb, rgb[..., 0]], [d, d]), {}, "^image 1"), (([rgb], [d.cpu()]), {}, r"^detections\[0\]"),
                            (([rgb], [d[:, :3]]), {}, r"^detections\[0\]"), (([rgb], [d[0]]), {}, r"^detections\[0\]")):
        with pytest.raises(ValueError, match=match):
            crop_detections(*args, **kw)


# -------------------------------------------------------------------------------------------------------------- detectors
@pytest.fixture(scope="module")
def yuvs():
    rng = np.random.default_rng(9)
    return [_yuv(h, w, rng) for h, w in SIZES]


@pytest.fixture(scope="module")
def images(yuvs):
    return [R.yuv420_to_rgb(*yuv, matrix_coeffs("bt601")) for yuv in yuvs]


@pytest.fixture(scope="module")
def net():
    n = F.network(5, 0.25)
    n.fuse_eval(False)
    return n


@pytest.fixture(scope="module")
def conf(net, images):
    """a threshold that leaves about a dozen rows in the sparsest image, plain or augmented, square or rectangular"""
    from object_detection_cib_amd.inference import AugmentedDetector, Detector
    picks = []
    for cls in (Detector, AugmentedDetector):
        for rect in (False, True):
            picks.append(_kth_score(_np(cls(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=0.0, iou_thres=IOU).rectangular(rect)(images)), 12))
    return min(picks)


def _check_nonempty(want, tag):
    counts = [len(w) for w in want]
    print(f"CROPS {tag}: rows per image {counts}")
    assert sum(c >= 1 for c in counts) > len(counts) // 2, counts


@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("rect", [False, True])
def test_detect_crops_equals_call_and_reference(net, yuvs, images, conf, rect, graphed):
    from object_detection_cib_amd.inference import Detector
    mk = lambda: Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU, graphed=graphed).rectangular(rect)
    want = [r.clone() for r in mk()(images)]
    _check_nonempty(want, f"detector rect {rect} graphed {graphed}")
    det = mk()
    got = det.detect_crops(images, size=(16, 16), out_u8=True)
    assert isinstance(got, list) and len(got) == 7                     # batch 4: the second chunk is padded by one record
    _same_rows(_np(got), _np(want), "detect_crops rows")               # (in the caller's order: the images differ in size)
    _check_result(got, images, want, (16, 16), "detect_crops")
    # NV12 surfaces give the boxes and the crops of the RGB images they stand for; another option set on the same detector
    kw = dict(mode="letterbox", square=False, gain=1.02, pad=10, mean=MEAN, std=STD)
    got = det.detect_crops([_surface(yuv, k) for k, yuv in enumerate(yuvs)], size=(8, 16), max_crops=5, **kw)
    _same_rows(_np(got), _np(want), "nv12 rows")
    assert got.u8 is None and [len(c) for c in got.crops] == [min(len(w), 5) for w in want]
    _check_result(got, images, want, (8, 16), "nv12", limit=5, u8=False, **kw)
    # and __call__ answers as before on the same object
    _same_rows(_np(det(images)), _np(want), "call after detect_crops")
    with pytest.raises(ValueError, match="^size"):
        det.detect_crops(images, size=(0, 16))
    with pytest.raises(ValueError, match="^image 1"):
        det.detect_crops([images[0], images[1][..., 0]])


def test_detect_crops_augmented(net, yuvs, images, conf):
    from object_detection_cib_amd.inference import AugmentedDetector
    det = AugmentedDetector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU).rectangular()
    want = [r.clone() for r in det(images)]
    _check_nonempty(want, "augmented")
    mixed = [images[0], _surface(yuvs[1], 1), Frame.from_host_yuv(R.packed_yuv(*yuvs[2], "i420"), "i420"), images[3], images[4],
             _surface(yuvs[5], 0), Frame.rgb(np.ascontiguousarray(images[6][..., ::-1]), bgr=True)]
    got = det.detect_crops(mixed, size=(16, 16), bgr=True, out_u8=True)
    _same_rows(_np(got), _np(want), "augmented rows")
    _check_result(got, images, want, (16, 16), "augmented", bgr=True)


def test_detect_crops_on_images_without_rows(net, images):
    from object_detection_cib_amd.inference import Detector
    det = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=1.0, iou_thres=IOU)             # (no score is above 1)
    got = det.detect_crops(images[:5], size=(8, 16), out_u8=True)
    assert [len(g) for g in got] == [0] * 5
    assert [tuple(c.shape) for c in got.crops] == [(0, 3, 8, 16)] * 5 and [tuple(c.shape) for c in got.u8] == [(0, 8, 16, 3)] * 5
    assert [tuple(c.shape) for c in got.rects] == [(0, 4)] * 5 and [tuple(c.shape) for c in got.valid] == [(0,)] * 5


# -------------------------------------------------------------------------------------------------------------- classifier
def _stub(x):
    """three scores from three fixed pixels of the crop, elementwise operations only: the same bits for the same crop whatever
    the batch it arrives in"""
    v = (x[:, 0, 2, 3] + x[:, 1, 8, 8] + x[:, 2, 13, 5]) * (1.0 / 3.0)
    centres = torch.tensor([0.2, 0.5, 0.8], device=x.device)
    return -(v[:, None] - centres[None, :]).abs()


def _want_cls2(images, want, **kw):
    """per image: (the stub's class on the reference crops uploaded to the device, valid)"""
    out = []
    for im, rows in zip(images, _np(want)):
        _, wv, wx, _ = C.crops_ref([im], rows, [0] * len(rows), 16, 16, **kw)
        c = _stub(torch.from_numpy(wx).to(DEV)).argmax(dim=1).cpu().numpy() if len(rows) else np.zeros(0, np.int64)
        out.append((np.where(wv, c, -1), wv))
    return out


@pytest.mark.parametrize("options", [{}, dict(square=False, gain=0.02, pad=0)])
def test_classified_detector(net, yuvs, images, conf, options):
    from object_detection_cib_amd.inference import ClassifiedDetector, Detector
    want = [r.clone() for r in Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU)(images)]
    _check_nonempty(want, "classified")
    ref = _want_cls2(images, want, **options)
    n_empty, n_valid = sum(int((~v).sum()) for _, v in ref), sum(int(v.sum()) for _, v in ref)
    agree = sum(int((c == r[:, 5].astype(np.int64)).sum()) for (c, _), r in zip(ref, _np(want)))
    print(f"CROPS classified {options}: {n_valid} crops, {n_empty} empty, classifier agrees on {agree}; classes "
          f"{np.bincount(np.concatenate([c[c >= 0] for c, _ in ref]), minlength=3).tolist()}")
    assert n_valid >= 6
    if options:
        assert n_empty >= 1                                           # (a 0.02 gain leaves most boxes without a pixel)
    else:
        assert n_empty == 0 and 0 < agree < n_valid                   # the filter has something to keep and something to drop
    calls = []

    def classifier(x):
        assert not torch.is_grad_enabled() and x.dtype == torch.float32 and tuple(x.shape[1:]) == (3, 16, 16)
        calls.append(len(x))
        return _stub(x)
    mk = lambda mode: ClassifiedDetector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU, classifier=classifier,
                                         crop_size=(16, 16), mode=mode, classifier_batch=5, **options)
    got = mk("annotate")(images)
    assert max(calls) <= 5 and sum(calls) == n_valid + n_empty
    _same_rows(_np(got), _np(want), "annotate rows")
    for i, (c, _) in enumerate(ref):
        np.testing.assert_array_equal(got.cls2[i].cpu().numpy(), c, err_msg=f"cls2 {i}")
    got = mk("filter")(images)
    keep = [c == r[:, 5].astype(np.int64) for (c, _), r in zip(ref, _np(want))]
    _same_rows(_np(got), [r[k] for r, k in zip(_np(want), keep)], "filter rows")
    for i, ((c, _), k) in enumerate(zip(ref, keep)):
        np.testing.assert_array_equal(got.cls2[i].cpu().numpy(), c[k], err_msg=f"filter cls2 {i}")
    # NV12 surfaces in rectangular mode: the same classes for the rows that detector returns
    got = mk("annotate").rectangular()([_surface(yuv, k) for k, yuv in enumerate(yuvs)])
    rect_want = [r.clone() for r in Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU).rectangular()(images)]
    _same_rows(_np(got), _np(rect_want), "rect surfaces rows")
    for i, (c, _) in enumerate(_want_cls2(images, rect_want, **options)):
        np.testing.assert_array_equal(got.cls2[i].cpu().numpy(), c, err_msg=f"rect cls2 {i}")


def test_classified_detector_arguments(net):
    from object_detection_cib_amd.inference import ClassifiedDetector
    for kw, match in ((dict(classifier=None), "^classifier"), (dict(classifier=_stub, mode="drop"), "^mode"),
                      (dict(classifier=_stub, classifier_batch=0), "^classifier_batch"), (dict(classifier=_stub, crop_size=(0, 4)), "^size"),
                      (dict(classifier=_stub, gain=0), "^gain"), (dict(classifier=_stub, mean=MEAN), "^std")):
        with pytest.raises(ValueError, match=match):
            ClassifiedDetector(net, ANCH, image_size=S, **kw)
    det = ClassifiedDetector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=0.0, classifier=lambda x: x[:, 0, 0, 0], crop_size=(16, 16))
    with pytest.raises(ValueError, match="^classifier: returned"):
        det([np.zeros((32, 32, 3), np.uint8)])
