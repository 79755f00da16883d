"""Video frames as detector input on the device: kodhip_letterbox_frames (csrc/video.hip) through the C ABI against numpy -
`frames_reference.yuv420_to_rgb` of the whole frame, then `test_hip_rect._paste` (oracle resize_linear_u8 on a 114 canvas) -
and the front ends fed `Frame`s against the same front ends fed the converted numpy images.

Everything is compared exactly, on bit patterns: colour conversion and letterbox are integer arithmetic followed by one correctly
rounded fp32 division, and both sides of a detector comparison run the same network on what must be the same batch.  Figures
are printed before they are asserted (`pytest -s`).

Measured on an MI355X: every comparison exact; the 300 x 172 frame holds 25 000 - 31 000 samples at each saturation end and about
7 000 luma samples below 16; the seven detector frames keep 19 - 64 rows each at conf 0.805 (26 - 93 augmented, 32 - 101 fused); the
tracked clip emits 11 / 8 / 6 / 6 / 7 / 8 tracks; the 32 tests take about 2 s.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import frames_reference as R  # noqa: E402
import fusion_helpers as F  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.data.frames import FRAME_DESC, Frame, frame_table, matrix_coeffs  # noqa: E402
from test_hip_rect import ANCH, BATCH, IOU, S, TINY_CANVAS, TINY_CASE, _bits, _fit, _kernel_case, _np, _pairs_of, _paste, _same_rows  # noqa: E402
from test_hip_rect import _launch as _launch_pool  # noqa: E402

CANVASES = ((64, 128), (128, 64), (96, 160))
DEV = "cuda"


# ------------------------------------------------------------------------------------------------------ frames on the device
def _yuv(h, w, rng):
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))


def _dev_plane(plane, pitch, rng):
    """a [rows, row bytes] plane on the device with rows `pitch` apart, in a buffer that ends with the plane's last byte"""
    buf = torch.from_numpy(R.pitched(plane, pitch, rng)).to(DEV)
    return buf.as_strided(plane.shape, (pitch, 1))


def _pitches(k, nb0, nb1):
    """frame k's pitches of plane 0 and of planes 1 / 2: row + 6, 256-aligned, or two different odd ones"""
    up = lambda n: (n + 255) // 256 * 256
    return ((nb0 + 6, nb1 + 6), (up(nb0), up(nb1)), (nb0 + 9, nb1 + 3))[k % 3]


def _make_frame(fmt, matrix, yuv, k, rng):
    """(Frame on the device in `fmt`, the RGB image it stands for)"""
    y, u, v = yuv
    h, w = y.shape
    rgb = R.yuv420_to_rgb(y, u, v, matrix_coeffs(matrix))
    if fmt in ("rgb", "bgr"):
        p0, _ = _pitches(k, 3 * w, 0)
        src = rgb if fmt == "rgb" else rgb[..., ::-1]
        t = _dev_plane(np.ascontiguousarray(src).reshape(h, 3 * w), p0, rng).as_strided((h, w, 3), (p0, 3, 1))
        return Frame.rgb(t, bgr=fmt == "bgr"), rgb
    if fmt == "nv12":
        p0, p1 = _pitches(k, w, w)
        uv = np.stack([u, v], axis=-1).reshape(h // 2, w)
        return Frame.nv12(_dev_plane(y, p0, rng), _dev_plane(uv, p1, rng), matrix), rgb
    p0, p1 = _pitches(k, w, w // 2)
    return Frame.i420(_dev_plane(y, p0, rng), _dev_plane(u, p1, rng), _dev_plane(v, p1, rng), matrix), rgb


def _launch(frames, geo, H, W, f32=True, pairs=True):
    """kodhip_letterbox_frames on records whose geometry is `geo` (nh, nw, top, left per frame)"""
    assert _lib.lib().kodhip_frame_desc_bytes() == FRAME_DESC.itemsize
    descs, _ = frame_table(frames, max(H, W))
    for d, f, (nh, nw, top, left) in zip(descs, frames, geo):
        d["nh"], d["nw"], d["top"], d["left"] = nh, nw, top, left
        d["scale_x"], d["scale_y"] = 1.0 / (nw / float(f.w)), 1.0 / (nh / float(f.h))
    d_dev = torch.from_numpy(descs.view(np.uint8)).to(DEV)
    B = len(frames)
    x = torch.full((B, 3, H, W), -7.0, device=DEV) if f32 else None
    p = torch.full((B, H, W // 2, 8), -7.0, dtype=torch.bfloat16, device=DEV) if pairs else None
    _lib.check(_lib.lib().kodhip_letterbox_frames(d_dev.data_ptr(), x.data_ptr() if f32 else None, p.data_ptr() if pairs else None,
                                                  B, H, W, stream()), "letterbox_frames")
    torch.cuda.synchronize()
    return (x.cpu().numpy() if f32 else None), (p.cpu().view(torch.int16).numpy() if pairs else None)


def _case(H, W):
    """sizes and geometry of one batch: no resize at odd top and left, 20 x 38 upscaled, 300 x 172 downscaled, 42 x 2 and 2 x 20
    (every tap clamped, one chroma column / row), 300 x 172 again at odd offsets"""
    sizes = [(H - 6, W - 6), (20, 38), (300, 172), (42, 2), (2, 20), (300, 172)]
    geo = [(H - 6, W - 6, 3, 3)] + [_fit(h, w, H, W) for h, w in sizes[1:]]
    nh, nw = max(1, geo[5][0] - 2), max(1, geo[5][1] - 2)
    geo[5] = (nh, nw, ((H - nh) // 2) | 1, ((W - nw) // 2) | 1)
    return sizes, geo


FORMATS = [("nv12", "bt601"), ("nv12", "bt709"), ("nv12", "bt601-full"), ("nv12", "bt709-full"), ("i420", "bt709"), ("bgr", "bt601")]


@pytest.mark.parametrize("fmt,matrix", FORMATS)
@pytest.mark.parametrize("canvas", CANVASES)
def test_kernel_equals_numpy_bit_for_bit(canvas, fmt, matrix):
    H, W = canvas
    rng = np.random.default_rng(H + len(fmt) + len(matrix))
    sizes, geo = _case(H, W)
    for (h, w), (nh, nw, top, left) in zip(sizes, geo):
        assert 1 <= nh and top >= 0 and top + nh <= H and 1 <= nw and left >= 0 and left + nw <= W
    assert geo[0][:2] == sizes[0] and geo[0][2] % 2 and geo[0][3] % 2 and geo[5][2] % 2 and geo[5][3] % 2
    assert geo[1][0] > 20 and geo[2][0] < 300 and geo[3][1] > 2 and geo[4][0] > 2
    yuvs = [_yuv(h, w, rng) for h, w in sizes]
    made = [_make_frame(fmt, matrix, yuv, k, rng) for k, yuv in enumerate(yuvs)]
    frames, rgbs = [m[0] for m in made], [m[1] for m in made]
    big = rgbs[2]
    low = sum(int((yuv[0] < 16).sum()) for yuv in yuvs)
    print(f"FRAMES kernel {H} x {W} {fmt} {matrix}: pitches {[f.pitches for f in frames]}, 300 x 172: {int((big == 0).sum())} zeros, "
          f"{int((big == 255).sum())} at 255, {low} luma samples below 16")
    assert (big == 0).any() and (big == 255).any() and low > 0          # both saturation ends, and Y below the offset
    assert any(f.pitches[0] % 4 for f in frames) and any(f.pitches[0] % 256 == 0 for f in frames)
    assert fmt == "bgr" or any(f.pitches[0] != f.pitches[1] for f in frames)
    want = np.stack([_paste(im, *g, H, W) for im, g in zip(rgbs, geo)])
    wp = _pairs_of(want)
    x, p = _launch(frames, geo, H, W)
    np.testing.assert_array_equal(_bits(x), _bits(want))
    np.testing.assert_array_equal(p, wp)
    assert (p[..., 3] == 0).all() and (p[..., 7] == 0).all()
    np.testing.assert_array_equal(_bits(_launch(frames, geo, H, W, pairs=False)[0]), _bits(want))
    np.testing.assert_array_equal(_launch(frames, geo, H, W, f32=False)[1], wp)


@pytest.mark.parametrize("canvas", [(96, 160), (128, 128)])
def test_rgb24_equals_letterbox_batch(canvas):
    H, W = canvas
    images, geo = _kernel_case(H, W, seed=H)
    frames = [Frame.rgb(torch.from_numpy(im).to(DEV)) for im in images]
    a = _launch_pool("kodhip_letterbox_batch", images, geo, (H, W))
    b = _launch(frames, geo, H, W)
    np.testing.assert_array_equal(_bits(a[0]), _bits(b[0]))
    np.testing.assert_array_equal(a[1], b[1])
    if H == W:
        c = _launch_pool("kodhip_val_prep_batch", images, geo, (H,))
        np.testing.assert_array_equal(_bits(c[0]), _bits(b[0]))
        np.testing.assert_array_equal(c[1], b[1])


@pytest.mark.parametrize("fmt", ["rgb", "bgr", "nv12", "i420"])
def test_tiny_canvas_equals_numpy_bit_for_bit(fmt):
    """test_hip_rect's tiny case (a 6 x 10 canvas: 30 pairs, one partial block; copy, 1 x 1 upscaled at odd top and left,
    downscale, widened at left = 1) through the frames: packed with a pitch above the row, and the even-sized sources as 4:2:0"""
    H, W = TINY_CANVAS
    rng = np.random.default_rng(6)
    if fmt in ("rgb", "bgr"):
        case = TINY_CASE
        rgbs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w), _ in case]
        frames = []
        for im in rgbs:
            h, w = im.shape[:2]
            src = np.ascontiguousarray(im if fmt == "rgb" else im[..., ::-1]).reshape(h, 3 * w)
            frames.append(Frame.rgb(_dev_plane(src, 3 * w + 5, rng).as_strided((h, w, 3), (3 * w + 5, 3, 1)), bgr=fmt == "bgr"))
        assert all(f.pitches[0] == 3 * f.w + 5 for f in frames if f.h > 1)      # (a one-row frame has no pitch)
    else:
        case = [c for c in TINY_CASE if c[0][0] % 2 == 0 and c[0][1] % 2 == 0]
        assert [c[0] for c in case] == [(6, 10), (12, 20), (2, 4)]
        made = [_make_frame(fmt, "bt601", _yuv(h, w, rng), k, rng) for k, ((h, w), _) in enumerate(case)]
        frames, rgbs = [m[0] for m in made], [m[1] for m in made]
    geo = [g for _, g in case]
    want = np.stack([_paste(im, *g, H, W) for im, g in zip(rgbs, geo)])
    wp = _pairs_of(want)
    x, p = _launch(frames, geo, H, W)
    np.testing.assert_array_equal(_bits(x), _bits(want))
    np.testing.assert_array_equal(p, wp)
    np.testing.assert_array_equal(_bits(_launch(frames, geo, H, W, pairs=False)[0]), _bits(want))
    np.testing.assert_array_equal(_launch(frames, geo, H, W, f32=False)[1], wp)


def test_padding_and_gaps_do_not_reach_the_output():
    H, W = 96, 160
    sizes, geo = _case(H, W)
    rng = np.random.default_rng(5)
    yuvs = [_yuv(h, w, rng) for h, w in sizes]
    outs = []
    for fill in (1, 2):
        pad = np.random.default_rng(100 + fill)
        frames = []
        for k, ((h, w), (y, u, v)) in enumerate(zip(sizes, yuvs)):
            pitch = w + 6 + 5 * k
            off = pitch * h + 37 * k                                    # a gap between the planes, filled like the padding
            buf = torch.from_numpy(R.nv12_surface(y, u, v, pitch, off, pad)).to(DEV)
            frames.append(Frame.nv12_surface(buf, h, w, pitch, off if k else None))
        outs.append(_launch(frames, geo, H, W))
    np.testing.assert_array_equal(_bits(outs[0][0]), _bits(outs[1][0]))
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    want = np.stack([_paste(R.yuv420_to_rgb(*yuv, matrix_coeffs("bt601")), *g, H, W) for yuv, g in zip(yuvs, geo)])
    np.testing.assert_array_equal(_bits(outs[0][0]), _bits(want))


def test_launcher_refuses_bad_arguments_and_launches_nothing():
    x = torch.full((1, 3, 64, 64), -7.0, device=DEV)
    h = _lib.lib()
    assert h.kodhip_version() >= 111
    for args in ((None, x.data_ptr(), None, 1, 64, 64), (8, None, None, 1, 64, 64), (8, x.data_ptr(), None, 0, 64, 64),
                 (8, x.data_ptr(), None, 1, 64, 63), (8, x.data_ptr() + 4, None, 1, 64, 64), (8, None, x.data_ptr() + 8, 1, 64, 64)):
        assert h.kodhip_letterbox_frames(*args, stream()) < 0
        assert b"letterbox_frames" in h.kodhip_last_error()
    torch.cuda.synchronize()
    assert bool((x == -7.0).all())


# ------------------------------------------------------------------------------------------------------------- detectors
SIZES = ((100, 38), (48, 128), (64, 64), (32, 70), (38, 100), (90, 128), (128, 60))      # h x w, all even: 4:2:0 frames


@pytest.fixture(scope="module")
def yuvs():
    rng = np.random.default_rng(9)
    return [_yuv(h, w, rng) for h, w in SIZES]


@pytest.fixture(scope="module")
def images(yuvs):
    """the numpy RGB images the frames stand for (BT.601; the expected side of every comparison is fed these)"""
    return [R.yuv420_to_rgb(*yuv, matrix_coeffs("bt601")) for yuv in yuvs]


@pytest.fixture(scope="module")
def net():
    n = F.network(5, 0.25)
    n.fuse_eval(False)
    return n


@pytest.fixture(scope="module")
def net_b():
    n = F.network(6, 0.25)
    n.fuse_eval(False)
    return n


def _kth_score(rows, k):
    """a threshold between the k-th and the (k + 1)-th best score of the image that has the fewest rows above it"""
    s = [np.sort(r[:, 4])[::-1] for r in rows]
    k = min(k, min(len(x) for x in s) - 2)
    assert k >= 1
    return float(np.float32((min(x[k] for x in s) + min(x[k + 1] for x in s)) / 2))


@pytest.fixture(scope="module")
def conf(net, net_b, images):
    from object_detection_cib_amd.inference import AugmentedDetector, Detector
    picks = []
    for cls, n in ((Detector, net), (Detector, net_b), (AugmentedDetector, net)):
        for rect in (False, True):
            picks.append(_kth_score(_np(cls(n, ANCH, image_size=S, batch_size=BATCH, conf_thres=0.0, iou_thres=IOU).rectangular(rect)(images)), 12))
    return min(picks)


def _surface(yuv, k=0, matrix="bt601"):
    """an NV12 decoder surface on the device: 256-aligned pitch, every other one with the UV plane behind an aligned height"""
    y, u, v = yuv
    h, w = y.shape
    pitch = (w + 255) // 256 * 256
    off = pitch * ((h + 15) // 16 * 16) if k % 2 else pitch * h
    buf = torch.from_numpy(R.nv12_surface(y, u, v, pitch, off, np.random.default_rng(k))).to(DEV)
    return Frame.nv12_surface(buf, h, w, pitch, off if k % 2 else None, matrix)


def _check_nonempty(want, tag):
    counts = [len(w) for w in want]
    print(f"FRAMES {tag}: rows per image {counts}")
    assert sum(c >= 1 for c in counts) > len(counts) // 2, counts


def test_detector_on_nv12_surfaces_and_host_i420(net, yuvs, images, conf):
    from object_detection_cib_amd.inference import Detector
    det = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU)
    want = _np(det(images))
    _check_nonempty(want, f"detector, conf {conf:.6g}")
    got = det([_surface(yuv, k) for k, yuv in enumerate(yuvs)])
    assert len(got) == 7                                              # batch 4: the second chunk is padded by one record
    _same_rows(_np(got), want, "nv12 surfaces")
    _same_rows(_np(det([Frame.from_host_yuv(R.packed_yuv(*yuv, "i420"), "i420") for yuv in yuvs])), want, "host i420")
    _same_rows(_np(det([Frame.from_host_yuv(R.packed_yuv(*yuv, "nv12"), "nv12") for yuv in yuvs])), want, "host nv12")
    # another matrix is another image
    other = _np(det([_surface(yuv, k, "bt709-full") for k, yuv in enumerate(yuvs)]))
    _same_rows(other, _np(det([R.yuv420_to_rgb(*yuv, matrix_coeffs("bt709-full")) for yuv in yuvs])), "bt709-full")
    assert any(len(a) != len(b) or not np.array_equal(a, b) for a, b in zip(other, want))
    # bad frames are named by the caller's index before anything runs; an empty call stays empty
    with pytest.raises(ValueError, match="image 1: .*even"):
        det([images[0], Frame.nv12(torch.zeros((5, 4), dtype=torch.uint8, device=DEV), torch.zeros((2, 4), dtype=torch.uint8, device=DEV))])
    with pytest.raises(ValueError, match="image 2"):
        det([images[0], _surface(yuvs[1]), Frame.rgb(np.zeros((1, 400, 3), np.uint8))])


def test_strided_crop_equals_its_contiguous_copy(net, conf):
    from object_detection_cib_amd.inference import Detector
    rng = np.random.default_rng(21)
    big = rng.integers(0, 256, (150, 201, 3), dtype=np.uint8)
    big_dev = torch.from_numpy(big).to(DEV)
    boxes = ((11, 111, 7, 140), (0, 150, 0, 201), (3, 64, 100, 201), (70, 149, 33, 98))
    det = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU)
    want = _np(det([np.ascontiguousarray(big[y0:y1, x0:x1]) for y0, y1, x0, x1 in boxes]))
    _check_nonempty(want, "crops")
    crops = [big_dev[y0:y1, x0:x1] for y0, y1, x0, x1 in boxes]
    assert not crops[0].is_contiguous() and crops[0].data_ptr() == big_dev.data_ptr() + 11 * 603 + 21
    _same_rows(_np(det([Frame.rgb(c) for c in crops])), want, "crops")
    bgr = torch.from_numpy(np.ascontiguousarray(big[..., ::-1])).to(DEV)
    _same_rows(_np(det([Frame.rgb(bgr[y0:y1, x0:x1], bgr=True) for y0, y1, x0, x1 in boxes])), want, "bgr crops")


@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("rect", [False, True])
def test_mixed_numpy_and_frames(net, yuvs, images, conf, rect, graphed):
    from object_detection_cib_amd.inference import Detector
    mk = lambda: Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU, graphed=graphed).rectangular(rect)
    want = [r.clone() for r in mk()(images)]
    _check_nonempty(want, f"mixed rect {rect} graphed {graphed}")
    rgb_dev = torch.from_numpy(images[3]).to(DEV)
    items = [images[0], _surface(yuvs[1], 1), Frame.from_host_yuv(R.packed_yuv(*yuvs[2], "i420"), "i420"), Frame.rgb(rgb_dev), images[4],
             _surface(yuvs[5], 0), Frame.rgb(np.ascontiguousarray(images[6][..., ::-1]), bgr=True)]
    got = mk()(items)
    _same_rows(_np(got), _np(want), "mixed")


def test_augmented_detector(net, yuvs, images, conf):
    from object_detection_cib_amd.inference import AugmentedDetector
    det = AugmentedDetector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU).rectangular()
    want = _np(det(images))
    _check_nonempty(want, "augmented")
    _same_rows(_np(det([_surface(yuv, k) for k, yuv in enumerate(yuvs)])), want, "augmented")


def test_ensemble_detector(net, net_b, yuvs, images, conf):
    from object_detection_cib_amd.inference import EnsembleDetector
    for rect in (False, True):
        det = EnsembleDetector([net, net_b], ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU, weights=[1.0, 0.5], rect=rect)
        want = _np(det(images))
        _check_nonempty(want, f"ensemble rect {rect}")
        _same_rows(_np(det([_surface(yuv, k) for k, yuv in enumerate(yuvs)])), want, f"ensemble rect {rect}")


def _tracking_net():
    net = F.network(5, 0.25)
    with torch.no_grad():                                             # boxes about half an anchor wide: neighbours in time overlap
        for name, p in net.named_parameters():
            if name.endswith("box_head.conv.bias"):
                p.copy_(torch.tensor([0.0, 0.0, -0.5, -0.5]).repeat(p.numel() // 4))
    net.fuse_eval(False)
    return net


def _scene(seed, h=72, w=144):
    """a blocky YUV scene with a little noise, wider than a frame: frames are crops that move two pixels per step"""
    rng = np.random.default_rng(seed)
    block = lambda hh, ww: np.clip(np.kron(rng.integers(0, 256, (-(-hh // 8), -(-ww // 8))), np.ones((8, 8)))[:hh, :ww]
                                   + rng.integers(-8, 9, (hh, ww)), 0, 255)
    return block(h, w).astype(np.uint8), block(h // 2, w // 2 + 4)[:, :w // 2].astype(np.uint8), block(h // 2, w // 2 + 4)[:, :w // 2].astype(np.uint8)


def _clip_frames(scene, n=6):
    y, u, v = scene
    return [tuple(np.ascontiguousarray(a) for a in (y[:, 2 * f:2 * f + 128], u[:, f:f + 64], v[:, f:f + 64])) for f in range(n)]


def _same_tracks(got, want, n, tag):
    assert len(got) == len(want) == n
    for f in range(n):
        np.testing.assert_array_equal(_bits(got[f].cpu().numpy()), _bits(want[f].cpu().numpy()), err_msg=f"{tag} boxes {f}")
        np.testing.assert_array_equal(got.ids[f].cpu().numpy(), want.ids[f].cpu().numpy(), err_msg=f"{tag} ids {f}")
        np.testing.assert_array_equal(got.det_index[f].cpu().numpy(), want.det_index[f].cpu().numpy(), err_msg=f"{tag} rows {f}")


def test_tracked_detector_clip_and_streams():
    from object_detection_cib_amd.inference import Detector, TrackedDetector
    net = _tracking_net()
    clips = [_clip_frames(_scene(11)), _clip_frames(_scene(12))]
    rgbs = [[R.yuv420_to_rgb(*yuv, matrix_coeffs("bt601")) for yuv in clip] for clip in clips]
    assert rgbs[0][0].shape == (72, 128, 3)
    rows = _np(Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=0.0).rectangular()(rgbs[0] + rgbs[1]))
    scores = np.stack([np.sort(r[:, 4])[::-1][:20] for r in rows])
    conf = float(np.float32((scores[:, 11].min() + scores[:, 12].min()) / 2))
    track = float(np.float32((scores[:, 5].min() + scores[:, 6].min()) / 2))
    assert 0 < conf < track < 1
    kw = dict(capacity=64, track_thresh=track, low_thresh=conf, new_thresh=track, match_thresh=0.9, match_thresh_low=0.9,
              match_thresh_new=0.9, fuse_score=False, track_buffer=2)
    mk = lambda streams: TrackedDetector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, rect=True, streams=streams, **kw)
    # a clip of one stream: 6 NV12 surfaces, two chunks
    want = mk(1).clip(rgbs[0])
    a = mk(1)
    got = a.clip([_surface(yuv, k) for k, yuv in enumerate(clips[0])])
    emitted = [len(want[f]) for f in range(6)]
    print(f"FRAMES tracked clip: conf {conf:.6g}, track {track:.6g}, emitted tracks per frame {emitted}")
    assert max(emitted) >= 1
    _same_tracks(got, want, 6, "clip")
    # the next frame of two streams per call
    b, c = mk(2), mk(2)
    total = 0
    for f in range(3):
        want = b([rgbs[0][f], rgbs[1][f]])
        got = c([_surface(clips[0][f], f), Frame.from_host_yuv(R.packed_yuv(*clips[1][f], "nv12"), "nv12")])
        _same_tracks(got, want, 2, f"streams step {f}")
        total += len(want[0]) + len(want[1])
    assert total >= 1
    assert b.tracker.state().tobytes() == c.tracker.state().tobytes()


def test_tiled_detector_refuses_frames(net, yuvs, images):
    from object_detection_cib_amd.inference import TiledDetector
    t = TiledDetector(net, ANCH, image_size=S)
    with pytest.raises(ValueError, match="image 1: .*Frame"):
        t([images[0], _surface(yuvs[1])])
