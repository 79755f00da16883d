"""Rectangular inference and validation on the device: kodhip_letterbox_batch and kodhip_val_prep_batch (the same launch on the
square; csrc/val_prep.hip) through the C ABI against `oracle.datapath.resize_linear_u8` pasted on a 114 canvas, and the front ends that use it - Detector / AugmentedDetector /
EnsembleDetector / TrackedDetector in rectangular mode (`rectangular()` / `rect=True`), the bounded graph cache,
DeviceValPipeline.make_batch(canvas=...) and validate() over a rectangular plan - against "the long way round": the numpy batch on the chunk's canvas, the eval forward,
`get_detections` and `non_max_suppression(letterbox=canvas table)`.

Everything is compared exactly, on bit patterns: the letterbox is integer arithmetic followed by one correctly rounded fp32
division, and both sides of every detector comparison run the same kernels on the same batch.  Figures are printed before they
are asserted (`pytest -s`).

Measured on an MI355X: every comparison exact; the ten detector images form the canvases (64, 128), (128, 128), (128, 64) and keep
28 - 247 rows each at conf 0.000445; the tracked clip emits 13 / 11 / 11 / 1 / 6 / 11 tracks; the module takes under 3 s.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fusion_helpers as F  # noqa: E402
from hip_helpers import stream  # noqa: E402
from object_detection_cib_amd import _lib  # noqa: E402
from object_detection_cib_amd.core.anchors.info import voc_anchor_info  # noqa: E402
from object_detection_cib_amd.core.nms import non_max_suppression  # noqa: E402
from object_detection_cib_amd.core.types import FeatureShape  # noqa: E402
from object_detection_cib_amd.data.device_pipeline import VAL_DESC, DeviceValPipeline, ImagePool  # noqa: E402
from object_detection_cib_amd.engine.rect import rect_batches, rect_canvas, rect_geometry, rect_order  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.layers import get_detections, get_detections_augmented  # noqa: E402
from object_detection_cib_amd.lightning.experiments.yv5_baseline.type_defs import LayerwiseAnchorInfo  # noqa: E402
from oracle.datapath import resize_linear_u8  # noqa: E402

ANCH = LayerwiseAnchorInfo(voc_anchor_info(8), voc_anchor_info(16), voc_anchor_info(32))
S, BATCH, NC = 128, 4, 3
IOU = 0.45


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_rows(got, want, tag):
    assert [len(g) for g in got] == [len(w) for w in want], (tag, [len(g) for g in got], [len(w) for w in want])
    for b, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=f"{tag} image {b}")


def _np(rows):
    return [r.cpu().numpy() for r in rows]


# ------------------------------------------------------------------------------------------------------- numpy reference
def _paste(img, nh, nw, top, left, H, W):
    """[3, H, W] fp32: the image resized to nh x nw (untouched when it has that size) on a 114 canvas at (top, left), / 255"""
    h, w = img.shape[:2]
    res = resize_linear_u8(img, nw, nh) if (nh, nw) != (h, w) else img
    canvas = np.full((H, W, 3), 114, dtype=np.uint8)
    canvas[top:top + nh, left:left + nw] = res
    return np.ascontiguousarray((canvas.astype(np.float32) / np.float32(255)).transpose(2, 0, 1))


def _rect_batch(images, H, W, size=S):
    """(fp32 [n, 3, H, W], KodLetterbox rows [n, 6]) of images letterboxed at `size` onto an H x W canvas"""
    xs, rows = [], []
    for im in images:
        h, w = im.shape[:2]
        nh, nw, top, left = rect_geometry(h, w, size, H, W)
        xs.append(_paste(im, nh, nw, top, left, H, W))
        rows.append([left, top, np.float32(w / float(nw)), np.float32(h / float(nh)), w, h])
    return np.stack(xs), np.float32(rows)


def _pairs_of(x):
    """fp32 [B, 3, H, W] -> the network's pair layout bf16 [B, H, W/2, 8] (r g b 0 of two neighbouring pixels) as int16 bits"""
    B, _, H, W = x.shape
    p = torch.zeros((B, H, W, 4), dtype=torch.bfloat16)
    p[..., :3] = torch.from_numpy(x).permute(0, 2, 3, 1).to(torch.bfloat16)
    return p.reshape(B, H, W // 2, 8).view(torch.int16).numpy()


# ---------------------------------------------------------------------------------------------------------------- kernel
CANVASES = ((64, 128), (128, 64), (96, 160), (128, 128))


def _fit(h, w, H, W):
    """the largest nh x nw of the image's aspect ratio that the canvas holds (at least 1 x 1), centred"""
    s = min(H / float(h), W / float(w))
    nh, nw = min(H, max(1, int(round(h * s)))), min(W, max(1, int(round(w * s))))
    return nh, nw, (H - nh) // 2, (W - nw) // 2


def _kernel_case(H, W, seed=0):
    """images and records of one batch on an H x W canvas: an image that needs no resize (odd top and left), 20 x 37
    upscaled, 300 x 171 downscaled, a 1-pixel-wide and a 1-pixel-high image (both widened: every tap is clamped), and the
    300 x 171 image again pushed to an odd left / top"""
    rng = np.random.default_rng(seed)
    sizes = [(H - 7, W - 7), (20, 37), (300, 171), (41, 1), (1, 20), (300, 171)]
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    geo = [(H - 7, W - 7, 3, 3)] + [_fit(h, w, H, W) for h, w in sizes[1:]]
    nh, nw = max(1, geo[5][0] - 2), max(1, geo[5][1] - 2)          # (two pixels smaller: room for an odd offset on both axes)
    geo[5] = (nh, nw, ((H - nh) // 2) | 1, ((W - nw) // 2) | 1)
    return images, geo


def _launch(entry, images, geo, dims, f32=True, pairs=True):
    pool = ImagePool(images, torch.device("cuda", 0))
    descs = np.zeros(len(images), dtype=VAL_DESC)
    for d, im, off, (nh, nw, top, left) in zip(descs, images, pool.offsets, geo):
        h, w = im.shape[:2]
        d["off"], d["h"], d["w"], d["nh"], d["nw"], d["top"], d["left"] = off, h, w, nh, nw, top, left
        d["scale_x"], d["scale_y"] = 1.0 / (nw / float(w)), 1.0 / (nh / float(h))
    d_dev = torch.from_numpy(descs.view(np.uint8)).cuda()
    B, (H, W) = len(images), (dims * 2)[-2:]                          # (dims: (S,) for kodhip_val_prep_batch, (H, W) otherwise)
    x = torch.full((B, 3, H, W), -7.0, device="cuda") if f32 else None
    p = torch.full((B, H, W // 2, 8), -7.0, dtype=torch.bfloat16, device="cuda") if pairs else None
    _lib.check(getattr(_lib.lib(), entry)(pool.data.data_ptr(), d_dev.data_ptr(), x.data_ptr() if f32 else None,
                                          p.data_ptr() if pairs else None, B, *dims, stream()), entry)
    torch.cuda.synchronize()
    return (x.cpu().numpy() if f32 else None), (p.cpu().view(torch.int16).numpy() if pairs else None)


@pytest.mark.parametrize("canvas", CANVASES)
def test_kernel_equals_numpy_bit_for_bit(canvas):
    assert _lib.lib().kodhip_val_prep_desc_bytes() == VAL_DESC.itemsize and _lib.lib().kodhip_version() >= 110
    H, W = canvas
    images, geo = _kernel_case(H, W)
    for im, (nh, nw, top, left) in zip(images, geo):
        assert 1 <= nh and top >= 0 and top + nh <= H and 1 <= nw and left >= 0 and left + nw <= W
    kinds = ["copy" if (nh, nw) == im.shape[:2] else "up" if nh > im.shape[0] or nw > im.shape[1] else "down" for im, (nh, nw, _, _) in zip(images, geo)]
    print(f"RECT kernel {H} x {W}: {[(im.shape[:2], g, k) for im, g, k in zip(images, geo, kinds)]}")
    assert kinds[0] == "copy" and "up" in kinds and "down" in kinds
    assert any(g[3] % 2 for g in geo) and any(g[2] % 2 for g in geo) and geo[5][3] % 2 == 1 and geo[5][2] % 2 == 1
    assert geo[3][1] > 1 and geo[4][0] > 1                       # the 1-pixel images are widened
    want = np.stack([_paste(im, *g, H, W) for im, g in zip(images, geo)])
    x, p = _launch("kodhip_letterbox_batch", images, geo, (H, W))
    np.testing.assert_array_equal(_bits(x), _bits(want))
    wp = _pairs_of(want)
    np.testing.assert_array_equal(p, wp)
    assert (p[..., 3] == 0).all() and (p[..., 7] == 0).all()     # the 4th channel of both pixels
    # either output alone
    np.testing.assert_array_equal(_bits(_launch("kodhip_letterbox_batch", images, geo, (H, W), pairs=False)[0]), _bits(want))
    np.testing.assert_array_equal(_launch("kodhip_letterbox_batch", images, geo, (H, W), f32=False)[1], wp)


@pytest.mark.parametrize("size", [128, 160])
def test_square_canvas_equals_val_prep_batch(size):
    images, geo = _kernel_case(size, size, seed=size)
    a = _launch("kodhip_val_prep_batch", images, geo, (size,))
    b = _launch("kodhip_letterbox_batch", images, geo, (size, size))
    np.testing.assert_array_equal(_bits(a[0]), _bits(b[0]))
    np.testing.assert_array_equal(a[1], b[1])


@pytest.mark.parametrize("size", [128, 160])
def test_val_prep_batch_equals_numpy_bit_for_bit(size):
    """kodhip_val_prep_batch on its own (it forwards to the letterbox launch, so the comparison above holds one kernel against
    itself): against the numpy reference, both outputs together and each alone"""
    images, geo = _kernel_case(size, size, seed=size)
    want = np.stack([_paste(im, *g, size, size) for im, g in zip(images, geo)])
    wp = _pairs_of(want)
    x, p = _launch("kodhip_val_prep_batch", images, geo, (size,))
    np.testing.assert_array_equal(_bits(x), _bits(want))
    np.testing.assert_array_equal(p, wp)
    np.testing.assert_array_equal(_bits(_launch("kodhip_val_prep_batch", images, geo, (size,), pairs=False)[0]), _bits(want))
    np.testing.assert_array_equal(_launch("kodhip_val_prep_batch", images, geo, (size,), f32=False)[1], wp)


# The smallest shape at which the flat index, the partial block and the odd-`left` pair logic can go wrong: a 6 x 10 canvas is 30
# pairs in one partial block.  (h, w) of the source, (nh, nw, top, left): a copy; one pixel upscaled at odd top and left; a
# downscale onto the whole canvas; a widened image at left = 1.  tests/test_hip_frames.py runs the same case through the frames.
TINY_CANVAS = (6, 10)
TINY_CASE = (((6, 10), (6, 10, 0, 0)), ((1, 1), (5, 5, 1, 3)), ((12, 20), (6, 10, 0, 0)), ((2, 4), (4, 8, 1, 1)))


def test_tiny_canvas_equals_numpy_bit_for_bit():
    H, W = TINY_CANVAS
    rng = np.random.default_rng(6)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w), _ in TINY_CASE]
    geo = [g for _, g in TINY_CASE]
    want = np.stack([_paste(im, *g, H, W) for im, g in zip(images, geo)])
    wp = _pairs_of(want)
    x, p = _launch("kodhip_letterbox_batch", images, geo, (H, W))
    np.testing.assert_array_equal(_bits(x), _bits(want))
    np.testing.assert_array_equal(p, wp)
    np.testing.assert_array_equal(_bits(_launch("kodhip_letterbox_batch", images, geo, (H, W), pairs=False)[0]), _bits(want))
    np.testing.assert_array_equal(_launch("kodhip_letterbox_batch", images, geo, (H, W), f32=False)[1], wp)


def test_val_prep_batch_argument_checks_launch_nothing():
    x = torch.full((1, 3, 64, 64), -7.0, device="cuda")
    h = _lib.lib()
    for args in ((None, 8, x.data_ptr(), None, 1, 64), (8, 8, None, None, 1, 64), (8, 8, x.data_ptr(), None, 0, 64),
                 (8, 8, x.data_ptr(), None, 1, 63), (8, 8, x.data_ptr() + 4, None, 1, 64), (8, 8, None, x.data_ptr() + 8, 1, 64)):
        assert h.kodhip_val_prep_batch(*args, stream()) < 0
        assert b"val_prep_batch" in h.kodhip_last_error()
    torch.cuda.synchronize()
    assert bool((x == -7.0).all())


def test_letterbox_batch_argument_checks_launch_nothing():
    x = torch.full((1, 3, 64, 64), -7.0, device="cuda")
    h = _lib.lib()
    for args in ((None, 8, x.data_ptr(), None, 1, 64, 64), (8, 8, None, None, 1, 64, 64), (8, 8, x.data_ptr(), None, 0, 64, 64),
                 (8, 8, x.data_ptr(), None, 1, 64, 63), (8, 8, x.data_ptr() + 4, None, 1, 64, 64), (8, 8, None, x.data_ptr() + 8, 1, 64, 64)):
        assert h.kodhip_letterbox_batch(*args, stream()) < 0
        assert b"letterbox_batch" in h.kodhip_last_error()
    torch.cuda.synchronize()
    assert bool((x == -7.0).all())


# ------------------------------------------------------------------------------------------------------------- detectors
# h x w: ten images, sorted by aspect ratio they form the chunks (64 x 128), (128 x 128), (128 x 64 - two images, padded)
SIZES = ((100, 37), (48, 128), (64, 64), (31, 70), (37, 100), (90, 128), (128, 60), (20, 45), (77, 77), (50, 110))


@pytest.fixture(scope="module")
def images():
    rng = np.random.default_rng(9)
    ranges = ((0, 256), (0, 48), (208, 256), (96, 160), (0, 128))
    return [rng.integers(*ranges[k % 5], (h, w, 3), dtype=np.uint8) for k, (h, w) in enumerate(SIZES)]


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


def _eager(net, augment=False):
    def forward(x):
        with torch.no_grad():
            if augment:
                return get_detections_augmented(x, net, ANCH)
            return get_detections(FeatureShape(width=x.shape[3], height=x.shape[2]), net(x), ANCH)
    return forward


def _long_way(images, post, sort=True, size=S):
    """the long way round, chunk by chunk: the numpy batch on the chunk's canvas (the last image repeated up to BATCH) ->
    `post(x on the device, KodLetterbox rows)` -> the real images' results, back in the caller's order; also the canvases"""
    shapes = [im.shape[:2] for im in images]
    order = rect_order(shapes).tolist() if sort else list(range(len(images)))
    out, canvases = [None] * len(images), []
    for i in range(0, len(order), BATCH):
        idx = order[i:i + BATCH]
        H, W = rect_canvas([shapes[k] for k in idx], size)
        canvases.append((H, W))
        padded = idx + [idx[-1]] * (BATCH - len(idx))
        x, rows = _rect_batch([images[k] for k in padded], H, W, size)
        res = post(torch.from_numpy(x).cuda(), rows)
        for k, r in zip(idx, res):
            out[k] = r.clone()
    return out, canvases


def _nms(forward, conf, **kw):
    return lambda x, rows: non_max_suppression(forward(x), conf, IOU, multi_label=False, letterbox=rows, **kw)


@pytest.fixture(scope="module")
def conf(net, net_b, images):
    """a threshold that leaves about 20 candidates in the sparsest image of either network, plain or augmented"""
    picks = []
    for fw in (_eager(net), _eager(net_b), _eager(net, augment=True)):
        def post(x, rows, fw=fw):
            picks.append(F.conf_for(fw(x).cpu().numpy(), 20))
            return [torch.zeros(0)] * BATCH
        _long_way(images, post)
    return min(picks)


def test_detector_rect_equals_the_long_way_round(net, images, conf):
    from object_detection_cib_amd.inference import Detector
    want, canvases = _long_way(images, _nms(_eager(net), conf))
    counts = [len(w) for w in want]
    print(f"RECT detector: conf {conf:.6g}, canvases {canvases}, rows per image {counts}")
    assert canvases == [(64, 128), (128, 128), (128, 64)] and min(counts) >= 1
    modes = [m.training for m in net.modules()]
    got = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU).rectangular()(images)
    assert [m.training for m in net.modules()] == modes and len(got) == len(images)
    _same_rows(_np(got), _np(want), "detector rect")                # (in the caller's order: the images differ in size)
    for g, (h, w) in zip(_np(got), SIZES):
        assert (g[:, :4] >= 0).all() and (g[:, [0, 2]] <= w).all() and (g[:, [1, 3]] <= h).all()
    # and the square detector answers differently: the canvas reached the network
    sq = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU)(images)
    assert any(len(a) != len(b) or not np.array_equal(a, b) for a, b in zip(_np(sq), _np(got)))
    # bad images are named by the caller's index, before anything runs
    d = Detector(net, ANCH, image_size=S, batch_size=BATCH).rectangular()
    with pytest.raises(ValueError, match="image 2"):
        d([images[0], images[1], np.zeros((1, 400, 3), np.uint8), images[2]])
    assert d([]) == []


def test_all_square_inputs_rect_equals_square(net, conf):
    from object_detection_cib_amd.inference import Detector
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (n, n, 3), dtype=np.uint8) for n in (128, 50, 77, 200, 64, 31)]
    a = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU)(imgs)
    b = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU).rectangular()(imgs)
    assert min(len(r) for r in a) >= 1
    _same_rows(_np(b), _np(a), "all-square rect")


def test_augmented_detector_rect(net, images, conf):
    from object_detection_cib_amd.inference import AugmentedDetector
    want, _ = _long_way(images, _nms(_eager(net, augment=True), conf))
    assert min(len(w) for w in want) >= 1
    got = AugmentedDetector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU).rectangular()(images)
    _same_rows(_np(got), _np(want), "augmented rect")


def test_ensemble_detector_rect(net, net_b, images, conf):
    from object_detection_cib_amd.core.nms import fuse_detections
    from object_detection_cib_amd.inference import EnsembleDetector

    def post(x, rows):
        outs = [non_max_suppression(fw(x), conf, IOU, multi_label=False, letterbox=rows) for fw in (_eager(net), _eager(net_b))]
        packed = torch.stack([o.packed for o in outs], dim=1).reshape(BATCH * 2, 300, 6)
        counts = torch.stack([o.counts for o in outs], dim=1).reshape(BATCH * 2)
        return fuse_detections(packed, counts, np.arange(BATCH + 1) * 2, np.tile(np.float32([1.0, 0.5]), BATCH), thres=0.55, agnostic=False,
                               max_det=300)
    want, _ = _long_way(images, post)
    assert min(len(w) for w in want) >= 1
    got = EnsembleDetector([net, net_b], ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU, merge="wbf",
                           weights=[1.0, 0.5], rect=True)(images)
    _same_rows(_np(got), _np(want), "ensemble rect")


def test_tracked_detector_rect_clip():
    from object_detection_cib_amd.core.tracking import ByteTracker
    from object_detection_cib_amd.inference import Detector, TrackedDetector
    net = F.network(5, 0.25)
    with torch.no_grad():                                             # boxes about half an anchor wide: neighbours in time overlap
        for name, p in net.named_parameters():
            if name.endswith("box_head.conv.bias"):
                p.copy_(torch.tensor([0.0, 0.0, -0.5, -0.5]).repeat(p.numel() // 4))
    net.fuse_eval(False)
    rng = np.random.default_rng(11)
    scene = np.kron(rng.integers(0, 256, (9, 18, 3)), np.ones((8, 8, 1))) + rng.integers(-8, 9, (72, 144, 3))
    scene = np.clip(scene, 0, 255).astype(np.uint8)
    frames = [np.ascontiguousarray(scene[:, 2 * f:2 * f + 128]) for f in range(6)]
    assert frames[0].shape == (72, 128, 3) and rect_canvas([f.shape[:2] for f in frames], S) == (96, 128)
    rows = _np(Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=0.0).rectangular()(frames))
    scores = np.stack([np.sort(r[:, 4])[::-1][:20] for r in rows])
    conf = float(np.float32((scores[:, 11].min() + scores[:, 12].min()) / 2))
    track = float(np.float32((scores[:, 5].min() + scores[:, 6].min()) / 2))
    assert 0 < conf < track < 1
    kw = dict(capacity=64, track_thresh=track, low_thresh=conf, new_thresh=track, match_thresh=0.9, match_thresh_low=0.9,
              match_thresh_new=0.9, fuse_score=False, track_buffer=2)
    det = TrackedDetector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, rect=True, graphed=True, **kw)
    got = det.clip(frames)
    assert list(det._geval) == [(BATCH, 3, 96, 128)]                  # one canvas, one captured forward for both chunks
    plain = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf).rectangular()
    trk = ByteTracker(streams=1, **kw)
    emitted = []
    for f, frame_rows in enumerate(plain(frames)):                    # (equal aspect ratios: the call keeps the frame order)
        packed = torch.full((1, 300, 6), float("nan"), device="cuda")
        packed[0, :len(frame_rows)] = frame_rows
        one = trk.update((packed, torch.tensor([len(frame_rows)], dtype=torch.int32, device="cuda")), stream=0)
        emitted.append(len(one[0]))
        np.testing.assert_array_equal(_bits(got[f].cpu().numpy()), _bits(one[0].cpu().numpy()), err_msg=f"frame {f}")
        np.testing.assert_array_equal(got.ids[f].cpu().numpy(), one.ids[0].cpu().numpy(), err_msg=f"ids of frame {f}")
        np.testing.assert_array_equal(got.det_index[f].cpu().numpy(), one.det_index[0].cpu().numpy(), err_msg=f"rows of frame {f}")
    print(f"RECT tracked clip: conf {conf:.6g}, track {track:.6g}, emitted tracks per frame {emitted}")
    assert len(got) == 6 and max(emitted) >= 1
    assert det.tracker.state().tobytes() == trk.state().tobytes()


def test_tiled_detector_refuses_rect(net):
    from object_detection_cib_amd.inference import TiledDetector
    with pytest.raises(ValueError, match="rect"):
        TiledDetector(net, ANCH, image_size=S, rect=True)
    t = TiledDetector(net, ANCH, image_size=S, rect=False)
    with pytest.raises(ValueError, match="rect"):
        t.rectangular()
    assert t.rectangular(False, max_graphs=3).max_graphs == 3 and not t.rect


# ----------------------------------------------------------------------------------------------------------- graph cache
def test_graphed_rect_keeps_at_most_max_graphs(images, conf):
    from object_detection_cib_amd.inference import Detector
    net = F.network(5, 0.25)                                          # (its own engine: the pins below are this test's)
    net.fuse_eval(False)
    eng = net.engine()
    first, second, third = (BATCH, 64, 128), (BATCH, 128, 128), (BATCH, 128, 64)      # the chunks' shapes, in sorted order
    eng.pin_shape(*first)                                             # somebody else's pin on the first chunk's shape
    eager = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU).rectangular()(images)
    d = Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=IOU, graphed=True).rectangular(max_graphs=2)
    assert d.rect and d.max_graphs == 2
    got = [g.clone() for g in d(images)]
    assert min(len(r) for r in eager) >= 1
    for g, e in zip(got, eager):
        assert torch.equal(g, e)
    key = lambda shp: (shp[0], 3, shp[1], shp[2])
    assert list(d._geval) == [key(second), key(third)] and len(d._geval) <= 2
    assert first in eng._pinned                                       # the evicted graph gave back its pin, not the other one
    assert eng._pin_counts[first] == 1 and {second, third} <= eng._pinned
    # the first chunk's images again: captured again, the least recently used graph (the second chunk's) goes, unpinned
    order = rect_order(SIZES).tolist()
    again = [g.clone() for g in d([images[k] for k in order[:BATCH]])]
    for g, k in zip(again, order[:BATCH]):
        assert torch.equal(g, eager[k])
    assert list(d._geval) == [key(third), key(first)]
    assert second not in eng._pinned and eng._pin_counts[first] == 2
    eng.unpin_shape(*first)
    assert first in eng._pinned
    with pytest.raises(ValueError, match="not pinned"):
        eng.unpin_shape(*second)
    with pytest.raises(ValueError, match="max_graphs"):
        Detector(net, ANCH, image_size=S).rectangular(max_graphs=0)


# ------------------------------------------------------------------------------------------------------------ validation
def test_make_batch_on_a_canvas(images):
    rng = np.random.default_rng(3)
    boxes, labels = [], []
    for h, w in SIZES:
        n = int(rng.integers(0, 4))
        xy = rng.uniform(0, 1, (n, 2, 2)) * [w, h]
        boxes.append(np.concatenate((xy.min(1), xy.max(1)), axis=1))
        labels.append(rng.integers(0, NC, n))
    pipe = DeviceValPipeline(images, boxes, labels, S, torch.device("cuda", 0))
    plan = pipe.rect_batches(BATCH)
    assert plan == rect_batches(SIZES, S, BATCH) and [(H, W) for _, H, W in plan] == [(64, 128), (128, 128), (128, 64)]
    for idx, H, W in plan:
        img, pairs, targets = pipe.make_batch(idx, out_f32=True, out_pairs=True, canvas=(H, W))
        want, _ = _rect_batch([images[k] for k in idx], H, W)
        assert tuple(img.shape) == (len(idx), 3, H, W) and tuple(pairs.shape) == (len(idx), H, W // 2, 8)
        np.testing.assert_array_equal(_bits(img.cpu().numpy()), _bits(want))
        np.testing.assert_array_equal(pairs.cpu().view(torch.int16).numpy(), _pairs_of(want))
        for k, t in zip(idx, targets):
            h, w = SIZES[k]
            nh, nw, top, left = rect_geometry(h, w, S, H, W)
            bb = np.asarray(boxes[k], dtype=np.float64).reshape(-1, 4).copy()
            bb[:, [0, 2]] = bb[:, [0, 2]] / w * nw + left
            bb[:, [1, 3]] = bb[:, [1, 3]] / h * nh + top
            np.testing.assert_array_equal(t.boxes.numpy(), bb)
            np.testing.assert_array_equal(t.labels.numpy(), labels[k])
            assert (bb[:, [0, 2]] <= W).all() and (bb[:, [1, 3]] <= H).all()
    # canvas None is the square batch, (S, S) equals it
    a = pipe.make_batch([0, 1], out_pairs=True)
    b = pipe.make_batch([0, 1], out_pairs=True, canvas=(S, S))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))
    assert all(torch.equal(p.boxes, q.boxes) for p, q in zip(a[2], b[2]))
    with pytest.raises(ValueError, match="canvas"):
        pipe.make_batch([0], canvas=(64, 128))                        # 100 x 37 is upright


@pytest.mark.parametrize("graphed", [False, True])
def test_validate_over_a_rect_plan_of_squares(net, conf, graphed):
    from object_detection_cib_amd.lightning.experiments.yv5_baseline.exp import DefaultYolov5Experiment
    rng = np.random.default_rng(8)
    sides = (128, 50, 77, 200, 64, 31, 100, 128)
    imgs = [rng.integers(0, 256, (n, n, 3), dtype=np.uint8) for n in sides]
    # ground truth = the network's own two best boxes of every image (in image pixels), so that the report is not all zeros
    from object_detection_cib_amd.inference import Detector
    found = _np(Detector(net, ANCH, image_size=S, batch_size=BATCH, conf_thres=conf, iou_thres=0.6)(imgs))
    assert min(len(r) for r in found) >= 2
    boxes = [r[:2, :4].astype(np.float64) for r in found]
    labels = [r[:2, 5].astype(np.int64) for r in found]
    pipe = DeviceValPipeline(imgs, boxes, labels, S, torch.device("cuda", 0))
    plan = pipe.rect_batches(BATCH)
    assert [(idx, H, W) for idx, H, W in plan] == [([0, 1, 2, 3], S, S), ([4, 5, 6, 7], S, S)]
    exp = DefaultYolov5Experiment(net, None, ANCH, val_nms_conf_threshold=conf, val_nms_iou_threshold=0.6, graphed=graphed)
    assert exp._geval.max_graphs == 8
    square = exp.validate([pipe.make_batch(idx)[::2] + (None,) for idx, _, _ in plan], NC)
    rect = exp.validate([pipe.make_batch(idx, canvas=(H, W))[::2] + (None,) for idx, H, W in plan], NC)
    print(f"RECT validate graphed {graphed}: {square}")
    assert square["map50"] > 0
    np.testing.assert_equal(rect, square)                             # (NaN entries of an empty class compare equal)
