"""Second-stage crops: the pixels inside detection boxes at one fixed size, cut out on the device from the sources the detector
read - what a classifier behind the detector (YOLOv5 `apply_classifier`), an attribute / plate / OCR model, a re-identification
embedding or `detect.py --save-crop` (`save_one_box`) needs.

    res = crop_detections(sources, detections, size=(224, 224))
    res.crops[i]   # [n_i, 3, h, w] fp32      res.rects[i]   # [n_i, 4] int32  x0, y0, cw, ch      res.valid[i]   # [n_i] bool

kodhip_crop_plan turns the detection rows into crop records (the rectangle in YOLOv5's fp32 arithmetic: square, gain, pad, clip,
int()), kodhip_crop_batch cuts them out of RGB / BGR / NV12 / I420 frames where they lie and resizes each cutout on its own with
the validation letterbox's arithmetic (csrc/crops.hip); the boxes never visit the host.  The defaults are `apply_classifier`'s
(square, gain 1.3, pad 30, stretched to `size`); `square=False, gain=1.02, pad=10` are `save_one_box`'s.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from ..data.device_pipeline import ImagePool, _Stager
from ..data.frames import FRAME_DESC, Frame, check_images, frame_records, upload_frames
from .nms import PackedDetections

# csrc/crops.hip KodCropDesc (the size is asserted through kodhip_crop_desc_bytes)
CROP_DESC = np.dtype([("frame", "<i4"), ("valid", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("w", "<i4"), ("h", "<i4"), ("nh", "<i4"),
                      ("nw", "<i4"), ("top", "<i4"), ("left", "<i4"), ("scale_x", "<f8"), ("scale_y", "<f8")], align=True)
MODES = {"stretch": 0, "letterbox": 1}
MAX_LAUNCH = 65535                # crops per launch (the grid's second dimension) and frames per call

_STAGERS = {}


class CropOptions:
    """The checked options of a crop call (every ValueError names its argument); `crop_detections` lists them."""

    def __init__(self, size=(224, 224), mode: str = "stretch", square: bool = True, gain: float = 1.3, pad: float = 30,
                 max_crops: Optional[int] = None, bgr: bool = False, mean=None, std=None, out_u8: bool = False):
        try:
            h, w = (size, size) if isinstance(size, (int, np.integer)) else size
            h, w = int(h), int(w)
        except (TypeError, ValueError):
            raise ValueError(f"size {size!r}: expected (h, w)") from None
        if not (1 <= h <= 1024 and 1 <= w <= 1024):
            raise ValueError(f"size {size!r}: expected h and w in 1..1024")
        if mode not in MODES:
            raise ValueError(f"mode {mode!r}: expected 'stretch' or 'letterbox'")
        if not (np.isfinite(float(gain)) and float(gain) > 0):
            raise ValueError(f"gain {gain}: expected a finite value > 0")
        if not (np.isfinite(float(pad)) and float(pad) >= 0):
            raise ValueError(f"pad {pad}: expected a finite value >= 0")
        if max_crops is not None and int(max_crops) < 1:
            raise ValueError(f"max_crops {max_crops}: expected None or >= 1")
        if (mean is None) != (std is None):
            raise ValueError(f"{'std' if std is None else 'mean'}: mean and std come together (both or neither)")
        self.mean_std = None
        if mean is not None:
            m, s = (np.asarray(v, dtype=np.float32).reshape(-1) for v in (mean, std))
            if len(m) != 3 or not np.isfinite(m).all():
                raise ValueError(f"mean {mean!r}: expected 3 finite values")
            if len(s) != 3 or not np.isfinite(s).all() or (s == 0).any():
                raise ValueError(f"std {std!r}: expected 3 finite non-zero values")
            self.mean_std = (_lib.f32 * 6)(*m.tolist(), *s.tolist())
        self.h, self.w, self.mode, self.square = h, w, MODES[mode], bool(square)
        self.gain, self.pad, self.bgr, self.out_u8 = float(gain), float(pad), bool(bgr), bool(out_u8)
        self.max_crops = None if max_crops is None else int(max_crops)


class CropResult:
    """crops[i] fp32 [n_i, 3, h, w], u8[i] uint8 [n_i, h, w, 3] (None without out_u8), rects[i] int32 [n_i, 4] (x0, y0, cw, ch
    in image i's pixels; an empty crop: zeros), valid[i] bool [n_i] - per image, views of one buffer each per call."""

    def __init__(self, crops, u8, rects, valid):
        self.crops, self.u8, self.rects, self.valid = crops, u8, rects, valid


def pool_frames(pool: ImagePool) -> List[Frame]:
    """the images of an ImagePool as RGB24 Frames: views of the pool's buffer"""
    return [Frame.rgb(pool.data[off:off + h * w * 3].view(h, w, 3)) for off, (h, w) in zip(pool.offsets.tolist(), pool.shapes)]


def launch_crops(frames_dev: torch.Tensor, n_frames: int, rows: torch.Tensor, row_stride: int, row_index: np.ndarray,
                 frame_index: np.ndarray, opts: CropOptions, stager: _Stager):
    """kodhip_crop_plan + kodhip_crop_batch over N = len(row_index) >= 1 rows (more than 65 535: several launches into the same
    buffers).  frames_dev: the uploaded FRAME_DESC records; rows: the fp32 device tensor the row indices count from.
    -> (crops fp32 [N, 3, h, w], u8 [N, h, w, 3] | None, rects int32 [N, 4], valid bool [N])"""
    lib = _lib.lib()
    assert lib.kodhip_crop_desc_bytes() == CROP_DESC.itemsize and lib.kodhip_frame_desc_bytes() == FRAME_DESC.itemsize
    assert rows.dtype == torch.float32 and rows.is_cuda and rows.is_contiguous()
    N, dev = len(row_index), rows.device
    idx = stager.upload(np.concatenate((np.asarray(row_index, np.int32), np.asarray(frame_index, np.int32))))
    recs = torch.empty(N * CROP_DESC.itemsize, dtype=torch.uint8, device=dev)
    rects = torch.empty((N, 4), dtype=torch.int32, device=dev)
    crops = torch.empty((N, 3, opts.h, opts.w), dtype=torch.float32, device=dev)
    u8 = torch.empty((N, opts.h, opts.w, 3), dtype=torch.uint8, device=dev) if opts.out_u8 else None
    stream = torch.cuda.current_stream().cuda_stream
    for s in range(0, N, MAX_LAUNCH):
        n = min(MAX_LAUNCH, N - s)
        rec = recs.data_ptr() + s * CROP_DESC.itemsize
        _lib.check(lib.kodhip_crop_plan(frames_dev.data_ptr(), n_frames, rows.data_ptr(), row_stride, idx.data_ptr() + 4 * s,
                                        idx.data_ptr() + 4 * (N + s), n, opts.h, opts.w, opts.mode, int(opts.square), opts.gain,
                                        opts.pad, rec, rects[s:].data_ptr(), stream), "crop_plan")
        _lib.check(lib.kodhip_crop_batch(frames_dev.data_ptr(), n_frames, rec, n, crops[s:].data_ptr(),
                                         u8[s:].data_ptr() if u8 is not None else None, opts.h, opts.w, int(opts.bgr),
                                         opts.mean_std, stream), "crop_batch")
    return crops, u8, rects, rects[:, 2] > 0


def split_rows(t: Optional[torch.Tensor], counts: Sequence[int]):
    """a [N, ...] tensor as per-image views of counts[i] rows each (None stays None)"""
    if t is None:
        return None
    ends = np.cumsum(counts).tolist()
    return [t[e - n:e] for n, e in zip(counts, ends)]


def crop_detections(sources, detections, size=(224, 224), mode: str = "stretch", square: bool = True, gain: float = 1.3,
                    pad: float = 30, max_crops: Optional[int] = None, bgr: bool = False, mean=None, std=None,
                    out_u8: bool = False) -> CropResult:
    """sources: numpy HWC uint8 images and / or `Frame`s, as the detectors take them (numpy images go up as RGB24 records of an
    ImagePool, host YUV frames through `upload_frames`, device frames are read where they lie).  detections: one [n, >= 4]
    device tensor per source (x1, y1, x2, y2 first, in that source's pixels: what any detector front end returns), or a
    `PackedDetections`, whose buffer is read as it is.  size (h, w); mode "stretch" (cv2.resize of the cutout) | "letterbox"
    (aspect kept, centred on 114); square / gain / pad: the rectangle's arithmetic (the module's text); max_crops: each image's
    first k rows (best score first); bgr: both outputs in b, g, r order; mean, std (3 values each, in the output's channel
    order): (v / 255 - mean) / std as torchvision's Normalize; out_u8: also the uint8 HWC crops.  A row with no pixels inside
    its image (or non-finite) gives an empty crop: valid False, every pixel 114.  Bad arguments raise ValueError before
    anything is uploaded or launched; a call without rows launches nothing."""
    _lib.require_gpu()
    opts = CropOptions(size, mode, square, gain, pad, max_crops, bgr, mean, std, out_u8)
    sources = list(sources)
    packed = isinstance(detections, PackedDetections)
    dets = list(detections)
    if len(dets) != len(sources):
        raise ValueError(f"detections: {len(dets)} entries for {len(sources)} sources (expected one per source)")
    if len(sources) > MAX_LAUNCH:
        raise ValueError(f"sources: {len(sources)} in one call, more than {MAX_LAUNCH}")
    for i, d in enumerate(dets):
        if not (torch.is_tensor(d) and d.dim() == 2 and d.shape[1] >= 4 and d.is_cuda and d.is_floating_point()):
            raise ValueError(f"detections[{i}]: expected a floating-point [n, >= 4] tensor on the device")
    dev = dets[0].device if dets else torch.device("cuda", torch.cuda.current_device())
    if any(d.device != dev for d in dets):
        raise ValueError("detections: expected every tensor on the same device")
    if packed and (detections.packed.dtype != torch.float32 or not detections.packed.is_contiguous() or detections.packed.dim() != 3):
        raise ValueError("detections: expected PackedDetections.packed as a contiguous fp32 [B, max_det, >= 4] buffer")
    check_images(sources, dev)
    cap = opts.max_crops
    counts = [len(d) if cap is None else min(len(d), cap) for d in dets]
    N = sum(counts)
    if N == 0:
        empty = lambda *shape, dtype: [torch.empty((0, *shape), dtype=dtype, device=dev) for _ in sources]
        return CropResult(empty(3, opts.h, opts.w, dtype=torch.float32), empty(opts.h, opts.w, 3, dtype=torch.uint8) if out_u8 else None,
                          empty(4, dtype=torch.int32), empty(dtype=torch.bool))
    stager = _STAGERS.get(dev)
    if stager is None:
        stager = _STAGERS[dev] = _Stager(dev)
    # sources -> Frames on the device
    frames = list(sources)
    plain = [i for i, s in enumerate(sources) if not isinstance(s, Frame)]
    if plain:
        for i, f in zip(plain, pool_frames(ImagePool([sources[i] for i in plain], dev))):
            frames[i] = f
    frames = upload_frames(frames, dev, stager)
    frames_dev = stager.upload(frame_records(frames))
    if packed:
        rows = detections.packed
        max_det, stride = int(rows.shape[1]), int(rows.shape[2])
        row_index = np.concatenate([b * max_det + np.arange(n, dtype=np.int32) for b, n in enumerate(counts)])
    else:
        rows = torch.cat([d[:n, :4].float() for d, n in zip(dets, counts)]).contiguous()
        stride, row_index = 4, np.arange(N, dtype=np.int32)
    frame_index = np.repeat(np.arange(len(sources), dtype=np.int32), counts)
    crops, u8, rects, valid = launch_crops(frames_dev, len(sources), rows, stride, row_index, frame_index, opts, stager)
    return CropResult(split_rows(crops, counts), split_rows(u8, counts), split_rows(rects, counts), split_rows(valid, counts))
