"""Detector - "what is in this image?" for a trained network: images of any sizes in, boxes in each image's own pixel
coordinates out.

Every stage runs on the device and is the one validation uses, so the network sees what it was trained and validated on:
letterbox (`letterbox_table` + kodhip_letterbox_batch, csrc/val_prep.hip), the eval forward (eager, fused or replayed as
a hipGraph), the prediction decode (kodhip_decode) and the NMS in YOLOv5's detect.py form (kodhip_nms_ex: one label per box
by default, optional class filter / class-agnostic suppression / smaller max_det), whose last launch maps the kept boxes
from the letterboxed frame back into the source image.  `AugmentedDetector` is detect.py's `--augment`: the letterboxed batch
goes through the network three times (as is, flipped at 0.83 of its size, at 0.67: kodhip_tta_view / kodhip_decode_view) and
ONE NMS runs over the merged predictions.  `TiledDetector` is sliced inference for images much larger than `image_size`: the
image is cut into overlapping tiles at its native resolution (engine/tiles.py, kodhip_tile_batch), every tile and the letterboxed
whole image go through the network and kodhip_nms_ex, and one kodhip_merge_detections per image joins what the views found.
`TrackedDetector` follows the boxes through a video: Detector, then ByteTrack on the device (core/tracking.py, kodhip_track_update).
Rectangular mode (`Detector.rectangular()`, also AugmentedDetector's; `rect=True` on EnsembleDetector and TrackedDetector)
letterboxes every chunk onto the smallest canvas of multiples of 32 that holds its images instead of the image_size square
(engine/rect.py, kodhip_letterbox_batch).
Every front end but TiledDetector also takes `Frame` items (data/frames.py): video frames that are already on the device - packed
RGB / BGR with a row pitch, NV12 surfaces, I420 planes - or host NV12 / I420 arrays; a call that holds one goes through
kodhip_letterbox_frames (csrc/video.hip), which reads the frames where they lie.  A call of numpy images only is untouched.
`Detector.detect_crops` (AugmentedDetector's too) also returns the pixels inside the boxes at one fixed size - kodhip_crop_plan /
kodhip_crop_batch (csrc/crops.hip, core/crops.py) on each chunk's sources while they are still on the device - and
`ClassifiedDetector` runs those crops through a second-stage classifier (YOLOv5 apply_classifier).
"""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .core.crops import CropOptions, launch_crops, pool_frames, split_rows
from .core.nms import _key_cap, _workspace, fuse_detections, merge_detections, non_max_suppression
from .core.tracking import ByteTracker, Tracks
from .core.types import FeatureShape
from .data.device_pipeline import VAL_DESC, ImagePool, _Stager, letterbox_table                 # noqa: F401  (re-exported)
from .data.frames import FRAME_DESC, Frame, check_images as _check_images, frame_records, frame_table, upload_frames, wrap_frames
from .engine.graphed import GraphCache
from .engine.rect import rect_canvas, rect_order
from .engine.tiles import tile_plan


def _has_frames(images) -> bool:
    return any(isinstance(im, Frame) for im in images)


def _chunk_tables(shapes, image_size: int, batch_size: int, rect: bool):
    """[(canvas (H, W), VAL_DESC records, KodLetterbox rows)] of consecutive chunks of batch_size images; rect: every chunk
    on the `rect_canvas` of its own images.  Host arithmetic only: a bad image raises before anything is uploaded."""
    tables = []
    for i in range(0, len(shapes), batch_size):
        part = shapes[i:i + batch_size]
        descs, boxes = letterbox_table(part, image_size, i)
        canvas = (image_size, image_size)
        if rect:
            canvas = rect_canvas(part, image_size)
            descs, boxes = letterbox_table(part, image_size, i, canvas)
        tables.append((canvas, descs, boxes))
    return tables


def _caller_order(order, results):
    """results of images that were processed in `order` (None: as given), back in the caller's order"""
    if order is None:
        return results
    back = [None] * len(results)
    for k, r in zip(order, results):
        back[k] = r
    return back


class Detector:
    """det = Detector(net, anchor_info, image_size=640, ...); results = det(images)

    images: a sequence of HWC uint8 arrays (3 channels) of any sizes, or of `Frame`s (data/frames.py: frames on the device in
    RGB / BGR / NV12 / I420, host NV12 / I420), or a mix - one Frame sends the whole call through kodhip_letterbox_frames.
    results: one [n, 6] tensor per image, (x1, y1, x2, y2, score, class) in that image's own pixels, n <= max_det, best score first.  conf_thres / iou_thres / classes / agnostic
    / multi_label / max_det are detect.py's arguments (non_max_suppression's keywords).  graphed=True replays the eval
    forward + decode as a hipGraph (GraphedEvalForward); eval_fused is handed to `net.fuse_eval` (None: left alone).
    Images are processed in chunks of `batch_size`; a final partial chunk is padded by repeating its last image, so one
    engine shape set serves every call.

    `det.rectangular()` switches to detect.py's minimum-padding letterbox (`rect`, False by default; the constructor's
    argument list is the one it always had): every chunk is letterboxed onto the smallest canvas of multiples of 32
    that holds its images (engine/rect.py rect_canvas; kodhip_letterbox_batch), so a chunk of 16:9 frames is 384 x 640 at
    image_size 640, 0.60 of the square's pixels.  A call sorts its images by aspect ratio first (rect_order) and returns the
    results in the caller's order.  Every distinct canvas is an input shape of its own: the engine builds a buffer set for it
    (KODHIP_MAX_SHAPE_SETS are kept; sorted chunks visit each shape in one run, so each is allocated once per call), and
    with graphed=True it is captured on first use; at most `max_graphs` captured forwards are kept, least recently used
    first (engine/graphed.GraphCache) - a shape that comes back after its eviction is allocated and captured again.  The
    network sees the grey border closer to the content than it did in training; what that does to accuracy is not measured.

    `augment` (class attribute, False here; True in AugmentedDetector) routes the forward through test-time augmentation."""

    augment = False
    rect = False                  # set by rectangular()
    _frame_stager = None          # pinned ring for the planes of host Frames, made on first use

    def __init__(self, net, anchor_info, image_size: int = 640, batch_size: int = 16, conf_thres: float = 0.25,
                 iou_thres: float = 0.45, classes=None, agnostic: bool = False, multi_label: bool = False, max_det: int = 300,
                 graphed: bool = False, eval_fused: Optional[bool] = None):
        _lib.require_gpu()
        if int(image_size) < 32 or int(image_size) % 32:
            raise ValueError(f"image_size {image_size}: expected a multiple of 32 (the network's largest stride)")
        if int(batch_size) < 1:
            raise ValueError(f"batch_size {batch_size}: expected >= 1")
        if not 1 <= int(max_det) <= 300:
            raise ValueError(f"max_det {max_det}: expected 1..300")
        assert _lib.lib().kodhip_val_prep_desc_bytes() == VAL_DESC.itemsize
        assert _lib.lib().kodhip_letterbox_bytes() == 6 * 4
        self.net, self.anchor_info = net, anchor_info
        self.S, self.B = int(image_size), int(batch_size)
        self.conf_thres, self.iou_thres, self.classes = conf_thres, iou_thres, classes
        self.agnostic, self.multi_label, self.max_det = bool(agnostic), bool(multi_label), int(max_det)
        self.graphed, self.eval_fused = bool(graphed), eval_fused
        self.device = next(net.parameters()).device
        self._stager = _Stager(self.device)
        # input shape -> GraphedEvalForward (augment: GraphedAugmentedForward), at most max_graphs (8 until rectangular() says
        # otherwise), least recently used first
        self._geval = GraphCache()

    def rectangular(self, rect: bool = True, max_graphs: Optional[int] = None):
        """Switch the minimum-padding letterbox on (or off) and, with max_graphs, bound the captured forwards that changing
        canvases may leave behind; returns self: `det = Detector(net, anchor_info, graphed=True).rectangular(max_graphs=8)`."""
        if max_graphs is not None:
            self._geval.resize(max_graphs)
        self.rect = bool(rect)
        return self

    @property
    def max_graphs(self) -> int:
        return self._geval.max_graphs

    def _forward(self, x: torch.Tensor) -> torch.Tensor:
        """decoded detections [B, rows, 5 + nc] of a letterboxed batch"""
        if self.graphed:
            from .engine.graphed import GraphedAugmentedForward, GraphedEvalForward
            key = tuple(x.shape)
            cls = GraphedAugmentedForward if self.augment else GraphedEvalForward
            return self._geval.forward(key, lambda: cls(self.net, self.anchor_info, key[0], key[2], key[3]))(x)
        from .lightning.experiments.yv5_baseline.layers import get_detections, get_detections_augmented
        if self.augment:           # (the engine's eval forward, called directly: no module mode is touched)
            return get_detections_augmented(x, self.net, self.anchor_info)
        # every submodule's own mode is restored afterwards, as validation_step does
        modes = [(m, m.training) for m in self.net.modules()]
        self.net.eval()
        try:
            res = self.net(x)
        finally:
            for m, was in modes:
                m.training = was
        return get_detections(FeatureShape(width=x.shape[3], height=x.shape[2]), res, self.anchor_info)

    def _letterboxed(self, images, sort: bool = False, keep: Optional[list] = None):
        """The input half of a call: checks, all geometry (a bad image raises here, before anything is uploaded or launched),
        then chunk after chunk of batch_size images uploaded and letterboxed -> (order, iterator of (real images of the chunk,
        x fp32 [B, 3, H, W], the padded chunk's KodLetterbox rows)).  sort: in rectangular mode the images are taken sorted by
        aspect ratio (every chunk then holds alike shapes) and `order` holds their positions for `_caller_order`; otherwise
        None.  keep: a list that receives every chunk's sources on the device as the chunk is letterboxed (an ImagePool or the
        list of uploaded Frames), for a caller that reads them again (detect_crops)."""
        images = list(images)
        _check_images(images, self.device)
        shapes = [im.shape[:2] for im in images]
        order = None
        if sort and self.rect and len(images) > 1:
            letterbox_table(shapes, self.S)                       # (its ValueErrors name the caller's index)
            order = rect_order(shapes).tolist()
            images, shapes = [images[k] for k in order], [shapes[k] for k in order]
        tables = _chunk_tables(shapes, self.S, self.B, self.rect)
        if _has_frames(images):            # one Frame sends the whole call through kodhip_letterbox_frames
            images = wrap_frames(images)
        chunks = (images[c * self.B:(c + 1) * self.B] for c in range(len(tables)))
        return order, ((len(chunk), *self._letterbox(chunk, *table, keep=keep)) for chunk, table in zip(chunks, tables))

    def _detect(self, batches):
        """`_letterboxed`'s chunks through forward and NMS -> (real images of the chunk, the padded chunk's PackedDetections),
        chunk after chunk"""
        if self.eval_fused is not None:
            self.net.fuse_eval(self.eval_fused)
        for n, x, boxes in batches:
            det = self._forward(x)
            out = non_max_suppression(det, self.conf_thres, self.iou_thres, self.classes, agnostic=self.agnostic,
                                      multi_label=self.multi_label, max_det=self.max_det, letterbox=boxes)
            yield n, out

    def _chunks(self, images):
        """images, in the given order, in chunks of batch_size through letterbox, forward and NMS"""
        return self._detect(self._letterboxed(images)[1])

    def _letterbox(self, chunk, canvas, descs, boxes, keep: Optional[list] = None):
        """one chunk on the device: the upload of its images and the letterbox launch -> (x fp32 [B, 3, H, W] on `canvas`,
        the KodLetterbox rows of the padded chunk).  Frames: planes in host memory go up in one pinned upload, the others are
        read where they lie (kodhip_letterbox_frames); numpy images go into an ImagePool (kodhip_letterbox_batch)."""
        B, (H, W), n = self.B, canvas, len(chunk)
        lib = _lib.lib()
        if isinstance(chunk[0], Frame):
            assert lib.kodhip_frame_desc_bytes() == FRAME_DESC.itemsize
            if self._frame_stager is None:
                self._frame_stager = _Stager(self.device, depth=2)
            src = upload_frames(chunk, self.device, self._frame_stager)          # (alive until the launch is queued)
            descs, rows = frame_table(src, self.S, 0, canvas if self.rect else None)
            assert np.array_equal(rows, boxes[:n])
            launch, name = lib.kodhip_letterbox_frames, "letterbox_frames"
        else:
            src = ImagePool(chunk, self.device)
            descs["off"] = src.offsets
            launch, name = functools.partial(lib.kodhip_letterbox_batch, src.data.data_ptr()), "letterbox_batch"
        if keep is not None:
            keep.append(src)
        if n < B:              # pad with the last record: the batch keeps its shape, the copies are dropped by the caller
            descs = np.concatenate((descs, np.repeat(descs[-1:], B - n)))
            boxes = np.concatenate((boxes, np.repeat(boxes[-1:], B - n, axis=0)))
        d_dev = self._stager.upload(descs)
        x = torch.empty((B, 3, H, W), dtype=torch.float32, device=self.device)
        _lib.check(launch(d_dev.data_ptr(), x.data_ptr(), None, B, H, W, torch.cuda.current_stream().cuda_stream), name)
        return x, boxes

    @torch.no_grad()
    def __call__(self, images: Sequence[np.ndarray]) -> List[torch.Tensor]:
        order, batches = self._letterboxed(images, sort=True)
        return _caller_order(order, [r for n, out in self._detect(batches) for r in out[:n]])

    def _crop_chunks(self, images, opts: CropOptions):
        """`__call__`'s chunks, each followed by plan + crop over its kept rows while the chunk's sources are still on the
        device -> (order, iterator of (the real images' [n_i, 6] rows, rows per image that were cropped, `launch_crops`'s
        result or None for a chunk without rows))"""
        kept: list = []
        order, batches = self._letterboxed(images, sort=True, keep=kept)

        def chunks():
            for n, out in self._detect(batches):
                src = kept.pop()
                assert not kept
                frames = (pool_frames(src) if isinstance(src, ImagePool) else src)[:n]
                counts = [len(r) if opts.max_crops is None else min(len(r), opts.max_crops) for r in out[:n]]
                res = None
                if sum(counts):
                    max_det = int(out.packed.shape[1])
                    row_index = np.concatenate([b * max_det + np.arange(c, dtype=np.int32) for b, c in enumerate(counts)])
                    frame_index = np.repeat(np.arange(n, dtype=np.int32), counts)
                    res = launch_crops(self._stager.upload(frame_records(frames)), n, out.packed, int(out.packed.shape[2]), row_index,
                                       frame_index, opts, self._stager)
                yield list(out[:n]), counts, res
        return order, chunks()

    @torch.no_grad()
    def detect_crops(self, images, size=(224, 224), **crop_options) -> "CropDetections":
        """`__call__` plus the pixels inside the boxes: the list `det(images)` returns (same boxes, same order - the caller's,
        also in rectangular mode) with `.crops[i]` fp32 [n_i, 3, h, w], `.rects[i]` int32 [n_i, 4] (x0, y0, cw, ch in image i's
        pixels), `.valid[i]` bool [n_i] and, with out_u8=True, `.u8[i]` uint8 [n_i, h, w, 3].  size and the keyword options are
        `core.crops.crop_detections`'s (mode, square, gain, pad, max_crops, bgr, mean, std, out_u8; with max_crops = k the
        crops belong to an image's first k rows).  Per chunk: letterbox, forward, NMS, then kodhip_crop_plan +
        kodhip_crop_batch on the chunk's sources - the numpy images' pool or the frames where they lie; the boxes stay on
        the device in between."""
        opts = CropOptions(size, **crop_options)
        order, chunks = self._crop_chunks(images, opts)
        dev = self.device
        rows, crops, u8, rects, valid = [], [], [], [], []
        for dets, counts, res in chunks:
            rows.extend(dets)
            if res is None:
                res = (torch.empty((0, 3, opts.h, opts.w), dtype=torch.float32, device=dev),
                       torch.empty((0, opts.h, opts.w, 3), dtype=torch.uint8, device=dev) if opts.out_u8 else None,
                       torch.empty((0, 4), dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.bool, device=dev))
            for dst, t in zip((crops, u8, rects, valid), res):
                dst.extend(split_rows(t, counts) or [None] * len(counts))
        back = lambda items: _caller_order(order, items)
        return CropDetections(back(rows), back(crops), back(u8) if opts.out_u8 else None, back(rects), back(valid))


class CropDetections(list):
    """What `Detector.detect_crops` returns: `Detector.__call__`'s list of per-image [n, 6] tensors, which also carries the
    per-image crops, rectangles and valid flags (core.crops.CropResult's fields; u8 is None without out_u8)."""

    def __init__(self, items, crops, u8, rects, valid):
        super().__init__(items)
        self.crops, self.u8, self.rects, self.valid = crops, u8, rects, valid


class AugmentedDetector(Detector):
    """Detector with test-time augmentation (YOLOv5 detect.py `--augment`): same constructor, same call, same results format.

    The forward becomes `get_detections_augmented` - three views of the letterboxed batch, up to three engine shape sets -
    eager, or one hipGraph over all three views with graphed=True (GraphedAugmentedForward).  Everything after the forward is
    unchanged: the NMS options, the un-letterbox launch and the chunk padding apply to the merged tensor, which lives in the
    letterboxed full-size frame.  It has about 1.8 times the rows of one forward (45147 against 25200 at 640 px), so with
    multi_label=True the NMS key workspace roughly doubles: 45147 * 80 keys need a 4 Mi-key capacity per image at nc = 80,
    against 2 Mi without augmentation."""

    augment = True


class ClassifiedDetections(list):
    """What `ClassifiedDetector` returns: the per-image [n, 6] tensors, with `.cls2[i]` int64 [n]: the classifier's class of
    every returned row (-1: the row's crop was empty)."""

    def __init__(self, items, cls2):
        super().__init__(items)
        self.cls2 = cls2


class ClassifiedDetector(Detector):
    """det = ClassifiedDetector(net, anchor_info, ..., classifier=model, crop_size=(224, 224), mode="filter"); results = det(images)

    Detector with a second-stage classifier (YOLOv5 utils/general.py apply_classifier): the constructor is Detector's plus,
    by keyword, `classifier` - any callable that takes crops fp32 [n, 3, h, w] and returns scores [n, K], called under
    torch.no_grad() in pieces of at most `classifier_batch` - `crop_size`, `mode` and the crop options of
    `core.crops.crop_detections` (`crop_mode` is its `mode`; square, gain, pad, bgr, mean, std; apply_classifier's values by
    default).  `augment=True` runs the detector with test-time augmentation (AugmentedDetector's forward).  Every chunk's
    crops are cut on the device (`Detector.detect_crops`'s path) and classified before the next chunk is read.
    mode "filter": YOLOv5's rule - a row stays when its class equals the classifier's argmax; rows with an empty crop are
    dropped.  mode "annotate": every row stays.  Either way the result carries `.cls2` (the argmax per returned row; -1 for
    an empty crop)."""

    def __init__(self, net, anchor_info, *args, classifier, crop_size=(224, 224), mode: str = "filter", classifier_batch: int = 256,
                 crop_mode: str = "stretch", square: bool = True, gain: float = 1.3, pad: float = 30, bgr: bool = False, mean=None,
                 std=None, augment: bool = False, **kwargs):
        if not callable(classifier):
            raise ValueError("classifier: expected a callable taking [n, 3, h, w] crops and returning [n, K] scores")
        if mode not in ("filter", "annotate"):
            raise ValueError(f"mode {mode!r}: expected 'filter' or 'annotate'")
        if int(classifier_batch) < 1:
            raise ValueError(f"classifier_batch {classifier_batch}: expected >= 1")
        self.crop_options = CropOptions(crop_size, crop_mode, square, gain, pad, None, bgr, mean, std)
        super().__init__(net, anchor_info, *args, **kwargs)
        self.classifier, self.mode, self.classifier_batch, self.augment = classifier, mode, int(classifier_batch), bool(augment)

    def _classify(self, crops: torch.Tensor) -> torch.Tensor:
        """argmax of the classifier's scores, int64 [n]"""
        parts = []
        for s in range(0, len(crops), self.classifier_batch):
            piece = crops[s:s + self.classifier_batch]
            scores = self.classifier(piece)
            if not (torch.is_tensor(scores) and scores.dim() == 2 and scores.shape[0] == len(piece) and scores.shape[1] >= 1):
                raise ValueError(f"classifier: returned {tuple(scores.shape) if torch.is_tensor(scores) else type(scores).__name__} "
                                 f"for {len(piece)} crops (expected [{len(piece)}, K] scores)")
            parts.append(scores.argmax(dim=1))
        return torch.cat(parts)

    @torch.no_grad()
    def __call__(self, images: Sequence[np.ndarray]) -> ClassifiedDetections:
        order, chunks = self._crop_chunks(images, self.crop_options)
        rows, cls2 = [], []
        for dets, counts, res in chunks:
            if res is None:
                rows.extend(dets)
                cls2.extend(torch.empty(0, dtype=torch.int64, device=self.device) for _ in dets)
                continue
            crops, _, _, valid = res
            c2 = torch.where(valid, self._classify(crops), torch.full_like(valid, -1, dtype=torch.int64))
            for r, c in zip(dets, split_rows(c2, counts)):
                if self.mode == "filter":
                    keep = c == r[:, 5].long()                      # (an empty crop's -1 equals no class)
                    r, c = r[keep], c[keep]
                rows.append(r)
                cls2.append(c)
        return ClassifiedDetections(_caller_order(order, rows), _caller_order(order, cls2))


class EnsembleDetector:
    """det = EnsembleDetector([net_a, net_b], anchor_info, image_size=640, ...); results = det(images)

    Several networks on the same images (YOLOv5 `detect.py --weights a.pt b.pt`): Detector's call and result format.  `nets`
    are one or more networks on one device with the same class count - widths, depths and parameters may differ;
    `anchor_info` is one LayerwiseAnchorInfo for all of them or one per network.  Validation, letterboxing and chunk padding
    happen once per chunk, every member's forward reads the same input tensor (graphed=True: one GraphedEvalForward per
    member and input shape; eval_fused is handed to every member).  rect / max_graphs are `Detector.rectangular`'s: every chunk
    on its own minimum-padding canvas, the call's images sorted by aspect ratio, at most max_graphs captured forwards per member.

    merge "wbf" (default): each member's detections go through non_max_suppression with the detector's options and the
    letterbox, and ONE weighted boxes fusion per chunk (core.nms.fuse_detections: `weights` per member, `fuse_thres`,
    `agnostic`, `max_det`) averages what the members agree on and ranks it by how many of them found it.  fuse_thres must
    not be below iou_thres: one member's surviving boxes could then fuse with each other.  A single member has nothing to
    fuse and is returned as its NMS leaves it.
    merge "nms": YOLOv5's `Ensemble` - the members' decoded tensors are concatenated along the row axis and go through one
    non_max_suppression; `weights` must be None."""

    def __init__(self, nets, anchor_info, image_size: int = 640, batch_size: int = 16, conf_thres: float = 0.25,
                 iou_thres: float = 0.45, classes=None, agnostic: bool = False, multi_label: bool = False, max_det: int = 300,
                 graphed: bool = False, eval_fused: Optional[bool] = None, merge: str = "wbf", weights=None,
                 fuse_thres: float = 0.55, rect: bool = False, max_graphs: int = 8):
        nets = list(nets)
        if not nets:
            raise ValueError("nets: expected at least one network")
        if merge not in ("wbf", "nms"):
            raise ValueError(f"merge {merge!r}: expected 'wbf' or 'nms'")
        # (a LayerwiseAnchorInfo is itself a named tuple: a plain list or tuple holds one per network)
        per_net = isinstance(anchor_info, (list, tuple)) and not hasattr(anchor_info, "_fields")
        infos = list(anchor_info) if per_net else [anchor_info] * len(nets)
        if len(infos) != len(nets):
            raise ValueError(f"anchor_info: {len(infos)} entries for {len(nets)} networks (expected one, or one per network)")
        if merge == "nms" and weights is not None:
            raise ValueError("weights: merge 'nms' takes none (every member's rows enter one NMS as they are)")
        if weights is None:
            w = np.ones(len(nets), dtype=np.float32)
        else:
            w = np.asarray(weights, dtype=np.float32).reshape(-1)
            if len(w) != len(nets) or not (np.isfinite(w).all() and (w > 0).all()):
                raise ValueError(f"weights {w.tolist()}: expected {len(nets)} finite values > 0, one per network")
        if not 0.0 <= float(fuse_thres) <= 1.0:
            raise ValueError(f"fuse_thres {fuse_thres}: expected a value in [0, 1]")
        if merge == "wbf" and float(fuse_thres) < float(iou_thres):
            raise ValueError(f"fuse_thres {fuse_thres} below iou_thres {iou_thres}: one member's surviving boxes could fuse with each other")
        # (Detector's own checks: image_size, batch_size, max_det, a GPU)
        self.members = [Detector(net, info, image_size, batch_size, conf_thres, iou_thres, classes, agnostic, multi_label, max_det,
                                 graphed, eval_fused).rectangular(rect, max_graphs) for net, info in zip(nets, infos)]
        first = self.members[0]
        if any(m.device != first.device for m in self.members):
            raise ValueError("nets: expected every network on the same device")
        if merge == "wbf" and len(nets) * int(max_det) > _lib.lib().kodhip_fuse_max_rows():
            raise ValueError(f"{len(nets)} networks x max_det {max_det} rows exceed the fusion's {_lib.lib().kodhip_fuse_max_rows()} "
                             f"rows per image; lower max_det")
        self.S, self.B, self.device = first.S, first.B, first.device
        self.conf_thres, self.iou_thres, self.classes = conf_thres, iou_thres, classes
        self.agnostic, self.multi_label, self.max_det = bool(agnostic), bool(multi_label), int(max_det)
        self.graphed, self.eval_fused, self.rect = bool(graphed), eval_fused, bool(rect)
        self.merge, self.weights, self.fuse_thres = merge, w, float(fuse_thres)
        self._stager = first._stager

    @torch.no_grad()
    def __call__(self, images: Sequence[np.ndarray]) -> List[torch.Tensor]:
        # (checks, geometry, rect order, letterbox and chunk padding: Detector's, once for all members)
        order, batches = self.members[0]._letterboxed(images, sort=True)
        if self.eval_fused is not None:
            for m in self.members:
                m.net.fuse_eval(self.eval_fused)
        B, M = self.B, len(self.members)
        nms = dict(agnostic=self.agnostic, multi_label=self.multi_label, max_det=self.max_det)
        results = []
        for n, x, boxes in batches:
            dets = [m._forward(x) for m in self.members]
            nc = {int(d.shape[2]) - 5 for d in dets}
            if len(nc) != 1:
                raise ValueError(f"nets: class counts {sorted(nc)} differ")
            if self.merge == "nms":
                out = non_max_suppression(torch.cat([d.float() for d in dets], dim=1), self.conf_thres, self.iou_thres, self.classes,
                                          letterbox=boxes, **nms)
            else:
                outs = [non_max_suppression(d, self.conf_thres, self.iou_thres, self.classes, letterbox=boxes, **nms) for d in dets]
                if M == 1:
                    out = outs[0]
                else:
                    # image-major: view b * M + m is model m of image b
                    rows = torch.stack([o.packed for o in outs], dim=1).reshape(B * M, self.max_det, 6)
                    counts = torch.stack([o.counts for o in outs], dim=1).reshape(B * M)
                    out = fuse_detections(rows, counts, np.arange(B + 1) * M, np.tile(self.weights, B), thres=self.fuse_thres,
                                          agnostic=self.agnostic, max_det=self.max_det)
            results.extend(out[:n])
        return _caller_order(order, results)


TILE_DESC = np.dtype([("off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("x0", "<i4"), ("y0", "<i4")], align=True)


def tiled_plans(shapes: Sequence[Sequence[int]], image_size: int, overlap: float = 0.2, full_view: bool = True,
                tile_max_det: int = 300):
    """one `tile_plan` per (h, w); raises ValueError for a bad image or for one whose views bring more rows to the merge
    than kodhip_merge_max_rows() allows - host arithmetic only, nothing is uploaded or launched"""
    limit = _lib.lib().kodhip_merge_max_rows()
    plans = []
    for i, (h, w) in enumerate(shapes):
        try:
            plan = tile_plan(h, w, image_size, overlap, full_view)
        except ValueError as e:
            raise ValueError(f"image {i}: {e}") from None
        if len(plan.views) * int(tile_max_det) > limit:
            raise ValueError(f"image {i} ({int(h)} x {int(w)}): {len(plan.views)} views x tile_max_det {tile_max_det} rows exceed the "
                             f"merge's {limit} rows per image; lower tile_max_det, or raise image_size or lower overlap for fewer tiles")
        plans.append(plan)
    return plans


class TiledDetector(Detector):
    """det = TiledDetector(net, anchor_info, image_size=640, overlap=0.2, ...); results = det(images)

    Sliced inference for images much larger than `image_size` (aerial, inspection, microscopy): same call and result format as
    `Detector`, but the image is not shrunk.  Each image is cut into overlapping image_size x image_size tiles at its native
    resolution (engine/tiles.py; kodhip_tile_batch), with `full_view` the letterboxed whole image is one more view, every view
    goes through the network and its own NMS (Detector's arguments; at most `tile_max_det` rows per view, mapped into image
    pixels by the view's KodLetterbox row), and ONE merge per image (kodhip_merge_detections) joins what neighbouring tiles found
    twice or in halves: `merge` "nmm" (the keeper grows to the hull of what it absorbs) | "nms", `merge_metric` "ios"
    (intersection over the smaller area) | "iou", `merge_thres`; classes are compared directly unless `agnostic`.

    The views of all images of a call form one stream of slots, processed in chunks of `batch_size` (the final chunk is padded
    by repeating its last slot: one engine shape set, one GraphedEvalForward); every chunk's NMS writes into call-wide buffers
    on the device, and the host sees nothing before the merge's counts.  There is no rectangular mode: tiles are full squares
    by construction and the full view is batched with them, so rect=True is refused."""

    def __init__(self, net, anchor_info, image_size: int = 640, batch_size: int = 16, overlap: float = 0.2, full_view: bool = True,
                 merge: str = "nmm", merge_metric: str = "ios", merge_thres: float = 0.5, tile_max_det: int = 300,
                 conf_thres: float = 0.25, iou_thres: float = 0.45, classes=None, agnostic: bool = False, multi_label: bool = False,
                 max_det: int = 300, graphed: bool = False, eval_fused: Optional[bool] = None, rect: bool = False,
                 max_graphs: int = 8):
        super().__init__(net, anchor_info, image_size, batch_size, conf_thres, iou_thres, classes, agnostic, multi_label, max_det,
                         graphed, eval_fused)
        self.rectangular(rect, max_graphs)
        if merge not in ("nmm", "nms"):
            raise ValueError(f"merge {merge!r}: expected 'nmm' or 'nms'")
        if merge_metric not in ("ios", "iou"):
            raise ValueError(f"merge_metric {merge_metric!r}: expected 'ios' or 'iou'")
        if not 0.0 <= float(merge_thres) <= 1.0:
            raise ValueError(f"merge_thres {merge_thres}: expected a value in [0, 1]")
        if not 1 <= int(tile_max_det) <= 300:
            raise ValueError(f"tile_max_det {tile_max_det}: expected 1..300")
        tile_plan(self.S, self.S, self.S, overlap, full_view)                  # (the overlap's own ValueError, now)
        assert _lib.lib().kodhip_tile_desc_bytes() == TILE_DESC.itemsize
        self.overlap, self.full_view = float(overlap), bool(full_view)
        self.merge, self.merge_metric, self.merge_thres = merge, merge_metric, float(merge_thres)
        self.tile_max_det = int(tile_max_det)

    def rectangular(self, rect: bool = True, max_graphs: Optional[int] = None):
        if rect:
            raise ValueError("rect=True: TiledDetector has no rectangular mode - tiles are full image_size squares by "
                             "construction, and the full view is batched with them")
        return super().rectangular(False, max_graphs)

    def plans(self, shapes: Sequence[Sequence[int]]):
        """the tile plan of each (h, w); raises what a call with such images would raise"""
        return tiled_plans(shapes, self.S, self.overlap, self.full_view, self.tile_max_det)

    @torch.no_grad()
    def __call__(self, images: Sequence[np.ndarray]) -> List[torch.Tensor]:
        images = list(images)
        i = next((i for i, im in enumerate(images) if isinstance(im, Frame)), len(images))
        _check_images(images[:i])                                              # (the images before the first Frame)
        if i < len(images):
            raise ValueError(f"image {i}: TiledDetector takes numpy images only - its tile cutter reads the image pool, "
                             f"not a Frame's planes")
        plans = self.plans([im.shape[:2] for im in images])                    # (all geometry first, as Detector)
        if not images:
            return []
        if self.eval_fused is not None:
            self.net.fuse_eval(self.eval_fused)
        lib, B, S, dev = _lib.lib(), self.B, self.S, self.device
        pool = ImagePool(images, dev)
        # the slot stream: every view of every image, then the last slot again up to a whole number of chunks
        slots = [(i, v) for i, plan in enumerate(plans) for v in plan.views]
        view_start = np.concatenate(([0], np.cumsum([len(p.views) for p in plans])))
        V = len(slots)
        slots += [slots[-1]] * (-V % B)
        tdesc, vdesc = np.zeros(len(slots), dtype=TILE_DESC), np.zeros(len(slots), dtype=VAL_DESC)
        boxes = np.zeros((len(slots), 6), dtype=np.float32)
        for k, (i, v) in enumerate(slots):
            h, w = plans[i].h, plans[i].w
            if v.full:
                vdesc[k], row = (a[0] for a in letterbox_table([(h, w)], S, i))
                vdesc[k]["off"] = pool.offsets[i]
                assert tuple(row) == tuple(np.float32(v.letterbox))
            else:
                tdesc[k] = (pool.offsets[i], h, w, v.x0, v.y0)
            boxes[k] = v.letterbox
        t_dev, v_dev, lb_dev = self._stager.upload(tdesc), self._stager.upload(vdesc), self._stager.upload(boxes)
        stream = torch.cuda.current_stream().cuda_stream
        rows_all = torch.empty((len(slots), self.tile_max_det, 6), dtype=torch.float32, device=dev)
        counts_all = torch.empty(len(slots), dtype=torch.int32, device=dev)
        ncand = torch.empty(B, dtype=torch.int32, device=dev)
        keep = None
        x = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
        for c0 in range(0, len(slots), B):
            k = c0
            while k < c0 + B:                                                   # runs of tiles / of full views: one launch each
                e = k + 1
                while e < c0 + B and slots[e][1].full == slots[k][1].full:
                    e += 1
                if slots[k][1].full:
                    _lib.check(lib.kodhip_letterbox_batch(pool.data.data_ptr(), v_dev.data_ptr() + k * VAL_DESC.itemsize,
                                                          x[k - c0].data_ptr(), None, e - k, S, S, stream), "letterbox_batch")
                else:
                    _lib.check(lib.kodhip_tile_batch(pool.data.data_ptr(), t_dev.data_ptr() + k * TILE_DESC.itemsize,
                                                     x[k - c0].data_ptr(), None, e - k, S, stream), "tile_batch")
                k = e
            det = self._forward(x).contiguous()
            assert det.dtype == torch.float32
            _, rows, P = det.shape
            nc = P - 5
            if self.classes is not None and keep is None:
                keep = torch.zeros(nc, dtype=torch.uint8, device=dev)
                keep[torch.as_tensor(list(self.classes), dtype=torch.long, device=dev)] = 1
            key_cap = _key_cap(rows * nc if self.multi_label else rows)
            keys = _workspace(dev, B * key_cap)
            _lib.check(lib.kodhip_nms_ex(det.data_ptr(), keys.data_ptr(), key_cap, ncand.data_ptr(), rows_all[c0].data_ptr(),
                                         counts_all[c0:].data_ptr(), B, rows, nc, float(self.conf_thres), float(self.iou_thres),
                                         self.tile_max_det, 30000, 0.0 if self.agnostic else 4096.0, 0 if self.multi_label else 1,
                                         keep.data_ptr() if keep is not None else None, lb_dev.data_ptr() + c0 * 24, stream), "nms_ex")
        return list(merge_detections(rows_all[:V], counts_all[:V], view_start, thres=self.merge_thres, metric=self.merge_metric,
                                     mode=self.merge, agnostic=self.agnostic, max_det=self.max_det))


class TrackedDetector(Detector):
    """det = TrackedDetector(net, anchor_info, streams=4, ...); tracks = det(frames)

    Detector followed by ByteTracker (core/tracking.py; kodhip_track_update): `det(frames)` takes the next frame of every
    stream - `streams` HWC uint8 arrays, stream s at index s, of any sizes - and returns `Tracks`: per stream the [n, 6] tensor
    of the tracked boxes in that frame's own pixels, with `.ids` and `.det_index`.  `clip(frames, stream)` takes consecutive
    frames of ONE stream: they go through the network in chunks of `batch_size` and every chunk is one tracker launch over
    the chunk's real frames (the padded copies never reach the tracker).

    The constructor is Detector's plus ByteTracker's keywords (its `agnostic` is `track_agnostic` here: `agnostic` is the
    NMS's).  conf_thres is the NMS threshold and defaults to low_thresh: the
    second association needs the boxes below track_thresh, so a conf_thres above track_thresh is refused.  max_det rows per
    frame reach the tracker.  rect=True (`Detector.rectangular`) never reorders here: stream s stays at index s and a clip's frames stay in
    time order; the frames of one video have one size and so share one canvas, one engine shape and one captured graph."""

    def __init__(self, net, anchor_info, image_size: int = 640, batch_size: int = 16, conf_thres: Optional[float] = None,
                 iou_thres: float = 0.45, classes=None, agnostic: bool = False, multi_label: bool = False, max_det: int = 300,
                 graphed: bool = False, eval_fused: Optional[bool] = None, streams: int = 1, capacity: int = 256,
                 track_thresh: float = 0.5, low_thresh: float = 0.1, new_thresh: Optional[float] = None, match_thresh: float = 0.8,
                 match_thresh_low: float = 0.5, match_thresh_new: float = 0.7, fuse_score: bool = True, track_agnostic: bool = True,
                 track_buffer: int = 30, rect: bool = False, max_graphs: int = 8):
        conf = float(low_thresh) if conf_thres is None else float(conf_thres)
        if conf > float(track_thresh):
            raise ValueError(f"conf_thres {conf} above track_thresh {track_thresh}: no detection would reach the first association")
        super().__init__(net, anchor_info, image_size, batch_size, conf, iou_thres, classes, agnostic, multi_label, max_det, graphed,
                         eval_fused)
        self.rectangular(rect, max_graphs)
        self.tracker = ByteTracker(streams, capacity, track_thresh, low_thresh, new_thresh, match_thresh, match_thresh_low,
                                   match_thresh_new, fuse_score, track_agnostic, track_buffer, device=self.device)
        self.streams = self.tracker.streams

    def reset(self, stream: Optional[int] = None):
        self.tracker.reset(stream)

    @torch.no_grad()
    def __call__(self, frames: Sequence[np.ndarray]) -> Tracks:
        frames = list(frames)
        if len(frames) != self.streams:
            raise ValueError(f"{len(frames)} frames for {self.streams} streams: expected one frame per stream")
        rows, counts = [], []
        for n, out in self._chunks(frames):
            rows.append(out.packed[:n]); counts.append(out.counts[:n])
        return self.tracker.update((torch.cat(rows), torch.cat(counts)) if len(rows) > 1 else (rows[0], counts[0]))

    @torch.no_grad()
    def clip(self, frames: Sequence[np.ndarray], stream: int = 0) -> Tracks:
        """consecutive frames of one stream -> Tracks with one entry per frame; the other streams are left alone"""
        frames = list(frames)
        if not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream {stream}: expected 0..{self.streams - 1}")
        if not frames:
            raise ValueError("clip: expected at least one frame")
        parts = [self.tracker.update((out.packed[:n], out.counts[:n]), stream=int(stream)) for n, out in self._chunks(frames)]
        return parts[0] if len(parts) == 1 else Tracks.concat(parts)
