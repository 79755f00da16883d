"""Video frames as detector input: `Frame` describes pixels that stay where they are - a uint8 tensor on the device with any
row pitch (packed RGB / BGR, e.g. a crop `big[y0:y1, x0:x1]` of a larger frame), an NV12 decoder surface, I420 planes - or a
host array in one of these formats, which is uploaded as it is (NV12 / I420: 1.5 bytes per pixel instead of RGB's 3).
kodhip_letterbox_frames (csrc/video.hip) reads the planes through the addresses in a FRAME_DESC record and writes the network's
input: the validation letterbox bit for bit, with OpenCV's fixed-point 4:2:0 conversion applied to every bilinear tap.

    det([Frame.nv12_surface(buf, 720, 1280, pitch=1280), Frame.rgb(t[100:500, 200:900]), numpy_hwc_image])

A Frame never raises when it is built: what is wrong with it is kept and raised as a ValueError by the call that uses it,
which can name it by its index - before anything is uploaded or launched.  Everything here is host arithmetic on addresses,
shapes and strides; it works on CPU tensors as well (`frame_table` is testable without a GPU).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .device_pipeline import letterbox_table

RGB24, BGR24, NV12, I420 = 0, 1, 2, 3
FORMATS = {"rgb": RGB24, "bgr": BGR24, "nv12": NV12, "i420": I420}

# csrc/kodhip_frame.h KodFrameDesc (the size is asserted through kodhip_frame_desc_bytes)
FRAME_DESC = np.dtype([("plane0", "<u8"), ("plane1", "<u8"), ("plane2", "<u8"), ("pitch0", "<i4"), ("pitch12", "<i4"),
                       ("format", "<i4"), ("h", "<i4"), ("w", "<i4"), ("nh", "<i4"), ("nw", "<i4"), ("top", "<i4"), ("left", "<i4"),
                       ("scale_x", "<f8"), ("scale_y", "<f8"), ("yoff", "<i4"), ("cy", "<i4"), ("cvr", "<i4"), ("cvg", "<i4"),
                       ("cug", "<i4"), ("cub", "<i4")], align=True)

MATRICES = ("bt601", "bt709", "bt601-full", "bt709-full")
# OpenCV's constants (color_yuv.simd.hpp: ITUR_BT_601_SHIFT 20, _CY, _CVR, _CVG, _CUG, _CUB), verbatim: "bt601" gives the
# pixels cv2.cvtColor(..., COLOR_YUV2RGB_NV12 / _I420) gives
_OPENCV_BT601 = (16, 1220542, 1673527, -852492, -409993, 2116026)


def matrix_coeffs(name: str) -> Tuple[int, int, int, int, int, int]:
    """(yoff, CY, CVR, CVG, CUG, CUB) of a YUV -> RGB matrix in 20-bit fixed point.  "bt601": OpenCV's integers; "bt709",
    "bt601-full", "bt709-full": round(c * 2^20) of the exact coefficients from (Kr, Kb) = (0.299, 0.114) / (0.2126, 0.0722)
    (limited range: chroma scaled by 255 / 224, luma by 255 / 219 after subtracting 16; full range: neither)."""
    if name == "bt601":
        return _OPENCV_BT601
    if name not in MATRICES:
        raise ValueError(f"matrix {name!r}: expected one of {', '.join(MATRICES)}")
    kr, kb = (0.299, 0.114) if name.startswith("bt601") else (0.2126, 0.0722)
    kg = 1.0 - kr - kb
    full = name.endswith("-full")
    s, cy, yoff = (1.0, 1.0, 0) if full else (255.0 / 224.0, 255.0 / 219.0, 16)
    fix = lambda c: int(round(c * (1 << 20)))
    return (yoff, fix(cy), fix(2.0 * (1.0 - kr) * s), fix(-2.0 * kr * (1.0 - kr) / kg * s), fix(-2.0 * kb * (1.0 - kb) / kg * s),
            fix(2.0 * (1.0 - kb) * s))


def _as_tensor(a):
    if isinstance(a, np.ndarray):
        if a.dtype != np.uint8:
            raise ValueError(f"dtype {a.dtype}: expected uint8")
        if any(s < 0 for s in a.strides):
            a = np.ascontiguousarray(a)
        return torch.from_numpy(a)
    if not isinstance(a, torch.Tensor):
        raise ValueError(f"{type(a).__name__}: expected a uint8 tensor or numpy array")
    if a.dtype != torch.uint8:
        raise ValueError(f"dtype {a.dtype}: expected uint8")
    return a


def _rows(t: torch.Tensor, rows: int, row_bytes: int, what: str) -> torch.Tensor:
    """a plane as a [rows, row_bytes] view of its bytes with stride (pitch, 1): the innermost dimensions must be dense and
    the pitch at least a row"""
    if t.dim() == 3:
        if t.stride(2) != 1 or t.stride(1) != t.shape[2]:
            raise ValueError(f"{what}: strides {tuple(t.stride())}: expected (pitch, {t.shape[2]}, 1)")
        t = t.as_strided((t.shape[0], t.shape[1] * t.shape[2]), (t.stride(0), 1))
    if t.dim() != 2 or tuple(t.shape) != (rows, row_bytes):
        raise ValueError(f"{what}: shape {tuple(t.shape)}: expected {rows} rows of {row_bytes} bytes")
    if t.stride(1) != 1:
        raise ValueError(f"{what}: last-dimension stride {t.stride(1)}: expected 1")
    if rows > 1 and t.stride(0) < row_bytes:
        raise ValueError(f"{what}: pitch {t.stride(0)} below the row's {row_bytes} bytes")
    return t


class Frame:
    """An immutable description of one frame - format, size, the planes as [rows, row bytes] uint8 views (which keep the
    memory alive), the colour matrix - built by `Frame.rgb`, `Frame.nv12`, `Frame.nv12_surface`, `Frame.i420` or
    `Frame.from_host_yuv`.  `shape` is (h, w, 3), as a numpy image's."""

    __slots__ = ("format", "h", "w", "planes", "matrix", "coeffs", "error")

    def __init__(self, format: int, h: int, w: int, planes: Sequence[torch.Tensor], matrix: str = "bt601",
                 error: Optional[str] = None):
        self.format, self.h, self.w, self.planes, self.matrix, self.error = int(format), int(h), int(w), tuple(planes), matrix, error
        self.coeffs = (0, 0, 0, 0, 0, 0)
        if error is None and self.format in (NV12, I420):
            try:
                self.coeffs = matrix_coeffs(matrix)
            except ValueError as e:
                self.error = str(e)

    # ------------------------------------------------------------------------------------------------------ constructors
    @classmethod
    def _build(cls, make):
        try:
            return make()
        except (ValueError, TypeError, RuntimeError, AttributeError, IndexError) as e:
            return cls(RGB24, 0, 0, (), error=str(e))

    @classmethod
    def rgb(cls, t, bgr: bool = False) -> "Frame":
        """t: uint8 [h, w, 3] with strides (pitch, 3, 1), any pitch >= 3 w - a tensor on the device is read in place (a crop
        of a larger frame is a view: no copy); a CPU tensor or a numpy HWC array is uploaded by the call.  bgr: the bytes of a
        pixel are b, g, r (OpenCV's order)."""
        def make():
            x = _as_tensor(t)
            if x.dim() != 3 or x.shape[2] != 3:
                raise ValueError(f"shape {tuple(x.shape)}: expected [h, w, 3]")
            h, w = int(x.shape[0]), int(x.shape[1])
            return cls(BGR24 if bgr else RGB24, h, w, (_rows(x, h, 3 * w, "rgb"),))
        return cls._build(make)

    @classmethod
    def nv12(cls, y, uv, matrix: str = "bt601") -> "Frame":
        """y: uint8 [h, w]; uv: [h/2, w/2, 2] or [h/2, w] (u, v interleaved); last-dimension stride 1, any row pitch each."""
        def make():
            yy, cc = _as_tensor(y), _as_tensor(uv)
            if yy.dim() != 2:
                raise ValueError(f"y: shape {tuple(yy.shape)}: expected [h, w]")
            h, w = int(yy.shape[0]), int(yy.shape[1])
            cls._even(h, w)
            if cc.dim() == 3 and cc.shape[2] != 2:
                raise ValueError(f"uv: shape {tuple(cc.shape)}: expected [{h // 2}, {w // 2}, 2] or [{h // 2}, {w}]")
            return cls(NV12, h, w, (_rows(yy, h, w, "y"), _rows(cc, h // 2, w, "uv")), matrix)
        return cls._build(make)

    @classmethod
    def nv12_surface(cls, buf, height: int, width: int, pitch: int, uv_offset: Optional[int] = None, matrix: str = "bt601") -> "Frame":
        """One decoder surface in `buf` (1-D uint8): Y rows at byte 0, `pitch` bytes apart, the interleaved UV rows from
        `uv_offset` on with the same pitch (default pitch * height; a decoder that aligns the coded height passes its own)."""
        def make():
            b = _as_tensor(buf)
            h, w, p = int(height), int(width), int(pitch)
            if b.dim() != 1 or b.stride(0) != 1:
                raise ValueError(f"surface: shape {tuple(b.shape)}: expected a dense 1-D buffer")
            cls._even(h, w)
            if p < w:
                raise ValueError(f"surface: pitch {p} below the row's {w} bytes")
            off = p * h if uv_offset is None else int(uv_offset)
            if off < (h - 1) * p + w:
                raise ValueError(f"surface: uv_offset {off} inside the Y plane ({(h - 1) * p + w} bytes)")
            need = off + (h // 2 - 1) * p + w
            if b.numel() < need:
                raise ValueError(f"surface: {b.numel()} bytes, {need} needed for {h} x {w} at pitch {p}, uv_offset {off}")
            yy = b.as_strided((h, w), (p, 1), b.storage_offset())
            cc = b.as_strided((h // 2, w), (p, 1), b.storage_offset() + off)
            return cls(NV12, h, w, (yy, cc), matrix)
        return cls._build(make)

    @classmethod
    def i420(cls, y, u, v, matrix: str = "bt601") -> "Frame":
        """y: uint8 [h, w]; u, v: [h/2, w/2]; last-dimension stride 1; u and v share one row pitch."""
        def make():
            yy, uu, vv = _as_tensor(y), _as_tensor(u), _as_tensor(v)
            if yy.dim() != 2:
                raise ValueError(f"y: shape {tuple(yy.shape)}: expected [h, w]")
            h, w = int(yy.shape[0]), int(yy.shape[1])
            cls._even(h, w)
            planes = (_rows(yy, h, w, "y"), _rows(uu, h // 2, w // 2, "u"), _rows(vv, h // 2, w // 2, "v"))
            if h > 2 and planes[1].stride(0) != planes[2].stride(0):
                raise ValueError(f"u / v: pitches {planes[1].stride(0)} and {planes[2].stride(0)}: expected one pitch for both")
            return cls(I420, h, w, planes, matrix)
        return cls._build(make)

    @classmethod
    def from_host_yuv(cls, arr, fmt: str, matrix: str = "bt601") -> "Frame":
        """arr: cv2's packed 4:2:0 layout, a contiguous uint8 numpy array [h * 3 / 2, w] - fmt "nv12": Y rows, then h / 2 rows of
        interleaved UV; "i420": Y rows, then the U plane, then the V plane.  The call uploads these bytes (1.5 per pixel)
        through pinned memory and converts on the device."""
        def make():
            if fmt not in ("nv12", "i420"):
                raise ValueError(f"fmt {fmt!r}: expected 'nv12' or 'i420'")
            if not isinstance(arr, np.ndarray):
                raise ValueError(f"{type(arr).__name__}: expected a numpy array")
            a = _as_tensor(np.ascontiguousarray(arr))
            if a.dim() != 2 or a.shape[0] % 3:
                raise ValueError(f"shape {tuple(a.shape)}: expected [h * 3 / 2, w]")
            h, w = int(a.shape[0]) // 3 * 2, int(a.shape[1])
            cls._even(h, w)
            if fmt == "nv12":
                return cls(NV12, h, w, (a[:h], a[h:]), matrix)
            flat, q = a.reshape(-1), (h // 2) * (w // 2)
            return cls(I420, h, w, (a[:h], flat[h * w:h * w + q].view(h // 2, w // 2), flat[h * w + q:].view(h // 2, w // 2)), matrix)
        return cls._build(make)

    @staticmethod
    def _even(h: int, w: int):
        if h < 2 or w < 2 or h % 2 or w % 2:
            raise ValueError(f"{h} x {w}: a 4:2:0 frame has even height and width")

    # ------------------------------------------------------------------------------------------------------------ queries
    @property
    def shape(self) -> Tuple[int, int, int]:
        return (self.h, self.w, 3)

    @property
    def device(self) -> Optional[torch.device]:
        return self.planes[0].device if self.planes else None

    @property
    def pitches(self) -> Tuple[int, int]:
        """bytes between rows of plane 0 and of planes 1 / 2 (a plane of one row: its row's bytes)"""
        p = [t.stride(0) if t.shape[0] > 1 else t.shape[1] for t in self.planes]
        return p[0], (p[1] if len(p) > 1 else 0)

    @property
    def nbytes(self) -> int:
        """the bytes of the frame's rows, without padding"""
        return sum(t.shape[0] * t.shape[1] for t in self.planes)

    def check(self, index: int, device=None):
        """raise what is wrong with this frame as ValueError("image <index>: ..."); device: where planes that are not in host
        memory have to be"""
        if self.error is not None:
            raise ValueError(f"image {index}: {self.error}")
        devs = {t.device for t in self.planes}
        if len(devs) != 1:
            raise ValueError(f"image {index}: planes on different devices ({', '.join(sorted(map(str, devs)))})")
        dev = devs.pop()
        if device is not None and dev.type != "cpu" and dev != torch.device(device):
            raise ValueError(f"image {index}: frame on {dev}, the detector on {torch.device(device)}")


def check_images(images, device=None):
    """every item a numpy HWC uint8 image or a `Frame` (checked by itself; its planes in host memory or on `device`); raises
    ValueError("image <index>: ...")"""
    for i, im in enumerate(images):
        if isinstance(im, Frame):
            im.check(i, device)
        elif not (isinstance(im, np.ndarray) and im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3):
            raise ValueError(f"image {i}: expected an HWC uint8 array with 3 channels")


def wrap_frames(images) -> List[Frame]:
    """a call's items as Frames: numpy HWC arrays become `Frame.rgb`"""
    return [im if isinstance(im, Frame) else Frame.rgb(im) for im in images]


def upload_frames(frames: Sequence[Frame], device, stager) -> List[Frame]:
    """Frames whose planes are in host memory -> Frames on `device`: the rows of all of them (without their padding) go up in ONE
    upload through `stager`'s pinned ring; frames already on the device are passed through untouched."""
    host = [k for k, f in enumerate(frames) if f.device.type == "cpu"]
    if not host:
        return list(frames)
    parts = [t.numpy().reshape(-1) if t.is_contiguous() else t.contiguous().numpy().reshape(-1) for k in host for t in frames[k].planes]
    buf = stager.upload(np.concatenate(parts))
    out, off = list(frames), 0
    for k in host:
        f, planes = frames[k], []
        for t in f.planes:
            n = t.shape[0] * t.shape[1]
            planes.append(buf[off:off + n].view(t.shape[0], t.shape[1]))
            off += n
        out[k] = Frame(f.format, f.h, f.w, planes, f.matrix)
    return out


def frame_records(frames: Sequence[Frame], first_index: int = 0) -> np.ndarray:
    """FRAME_DESC records that describe the frames alone - plane addresses, pitches, format, size and matrix; the letterbox
    geometry is left at zero (`frame_table` fills it in; kodhip_crop_plan / kodhip_crop_batch never read it).  Host arithmetic
    only; raises ValueError("image <first_index + k>: ...") for a bad frame."""
    for k, f in enumerate(frames):
        f.check(first_index + k)
    descs = np.zeros(len(frames), dtype=FRAME_DESC)
    for d, f in zip(descs, frames):
        for j, t in enumerate(f.planes):
            d[f"plane{j}"] = t.data_ptr()
        d["pitch0"], d["pitch12"] = f.pitches
        d["format"], d["h"], d["w"] = f.format, f.h, f.w
        d["yoff"], d["cy"], d["cvr"], d["cvg"], d["cug"], d["cub"] = f.coeffs
    return descs


def frame_table(frames: Sequence[Frame], image_size: int, first_index: int = 0, canvas=None):
    """(FRAME_DESC records, KodLetterbox rows float32 [n, 6]) of frames letterboxed at image_size: `letterbox_table`'s geometry
    for their shapes (canvas None: the image_size square; (H, W): that canvas) plus each frame's plane addresses, pitches,
    format and matrix.  Host arithmetic only; raises ValueError("image <first_index + k>: ...") for a bad frame."""
    descs = frame_records(frames, first_index)
    geo, boxes = letterbox_table([(f.h, f.w) for f in frames], image_size, first_index, canvas)
    for d, g in zip(descs, geo):
        for name in ("h", "w", "nh", "nw", "top", "left", "scale_x", "scale_y"):
            d[name] = g[name]
    return descs, boxes
