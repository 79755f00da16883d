"""ByteTracker - "which of these boxes is the object I saw in the previous frame?" (ByteTrack, Zhang et al., ECCV 2022) on
the device: kodhip_track_update (csrc/tracking.hip) takes the rows and counts kodhip_nms_ex leaves behind
(`PackedDetections.packed` / `.counts`), keeps every track's Kalman filter and life cycle in one device buffer and emits the
tracked boxes with their identities.  One launch per call, one block per stream; the host sees nothing but the counts.

The association is greedy and fully ordered (pairs by similarity descending, ties by slot, then row), NOT ByteTrack's optimal
linear assignment: an optimal solver leaves ties undetermined and is a serial augmenting-path search.  include/kodhip.h has the
exact arithmetic; tests/track_reference.py is its plain form.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import _host, _lib
from .nms import PackedDetections

TRACK_HEADER = np.dtype([("frame", "<i4"), ("next_id", "<i4"), ("dropped", "<i4"), ("pad", "<i4")])
TRACK_RECORD = np.dtype([("state", "<i4"), ("id", "<i4"), ("last_frame", "<i4"), ("start_frame", "<i4"), ("score", "<f4"),
                         ("cls", "<f4"), ("kf", "<f4", (4, 5)), ("pad", "<i4", (2,))])
MAX_ROWS = 300


def state_dtype(cap: int) -> np.dtype:
    """one stream's state: the header's fields, then `tracks` [cap] records (state 0 free, 1 new, 2 tracked, 3 lost)"""
    return np.dtype([(n, TRACK_HEADER.fields[n][0]) for n in TRACK_HEADER.names] + [("tracks", TRACK_RECORD, (int(cap),))])


class Tracks(list):
    """What ByteTracker.update returns: per stream (per stream and frame, stream-major, for a clip) the [n, 6] tensor of
    the tracked boxes (x1, y1, x2, y2 of the filter, score, class; by slot), with `ids[i]` and `det_index[i]` (int32 [n]:
    the track's identity and the row of the input that it matched).  They are views of the device buffers `packed`
    [S, F, capacity, 6], `packed_ids` [S, F, capacity, 2] and `counts` [S, F]; rows beyond a count are uninitialised."""

    def __init__(self, packed: torch.Tensor, packed_ids: torch.Tensor, counts: torch.Tensor, host_counts):
        S, F = counts.shape
        super().__init__(packed[s, f, :host_counts[s][f]] for s in range(S) for f in range(F))
        self.ids = [packed_ids[s, f, :host_counts[s][f], 0] for s in range(S) for f in range(F)]
        self.det_index = [packed_ids[s, f, :host_counts[s][f], 1] for s in range(S) for f in range(F)]
        self.packed, self.packed_ids, self.counts, self.host_counts = packed, packed_ids, counts, host_counts

    @classmethod
    def concat(cls, parts):
        """the Tracks of consecutive calls on the same streams as one, along the frame axis"""
        S = parts[0].counts.shape[0]
        return cls(torch.cat([p.packed for p in parts], dim=1), torch.cat([p.packed_ids for p in parts], dim=1),
                   torch.cat([p.counts for p in parts], dim=1), [sum((p.host_counts[s] for p in parts), []) for s in range(S)])


class ByteTracker:
    """trk = ByteTracker(streams=1, capacity=256, ...); tracks = trk.update(detections)

    streams: independent videos tracked side by side (one block each).  capacity: track slots per stream, a power of two
    in 64..1024; a detection that finds no free slot is dropped and counted in `dropped`.  track_thresh / low_thresh: a
    detection is "high" above track_thresh and "low" between the two; new_thresh (None: track_thresh + 0.1): the score a
    high detection needs to start a track.  match_thresh / match_thresh_low / match_thresh_new: ByteTrack's cost limits of
    the three associations - a pair needs a similarity above float32(1 - limit).  fuse_score: similarity = IoU * score in
    the first and third association.  agnostic=False: only boxes of a track's class match it.  track_buffer: frames a lost
    track is kept.  The detections must include the low ones: run the NMS with conf_thres <= low_thresh."""

    def __init__(self, streams: int = 1, capacity: int = 256, track_thresh: float = 0.5, low_thresh: float = 0.1,
                 new_thresh: Optional[float] = None, match_thresh: float = 0.8, match_thresh_low: float = 0.5,
                 match_thresh_new: float = 0.7, fuse_score: bool = True, agnostic: bool = True, track_buffer: int = 30,
                 device="cuda"):
        _lib.require_gpu()
        lib = _lib.lib()
        assert lib.kodhip_track_header_bytes() == TRACK_HEADER.itemsize and lib.kodhip_track_bytes() == TRACK_RECORD.itemsize
        S, cap = int(streams), int(capacity)
        if S < 1:
            raise ValueError(f"streams {streams}: expected >= 1")
        if not (64 <= cap <= 1024 and cap & (cap - 1) == 0):
            raise ValueError(f"capacity {capacity}: expected a power of two in 64..1024")
        new = float(track_thresh) + 0.1 if new_thresh is None else float(new_thresh)
        for name, v in (("track_thresh", track_thresh), ("low_thresh", low_thresh), ("new_thresh", new), ("match_thresh", match_thresh),
                        ("match_thresh_low", match_thresh_low), ("match_thresh_new", match_thresh_new)):
            if not 0.0 <= float(v) <= 1.0:
                raise ValueError(f"{name} {v}: expected a value in [0, 1]")
        if float(low_thresh) > float(track_thresh):
            raise ValueError(f"low_thresh {low_thresh} above track_thresh {track_thresh}")
        if int(track_buffer) < 0:
            raise ValueError(f"track_buffer {track_buffer}: expected >= 0")
        self.streams, self.capacity = S, cap
        self.track_thresh, self.low_thresh, self.new_thresh = float(track_thresh), float(low_thresh), new
        self.sims = tuple(float(np.float32(1.0 - float(m))) for m in (match_thresh, match_thresh_low, match_thresh_new))
        self.fuse_score, self.agnostic, self.track_buffer = bool(fuse_score), bool(agnostic), int(track_buffer)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._stride = TRACK_HEADER.itemsize + cap * TRACK_RECORD.itemsize
        self._state = torch.empty(S * self._stride, dtype=torch.uint8, device=self.device)
        self._workspace = None
        self.reset()

    def reset(self, stream: Optional[int] = None):
        """free every slot and restart the frame and id counters - of all streams, or of one"""
        if stream is not None and not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream {stream}: expected 0..{self.streams - 1}")
        first, n = (0, self.streams) if stream is None else (int(stream), 1)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().kodhip_track_reset(self._state.data_ptr() + first * self._stride, n, self.capacity,
                                                     torch.cuda.current_stream().cuda_stream), "track_reset")

    def state(self) -> np.ndarray:
        """the streams' states as a numpy structured array [streams] of state_dtype(capacity) (tests, debugging)"""
        return self._state.cpu().numpy().view(state_dtype(self.capacity)).copy()

    @property
    def dropped(self):
        """detections per stream that found no free slot since the last reset"""
        return self.state()["dropped"].tolist()

    def _inputs(self, packed, stream):
        if isinstance(packed, PackedDetections):
            rows, counts = packed.packed, packed.counts
        else:
            rows, counts = packed
        if not (torch.is_tensor(rows) and torch.is_tensor(counts)):
            raise ValueError("expected a PackedDetections or a (rows, counts) pair of device tensors")
        S = self.streams if stream is None else 1
        if stream is not None:                                     # the frames of one stream: [F, max_rows, 6], [F]
            if not 0 <= int(stream) < self.streams:
                raise ValueError(f"stream {stream}: expected 0..{self.streams - 1}")
            if rows.dim() != 3:
                raise ValueError(f"rows {tuple(rows.shape)}: expected [F, max_rows, 6] for one stream")
            rows, counts = rows.unsqueeze(0), counts.reshape(1, -1)
        elif rows.dim() == 3:                                      # one frame per stream
            rows, counts = rows.unsqueeze(1), counts.reshape(-1, 1)
        if rows.dim() != 4 or rows.shape[0] != S or rows.shape[3] != 6 or rows.shape[1] < 1 or tuple(counts.shape) != tuple(rows.shape[:2]):
            raise ValueError(f"rows {tuple(rows.shape)} / counts {tuple(counts.shape)}: expected [{S}, F, max_rows, 6] and [{S}, F] "
                             f"(or [{S}, max_rows, 6] and [{S}])")
        if not 1 <= rows.shape[2] <= MAX_ROWS:
            raise ValueError(f"max_rows {rows.shape[2]}: expected 1..{MAX_ROWS}")
        if rows.dtype != torch.float32 or counts.dtype != torch.int32 or rows.device != self.device or counts.device != self.device:
            raise ValueError(f"expected float32 rows and int32 counts on {self.device}")
        return rows.contiguous(), counts.contiguous()

    @torch.no_grad()
    def update(self, packed, stream: Optional[int] = None) -> Tracks:
        """packed: what non_max_suppression returned for one frame per stream (B == streams), or (rows, counts) as
        [S, max_rows, 6] / [S], or [S, F, max_rows, 6] / [S, F] for F consecutive frames per stream in one launch.  With
        `stream`, the input is that one stream's frames ([F, max_rows, 6] / [F]) and the other streams stay as they are."""
        rows, counts = self._inputs(packed, stream)
        S, F, max_rows, _ = rows.shape
        cap, dev, lib = self.capacity, self.device, _lib.lib()
        out = torch.empty((S, F, cap, 6), dtype=torch.float32, device=dev)
        ids = torch.empty((S, F, cap, 2), dtype=torch.int32, device=dev)
        nout = torch.empty((S, F), dtype=torch.int32, device=dev)
        need = int(lib.kodhip_track_workspace_bytes(S, cap, max_rows))
        if need and (self._workspace is None or self._workspace.numel() < need):
            self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
        first = 0 if stream is None else int(stream)
        with torch.cuda.device(dev):
            _lib.check(lib.kodhip_track_update(self._state.data_ptr() + first * self._stride, rows.data_ptr(), counts.data_ptr(), S, F,
                                               max_rows, cap, self.track_thresh, self.low_thresh, self.new_thresh, *self.sims,
                                               int(self.fuse_score), int(self.agnostic), self.track_buffer, out.data_ptr(),
                                               ids.data_ptr(), nout.data_ptr(),
                                               self._workspace.data_ptr() if need else None,
                                               torch.cuda.current_stream().cuda_stream), "track_update")
            host = _host.fetch(nout)[0].tolist()                   # the one hand-off of a call (sizes the outputs)
        return Tracks(out, ids, nout, host)
