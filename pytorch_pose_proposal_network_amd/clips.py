"""Per-track skeleton clips on the device (no counterpart in the reference) over csrc/clips.hip: the last T frames of every
tracked person's keypoints as one tensor, the input of a skeleton-based action model (ST-GCN and its descendants take
[N, 3, T, V]).

* ``PoseClips(streams, frames, max_humans, ...)``   -- owns the per-stream clip state (64 slots each, a ring of T rows per
                                                       slot) and the output buffers.
* ``PoseClips.push(result, tracks, n_frames=None)`` -- one launch on the current stream: the DecodeResult and the TrackResult
                                                       of B = streams * frames images (image s * frames + t is frame t of
                                                       stream s) -> ClipRows; no allocation, no host synchronisation, no D2H.
* ``PoseClips.gather()``                            -- one launch: every clip in chronological order, zero-padded on the left,
                                                       normalised by the track's newest root box -> ClipBatch.
* ``ClipRows(row)`` / ``ClipBatch(x, ids, length)`` -- per person the slot its frame went to (-1: none); per slot the clip
                                                       f32 [3, T, K] (planes x, y, score), its track id and its length.

The rules (a clip follows a track id, ages as the track does, is born into the lowest free slot) are include/ppn.h's,
ppn_clip_push and ppn_clip_gather; tests/clips_ref.py restates them in NumPy.  Not built: more than one person per clip
tensor, bf16 output, a per-slot ready callback, MultiLaneInference integration.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import config as cfg
from . import decode as D
from . import lib as L
from .validate import _dense

SLOTS = L.PPN_CLIP_SLOTS
NORMS = {"none": L.PPN_CLIP_NORM_NONE, "root": L.PPN_CLIP_NORM_ROOT}


@dataclass
class ClipRows:
    """A view of the PoseClips' output buffer, on the device; the next push overwrites it."""
    row: torch.Tensor                # i32 [B, max_humans]   the slot person p's frame went to, -1: none


@dataclass
class ClipBatch:
    """Views of the PoseClips' output buffers, all on the device; the next gather overwrites them."""
    x: torch.Tensor                  # f32 [S, 64, 3, T, K]  planes x, y, score; the newest frame at T - 1, zeros before the first
    ids: torch.Tensor                # i32 [S, 64]           the slot's track id, 0: free
    length: torch.Tensor             # i32 [S, 64]           frames the clip holds, <= T

    def to_host(self, min_len: int = 1) -> List[Dict[int, Tuple[np.ndarray, int]]]:
        """One read-back: per stream {id: (x[3, T, K], len)} of the live slots with len >= min_len."""
        ids, length = self.ids.cpu().numpy(), self.length.cpu().numpy()
        x = self.x.cpu().numpy()
        return [{int(ids[s, i]): (x[s, i].copy(), int(length[s, i])) for i in range(ids.shape[1])
                 if ids[s, i] != 0 and length[s, i] >= min_len} for s in range(ids.shape[0])]


class PoseClips:
    """Up to 64 clips per stream, resident on the device, one per live track.

        tracker = Tracker(streams=1, frames=1)
        clips = PoseClips(streams=1, frames=1, max_gap=tracker.cfg.max_age)
        for frame in camera:                                         # u8 [1,S,S,3] on the device
            result, tracks, rows, batch = rt.inference_batch_clips(frame, model, tracker, clips, decoder)
            # batch.x[0, i] is the clip of track batch.ids[0, i]: feed the slots with batch.length == T to the action model

    length is T, the frames per clip; max_gap how many frames a clip survives without its id (the tracker's max_age keeps
    the two in step: then the clips are the live tracks, and 64 slots never overflow); norm "root" subtracts the centre of
    the track's newest root box and divides by its longer side, "none" hands out pixels."""

    def __init__(self, streams: int = 1, frames: int = 1, max_humans: int = 576, K: int = cfg.K, length: int = 32,
                 max_gap: int = 15, norm: str = "root", device="cuda"):
        if streams < 1 or frames < 1 or not 1 <= max_humans <= L.PPN_MATCH_MAX_PEOPLE:
            raise ValueError(f"{streams} streams x {frames} frames x {max_humans} people: at least one each, at most "
                             f"{L.PPN_MATCH_MAX_PEOPLE} people")
        if not 1 <= K <= L.PPN_MAX_KP:
            raise ValueError(f"K {K} outside 1..{L.PPN_MAX_KP}")
        if not 1 <= length <= L.PPN_CLIP_MAX_LEN or max_gap < 0 or norm not in NORMS:
            raise ValueError(f"PoseClips needs a length in 1..{L.PPN_CLIP_MAX_LEN}, max_gap >= 0 and norm in {sorted(NORMS)}")
        self.streams, self.frames, self.max_humans, self.K = int(streams), int(frames), int(max_humans), int(K)
        self.length = int(length)
        self.cfg = L.ClipCfg(self.K, self.length, int(max_gap), NORMS[norm])
        dev = torch.device(device)
        S, B, M, T = self.streams, self.streams * self.frames, self.max_humans, self.length
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        self.state = dict(id=torch.zeros(S, SLOTS, **i32), gap=torch.zeros(S, SLOTS, **i32), len=torch.zeros(S, SLOTS, **i32),
                          ref=torch.zeros(S, SLOTS, 4, **f32), mask=torch.zeros(S, SLOTS, T, **i32),
                          ring=torch.zeros(S, SLOTS, T, 3, self.K, **f32), pos=torch.zeros(S, **i32),
                          flags=torch.zeros(S, **i32))
        self.device = self.state["id"].device                          # "cuda" resolved to the device the tensors are on
        self.row = torch.full((B, M), -1, **i32)
        self.x = torch.zeros(S, SLOTS, 3, T, self.K, **f32)
        self.ids = torch.zeros(S, SLOTS, **i32)
        self.len = torch.zeros(S, SLOTS, **i32)
        self._n_frames = torch.zeros(S, **i32)
        self._st = L.ClipState(*(self.state[n].data_ptr() for n, _ in L.ClipState._fields_))

    def push(self, result: D.DecodeResult, tracks, n_frames=None, smoothed: bool = True) -> ClipRows:
        """ppn_clip_push on the current stream.  `tracks`: the TrackResult of the same batch; its smoothed centres are what
        the clips hold when `smoothed` is true and it has them, otherwise the raw box centres.  `n_frames` as in
        Tracker.update."""
        dev = self.device
        if dev.type != "cuda":
            raise ValueError("PoseClips.push runs on the device: the clips live on " + str(dev))
        B, M, K = self.streams * self.frames, self.max_humans, self.K
        if result.max_humans != M:
            raise ValueError(f"result holds {result.max_humans} people per image, the clips {M}")
        _dense("result.count", result.count, (B,), torch.int32, dev)
        _dense("result.kp_cell", result.kp_cell, (B, M, K), torch.int32, dev)
        _dense("result.bbox", result.bbox, (B, M, K, 4), torch.float32, dev)
        _dense("result.score", result.score, (B, M, K), torch.float32, dev)
        _dense("tracks.ids", tracks.ids, (B, M), torch.int32, dev)
        xy = tracks.xy if smoothed else None
        if xy is not None:
            _dense("tracks.xy", xy, (B, M, K, 2), torch.float32, dev)
        nf = None
        if n_frames is not None:
            if isinstance(n_frames, torch.Tensor) and n_frames.device == dev:
                nf = _dense("n_frames", n_frames, (self.streams,), torch.int32, dev)
            else:
                host = torch.as_tensor(n_frames, dtype=torch.int32).reshape(-1)
                if host.numel() != self.streams:
                    raise ValueError(f"{host.numel()} frame counts for {self.streams} streams")
                self._n_frames.copy_(host)
                nf = self._n_frames
        L.check(L.load().ppn_clip_push(C.byref(self.cfg), C.byref(self._st), result.count.data_ptr(),
                                       result.kp_cell.data_ptr(), result.bbox.data_ptr(), result.score.data_ptr(),
                                       tracks.ids.data_ptr(), xy.data_ptr() if xy is not None else None, self.streams,
                                       self.frames, M, nf.data_ptr() if nf is not None else None, self.row.data_ptr(),
                                       L.current_stream_ptr()), "ppn_clip_push")
        return ClipRows(self.row)

    def gather(self) -> ClipBatch:
        """ppn_clip_gather on the current stream: every clip of every stream."""
        if self.device.type != "cuda":
            raise ValueError("PoseClips.gather runs on the device: the clips live on " + str(self.device))
        L.check(L.load().ppn_clip_gather(C.byref(self.cfg), C.byref(self._st), self.streams, self.x.data_ptr(),
                                         self.ids.data_ptr(), self.len.data_ptr(), L.current_stream_ptr()), "ppn_clip_gather")
        return ClipBatch(self.x, self.ids, self.len)

    def reset(self, streams: Optional[Sequence[int]] = None):
        """Forget every clip, the ring position and the flags: of all streams, or of the named ones."""
        if streams is None:
            for t in self.state.values():
                t.zero_()
            return
        for s in streams:
            if not 0 <= int(s) < self.streams:
                raise ValueError(f"stream {s} outside 0..{self.streams - 1}")
            for t in self.state.values():
                t[int(s)].zero_()

    def flags(self) -> np.ndarray:
        """One D2H: per stream the OR of PPN_CLIP_FLAG_SLOT_OVERFLOW since the last reset (or clear_flags)."""
        return self.state["flags"].cpu().numpy()

    def clear_flags(self):
        self.state["flags"].zero_()

    def state_to_host(self) -> Dict[str, np.ndarray]:
        out = {n: t.cpu().numpy() for n, t in self.state.items()}
        out["mask"] = out["mask"].view(np.uint32)
        return out
