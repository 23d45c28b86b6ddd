"""Tracking people across the frames of a video on the device (no counterpart in the reference, whose rt_test.py treats
every frame on its own) over csrc/track.hip.

* ``Tracker(streams, frames, max_humans, ...)``  -- owns the per-stream track state (64 slots each) and the output buffers.
* ``Tracker.update(result, n_frames=None)``      -- one launch on the current stream: the DecodeResult of B = streams * frames
                                                    images (image s * frames + t is frame t of stream s) -> TrackResult; no
                                                    allocation, no host synchronisation, no D2H.
* ``TrackResult(ids, hits, xy, live)``           -- per person its track id (-1: untracked) and the track's hit count, the
                                                    smoothed keypoint centres, and per image the number of live tracks.

The rules (greedy matching by close keypoints, then IoU; exponential smoothing; ageing; births) are include/ppn.h's,
ppn_track_update; tests/track_ref.py restates them in NumPy.  Re-identification by appearance -- an id that
survives the death of a track -- is reid.py's, which takes a TrackResult.  Not built: a motion model, colouring drawn people
by id, InferencePipeline / MultiLaneInference integration, more than 64 tracks per stream.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import config as cfg
from . import decode as D
from . import lib as L
from .validate import _dense

SLOTS = L.PPN_TRACK_SLOTS
MAX_DET = L.PPN_TRACK_MAX_DET


@dataclass
class TrackResult:
    """Views of the Tracker's output buffers, all on the device; the next update overwrites them."""
    ids: torch.Tensor                # i32 [B, max_humans]        track id of person p, -1: untracked / no such person
    hits: torch.Tensor               # i32 [B, max_humans]        frames the track has been matched in, 0 where ids is -1
    xy: Optional[torch.Tensor]       # f32 [B, max_humans, K, 2]  (x, y) centres, smoothed for tracked people; None if unwanted
    live: torch.Tensor               # i32 [B]                    live tracks after the frame, -1: frame not processed
    count: torch.Tensor              # i32 [B]                    the DecodeResult's people counts (rows of xy that are written)

    def to_host(self) -> List[Dict[str, np.ndarray]]:
        """One read-back: per image ids[:n], hits[:n], xy[:n] (None if unwanted) and live, n = the image's people."""
        cnt = self.count.cpu().numpy()
        m = self.ids.shape[1]
        top = int(min(max(cnt.max(initial=0), 0), m))
        ids, hits = self.ids[:, :top].cpu().numpy(), self.hits[:, :top].cpu().numpy()
        xy = self.xy[:, :top].cpu().numpy() if self.xy is not None else None
        live = self.live.cpu().numpy()
        out = []
        for b in range(len(cnt)):
            n = int(min(max(cnt[b], 0), m)) if live[b] >= 0 else 0
            out.append(dict(ids=ids[b, :n].copy(), hits=hits[b, :n].copy(), xy=None if xy is None else xy[b, :n].copy(),
                            live=int(live[b])))
        return out


class Tracker:
    """Up to 64 tracks per stream, resident on the device.

        tracker = Tracker(streams=1, frames=1)
        for frame in camera:                                         # u8 [1,S,S,3] on the device
            result, tracks = rt.inference_batch_tracked(frame, model, tracker, decoder)
            # tracks.ids[0, p] follows the human that person p of this frame is

    iou_thr / kp_gate / min_close decide whether a person may continue a track (root-box IoU, or at least min_close
    keypoints within kp_gate * sqrt(track root area) of the track's), max_age how many frames a track survives unseen,
    birth_thr the root score a person needs to start one, alpha the weight of the new observation in the smoothed centres
    (1.0: no smoothing)."""

    def __init__(self, streams: int = 1, frames: int = 1, max_humans: int = 576, K: int = cfg.K, iou_thr: float = 0.3,
                 kp_gate: float = 0.1, min_close: int = 3, max_age: int = 15, birth_thr: float = 0.0, alpha: float = 1.0,
                 device="cuda"):
        if streams < 1 or frames < 1 or not 1 <= max_humans <= L.PPN_MATCH_MAX_PEOPLE:
            raise ValueError(f"{streams} streams x {frames} frames x {max_humans} people: at least one each, at most "
                             f"{L.PPN_MATCH_MAX_PEOPLE} people")
        if not 1 <= K <= L.PPN_MAX_KP:
            raise ValueError(f"K {K} outside 1..{L.PPN_MAX_KP}")
        vals = (iou_thr, kp_gate, birth_thr, alpha)
        if (not all(math.isfinite(v) for v in vals) or not 0.0 <= iou_thr <= 1.0 or kp_gate < 0 or not 0.0 < alpha <= 1.0
                or min_close < 1 or max_age < 0):
            raise ValueError("Tracker needs finite values, iou_thr in [0, 1], kp_gate >= 0, alpha in (0, 1], min_close >= 1 "
                             "and max_age >= 0")
        self.streams, self.frames, self.max_humans, self.K = int(streams), int(frames), int(max_humans), int(K)
        self.cfg = L.TrackCfg(self.K, int(min_close), int(max_age), float(iou_thr), float(kp_gate), float(birth_thr),
                              float(alpha))
        dev = torch.device(device)
        S, B, M = self.streams, self.streams * self.frames, self.max_humans
        i32 = dict(dtype=torch.int32, device=dev)
        self.state = dict(id=torch.zeros(S, SLOTS, **i32), miss=torch.zeros(S, SLOTS, **i32),
                          hits=torch.zeros(S, SLOTS, **i32), mask=torch.zeros(S, SLOTS, **i32),
                          root=torch.zeros(S, SLOTS, 4, dtype=torch.float32, device=dev),
                          xy=torch.zeros(S, SLOTS, self.K, 2, dtype=torch.float32, device=dev),
                          last_id=torch.zeros(S, **i32), flags=torch.zeros(S, **i32))
        self.device = self.state["id"].device                          # "cuda" resolved to the device the tensors are on
        self.ids = torch.full((B, M), -1, **i32)
        self.hits = torch.zeros(B, M, **i32)
        self.xy = torch.zeros(B, M, self.K, 2, dtype=torch.float32, device=dev)
        self.live = torch.full((B,), -1, **i32)
        self._n_frames = torch.zeros(S, **i32)
        self._st = L.TrackState(*(self.state[n].data_ptr() for n, _ in L.TrackState._fields_))

    def update(self, result: D.DecodeResult, n_frames=None, want_xy: bool = True) -> TrackResult:
        """ppn_track_update on the current stream.  `n_frames`: None, or per stream the number of leading frames that
        count (an i32 [streams] tensor on the device is used as it is; anything else is copied into the Tracker's own)."""
        dev = self.device
        if dev.type != "cuda":
            raise ValueError("Tracker.update runs on the device: the tracker lives on " + str(dev))
        B, M, K = self.streams * self.frames, self.max_humans, self.K
        if result.max_humans != M:
            raise ValueError(f"result holds {result.max_humans} people per image, the tracker {M}")
        _dense("result.count", result.count, (B,), torch.int32, dev)
        _dense("result.kp_cell", result.kp_cell, (B, M, K), torch.int32, dev)
        _dense("result.bbox", result.bbox, (B, M, K, 4), torch.float32, dev)
        _dense("result.score", result.score, (B, M, K), torch.float32, dev)
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
        L.check(L.load().ppn_track_update(C.byref(self.cfg), C.byref(self._st), result.count.data_ptr(),
                                          result.kp_cell.data_ptr(), result.bbox.data_ptr(), result.score.data_ptr(),
                                          self.streams, self.frames, M, nf.data_ptr() if nf is not None else None,
                                          self.ids.data_ptr(), self.hits.data_ptr(),
                                          self.xy.data_ptr() if want_xy else None, self.live.data_ptr(),
                                          L.current_stream_ptr()), "ppn_track_update")
        return TrackResult(self.ids, self.hits, self.xy if want_xy else None, self.live, result.count)

    def reset(self, streams: Optional[Sequence[int]] = None):
        """Forget every track, the id counter and the flags: of all streams, or of the named ones."""
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
        """One D2H: per stream the OR of PPN_TRACK_FLAG_DET_OVERFLOW / PPN_TRACK_FLAG_SLOT_OVERFLOW since the last reset
        (or clear_flags)."""
        return self.state["flags"].cpu().numpy()

    def clear_flags(self):
        self.state["flags"].zero_()

    def state_to_host(self) -> Dict[str, np.ndarray]:
        out = {n: t.cpu().numpy() for n, t in self.state.items()}
        out["mask"] = out["mask"].view(np.uint32)
        return out
