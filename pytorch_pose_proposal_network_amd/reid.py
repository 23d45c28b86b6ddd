"""Re-identification by appearance on the device (no counterpart in the reference) over csrc/reid.hip: a small integer
colour descriptor per person, read straight from the RAW frame, and a gallery per stream that gives every person a
PERSISTENT id -- one that survives a change of track id when the appearance matches somebody recently lost (a person who
walked behind a pillar for longer than the tracker's max_age, or moved too far between two frames).

* ``ReId(streams, frames, max_humans, src_hw, fmt, ..)`` -- owns the rectangle table, the descriptors, the gallery state (128
                                  entries per stream) and the outputs of B = streams * frames images (image s * frames + t
                                  is frame t of stream s, the tracker's layout).
* ``.rects(result)``           -- ppn_people_rois: the people's rectangles in source pixels (one launch).
* ``.describe(raw, pitch)``    -- ppn_people_descr: per rectangle 3 bands x 3 channels x 8 bins of sample counts from the
                                  NV12 / I420 / YUYV / packed BGR frame, without a colour conversion (one launch).
* ``.update(result, tracks)``  -- ppn_reid_update: the gallery moved on by the batch -> ReIdResult (one launch).
* ``.reid(raw, result, tracks)`` -- all three: three launches, no allocation, no host synchronisation, no D2H; the triple
                                  replays from a captured graph with the gallery carried over.
* ``ReIdResult.as_tracks(tracks)`` -- a TrackResult whose ids are the persistent ids: ``PoseClips.push``, ``Zones.update``
                                  and ``Renderer(..., tracks=)`` take it unchanged, so clips, dwell times and the drawn
                                  numbers follow the person across a track break.

The rules are include/ppn.h's; tests/reid_ref.py restates them in NumPy.  NO CLAIM is made about identification accuracy:
the descriptor is a colour histogram, the synthetic checkpoints and planted crowds say nothing about real clothing, and the
default ``sim_thr`` is a guess, not a measurement.  Not built: a learned embedding, identities across streams, more than 128
entries per stream, a motion model, MultiLaneInference integration.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import config as cfg
from . import decode as D
from . import lib as L
from .crops import _ALIGN, _MODES
from .track import TrackResult
from .windows import _PIX_FORMATS, _YUV_MATRICES, _dense, _raw_planes

SLOTS = L.PPN_REID_SLOTS
DESCR_LEN = L.PPN_DESCR_LEN
SIM_MAX = L.PPN_REID_SIM_MAX


@dataclass
class ReIdResult:
    """Views of the ReId's buffers, all on the device; the next call overwrites them."""
    pid: torch.Tensor                # i32 [B, max_humans]     persistent id of person p, -1: none
    sim: torch.Tensor                # i32 [B, max_humans]     the similarity a person was relinked with, -1: it was not
    live: torch.Tensor               # i32 [B]                 live gallery entries after the frame, -1: frame not processed
    descr: torch.Tensor              # i16 [B, max_rois, 72]   the counts (0..1024), [band][channel][bin]; u16 in C
    valid: torch.Tensor              # i32 [B, max_rois]       1: the slot has a descriptor
    roi: torch.Tensor                # i32 [B, max_rois, 4]    (y0, x0, h, w) in source pixels
    status: torch.Tensor             # i32 [B, max_rois]       ppn_people_rois' status

    def to_host(self) -> Dict[str, np.ndarray]:
        """One read-back of all seven arrays (descr as uint16)."""
        parts = [(n, getattr(self, n)) for n in ("pid", "sim", "live", "descr", "valid", "roi", "status")]
        flat = torch.cat([t.reshape(-1).view(torch.uint8) for _, t in parts]).cpu().numpy()
        out, at = {}, 0
        for n, t in parts:
            nb = t.numel() * t.element_size()
            out[n] = flat[at:at + nb].view(np.uint16 if n == "descr" else np.int32).reshape(tuple(t.shape)).copy()
            at += nb
        return out

    def as_tracks(self, tracks: TrackResult) -> TrackResult:
        """The tracker's result with the persistent ids in place of the track ids; hits, xy, live and count are the
        tracker's."""
        return TrackResult(self.pid, tracks.hits, tracks.xy, tracks.live, tracks.count)


class ReId:
    """Persistent ids for the people of `streams` x `frames` raw frames.

        tracker = Tracker(streams=1, frames=1, max_humans=decoder.cfg.max_humans)
        reid = ReId(1, 1, decoder.cfg.max_humans, (1080, 1920), "nv12", coords_hw=(384, 384))
        for raw in camera:                                             # u8 [1, nbytes] NV12 on the device
            res, tracks, rid = rt.inference_reid(raw, "nv12", (1080, 1920), model, tracker, reid, decoder=decoder)
            clips.push(res, rid.as_tracks(tracks))                     # a clip follows the person, not the track

    `max_humans`: the people slots per image of the incoming DecodeResult; `src_hw`, `fmt`: the raw frames ("nv12", "i420",
    "yuyv" or "bgr"); `coords_hw`: the space the boxes are in -- the network input for a plain decode, None (= `src_hw`) for a
    WindowMerger's result; `max_rois`: the first so many people of an image get a descriptor (the others still get ids, but
    can only be followed by track id); `mode`, `margin`, `min_size`: the rectangle, as PersonCropper's (no aspect rule).
    `sim_thr`: the histogram intersection, as a fraction of its maximum, from which a lost entry is taken up again -- a
    guess, not a measurement; `min_lost`: frames an entry must have been unseen before it can be; `memory`: frames an unseen
    entry is kept; `blend_shift`: a new descriptor enters the entry's with weight 2^-blend_shift.  `matrix` / `full_range`
    name the surface as the siblings do; no colour is converted."""

    def __init__(self, streams: int, frames: int, max_humans: int, src_hw, fmt: str, coords_hw=None, max_rois: int = 64,
                 mode: str = "people", margin: float = 0.0, min_size: int = 8, sim_thr: float = 0.7, min_lost: int = 1,
                 memory: int = 300, blend_shift: int = 2, matrix: str = "bt601", full_range: bool = False, K: int = cfg.K,
                 device=None):
        if fmt not in _ALIGN:
            raise ValueError(f"fmt must be one of {sorted(_ALIGN)}, not {fmt!r}")
        if mode not in _MODES:
            raise ValueError(f"mode must be one of {sorted(_MODES)}, not {mode!r}")
        if matrix not in _YUV_MATRICES:
            raise ValueError(f"matrix must be one of {sorted(_YUV_MATRICES)}, not {matrix!r}")
        if streams < 1 or frames < 1 or max_rois < 1 or not 1 <= max_humans <= L.PPN_MATCH_MAX_PEOPLE:
            raise ValueError(f"{streams} streams x {frames} frames x {max_humans} people x {max_rois} rois: at least one each, "
                             f"at most {L.PPN_MATCH_MAX_PEOPLE} people")
        if streams * frames * max_rois > 65535:
            raise ValueError(f"{streams * frames} images x {max_rois} rois exceed 65535 descriptors")
        if not 1 <= K <= L.PPN_MAX_KP:
            raise ValueError(f"K {K} outside 1..{L.PPN_MAX_KP}")
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.coords_hw = self.src_hw if coords_hw is None else (int(coords_hw[0]), int(coords_hw[1]))
        ay, ax = _ALIGN[fmt]
        if (min(self.src_hw) < 1 or max(self.src_hw) > 16384 or min(self.coords_hw) < 1 or self.src_hw[0] % ay
                or self.src_hw[1] % ax):
            raise ValueError(f"a {fmt} picture of {self.src_hw} with boxes in {self.coords_hw}: sizes must be in 1..16384 and "
                             "the picture even where the format shares chroma")
        if not (math.isfinite(margin) and margin >= 0) or min_size < max(1, ay, ax):
            raise ValueError(f"margin {margin} must be finite and not negative, min_size {min_size} at least {max(1, ay, ax)}")
        if not (math.isfinite(sim_thr) and 0.0 <= sim_thr <= 1.0):
            raise ValueError(f"sim_thr {sim_thr} outside 0..1")
        if min_lost < 1 or not 0 <= memory < 2 ** 31 or not 0 <= blend_shift <= 4:
            raise ValueError("ReId needs min_lost >= 1, memory >= 0 and blend_shift in 0..4")
        self.streams, self.frames, self.batch = int(streams), int(frames), int(streams) * int(frames)
        self.max_humans, self.max_rois, self.K, self.fmt = int(max_humans), int(max_rois), int(K), fmt
        self.matrix, self.full_range = matrix, bool(full_range)
        f32 = np.float32
        self.roi_cfg = L.RoiCfg(self.K, self.max_humans, self.max_rois, self.src_hw[0], self.src_hw[1],
                                float(f32(self.src_hw[0]) / f32(self.coords_hw[0])),
                                float(f32(self.src_hw[1]) / f32(self.coords_hw[1])), _MODES[mode], float(margin), 0.0, ay, ax,
                                int(min_size))
        self.thr = min(int(math.ceil(sim_thr * SIM_MAX)), SIM_MAX)
        self.cfg = L.ReIdCfg(self.thr, int(min_lost), int(memory), int(blend_shift), self.max_rois)
        dev = torch.device("cuda" if device is None else device)
        S, B, M, R = self.streams, self.batch, self.max_humans, self.max_rois
        i32 = dict(dtype=torch.int32, device=dev)
        i16 = dict(dtype=torch.int16, device=dev)                     # the bits of the u16 counts
        self.roi = torch.zeros(B, R, 4, **i32)
        self.status = torch.full((B, R), L.PPN_ROI_EMPTY, **i32)
        self.descr = torch.zeros(B, R, DESCR_LEN, **i16)
        self.valid = torch.zeros(B, R, **i32)
        self.state = dict(pid=torch.zeros(S, SLOTS, **i32), tid=torch.zeros(S, SLOTS, **i32), lost=torch.zeros(S, SLOTS, **i32),
                          n=torch.zeros(S, SLOTS, **i32), descr=torch.zeros(S, SLOTS, DESCR_LEN, **i16),
                          last_pid=torch.zeros(S, **i32), flags=torch.zeros(S, **i32))
        self.device = self.roi.device
        self.pid = torch.full((B, M), -1, **i32)
        self.sim = torch.full((B, M), -1, **i32)
        self.live = torch.full((B,), -1, **i32)
        self._n_frames = torch.zeros(S, **i32)
        self._st = L.ReIdState(*(self.state[n].data_ptr() for n, _ in L.ReIdState._fields_))
        self.out = ReIdResult(self.pid, self.sim, self.live, self.descr, self.valid, self.roi, self.status)

    def _on_device(self, what: str):
        if self.device.type != "cuda":
            raise ValueError(f"ReId.{what} runs on the device: its buffers live on {self.device}")

    # ---- the three launches ------------------------------------------------------------------------------------------
    def rects(self, result: D.DecodeResult) -> ReIdResult:
        """ppn_people_rois on the current stream: the rectangles and status of `result`'s people."""
        self._on_device("rects")
        dev, K, M, B = self.device, self.K, self.max_humans, self.batch
        if result.max_humans != M:
            raise ValueError(f"result holds {result.max_humans} people per image, the ReId expects {M}")
        _dense("result.count", result.count, (B,), torch.int32, dev)
        _dense("result.kp_cell", result.kp_cell, (B, M, K), torch.int32, dev)
        _dense("result.bbox", result.bbox, (B, M, K, 4), torch.float32, dev)
        L.check(L.load().ppn_people_rois(C.byref(self.roi_cfg), result.count.data_ptr(), result.kp_cell.data_ptr(),
                                         result.bbox.data_ptr(), B, self.roi.data_ptr(), self.status.data_ptr(),
                                         L.current_stream_ptr()), "ppn_people_rois")
        return self.out

    def describe(self, raw: torch.Tensor, pitch: Optional[int] = None) -> ReIdResult:
        """ppn_people_descr on the current stream: the descriptors of the rectangles ``rects`` wrote, read from `raw` --
        u8 frames on the device as ``windows.ingest_windows`` takes them: [B, nbytes] laid out as
        ``rt.yuv_frame_layout(fmt, src_hw, pitch)`` says, for "bgr" [B, H, pitch] or [B, H, W, 3]."""
        self._on_device("describe")
        if not (isinstance(raw, torch.Tensor) and raw.dim() >= 2 and raw.shape[0] == self.batch):
            raise ValueError(f"raw must hold {self.batch} frames")
        raw, planes = _raw_planes("ReId.describe", raw, self.fmt, self.src_hw, self.matrix, pitch)
        surf = L.YuvSurface(format=_PIX_FORMATS[self.fmt], height=self.src_hw[0], width=self.src_hw[1],
                            matrix=_YUV_MATRICES[self.matrix], full_range=int(self.full_range), **planes)
        L.check(L.load().ppn_people_descr(C.byref(surf), self.batch, self.roi.data_ptr(), self.status.data_ptr(),
                                          self.max_rois, self.descr.data_ptr(), self.valid.data_ptr(),
                                          L.current_stream_ptr()), "ppn_people_descr")
        return self.out

    def update(self, result: D.DecodeResult, tracks: TrackResult, n_frames=None) -> ReIdResult:
        """ppn_reid_update on the current stream: the gallery moved on by the batch, with the descriptors ``describe``
        wrote.  `tracks`: the TrackResult of the same batch; `n_frames` as in Tracker.update."""
        self._on_device("update")
        dev, B, M = self.device, self.batch, self.max_humans
        if result.max_humans != M:
            raise ValueError(f"result holds {result.max_humans} people per image, the ReId expects {M}")
        _dense("result.count", result.count, (B,), torch.int32, dev)
        _dense("tracks.ids", tracks.ids, (B, M), torch.int32, dev)
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
        L.check(L.load().ppn_reid_update(C.byref(self.cfg), C.byref(self._st), result.count.data_ptr(), tracks.ids.data_ptr(),
                                         self.descr.data_ptr(), self.valid.data_ptr(), self.streams, self.frames, M,
                                         nf.data_ptr() if nf is not None else None, self.pid.data_ptr(), self.sim.data_ptr(),
                                         self.live.data_ptr(), L.current_stream_ptr()), "ppn_reid_update")
        return self.out

    def reid(self, raw: torch.Tensor, result: D.DecodeResult, tracks: TrackResult, n_frames=None,
             pitch: Optional[int] = None) -> ReIdResult:
        """rects, describe and update: three launches on the current stream."""
        self.rects(result)
        self.describe(raw, pitch)
        return self.update(result, tracks, n_frames)

    __call__ = reid

    # ---- the state ---------------------------------------------------------------------------------------------------
    def reset(self, streams: Optional[Sequence[int]] = None):
        """Forget every entry, the pid counter and the flags: of all streams, or of the named ones."""
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
        """One D2H: per stream the OR of PPN_REID_FLAG_SLOT_OVERFLOW since the last reset (or clear_flags)."""
        return self.state["flags"].cpu().numpy()

    def clear_flags(self):
        self.state["flags"].zero_()

    def state_to_host(self) -> Dict[str, np.ndarray]:
        out = {n: t.cpu().numpy() for n, t in self.state.items()}
        out["descr"] = out["descr"].view(np.uint16)
        return out
