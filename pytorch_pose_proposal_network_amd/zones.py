"""Zones and counting lines on the device (no counterpart in the reference) over csrc/zones.hip: how many people stand in a
polygon, who entered or left it, how long they have been there, and how many crossed a line in which direction -- what a
tracker is installed for, without reading its result back.

* ``Zones(streams, frames, max_humans, ...)``           -- owns the per-stream geometry tables (up to 16 polygons of 3 to 8
                                                           vertices and 16 line segments), the per-stream state (64 tracked
                                                           ids each) and the output buffers.
* ``Zones.set_zones(stream, polygons)`` / ``set_lines`` -- validate on the host and upload one stream's table.
* ``Zones.update(result, tracks, n_frames=None)``       -- one launch on the current stream: the DecodeResult and the
                                                           TrackResult of B = streams * frames images (image s * frames + t is
                                                           frame t of stream s) -> ZoneResult; no allocation, no host
                                                           synchronisation, no D2H.
* ``ZoneResult(slot, inside, zone, line)``              -- per person its slot (-1: none) and the mask of the zones it is in;
                                                           per image and zone (occupancy, entered, exited, loitering); per
                                                           image and line (forward, backward).
* ``Zones.totals()``                                    -- one D2H: the cumulative (entered, exited) and (forward, backward).

Coordinates are in the pixels of the DecodeResult the update is given: the network's input pixels after rt.inference_batch,
frame pixels after rt.inference_windows.  The rules (include/ppn.h, ppn_zone_update) are restated in NumPy by
tests/zones_ref.py.  Zones, lines and their counts are drawn by render.Overlay.  Not built: per-keypoint anchors such as ankles,
more than 16 zones or lines or 8 vertices, hysteresis against a person dithering on a line (net forward - backward stays right), MultiLaneInference
integration.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import config as cfg
from . import decode as D
from . import lib as L
from .validate import _dense

SLOTS = L.PPN_ZONE_SLOTS
ANCHORS = {"center": L.PPN_ZONE_ANCHOR_CENTER, "bottom": L.PPN_ZONE_ANCHOR_BOTTOM}


@dataclass
class ZoneResult:
    """Views of the Zones' output buffers, all on the device; the next update overwrites them."""
    slot: torch.Tensor               # i32 [B, max_humans]   the person's slot, -1: none
    inside: torch.Tensor             # i32 [B, max_humans]   bit z: the person's anchor is in zone z (the bits of a u32)
    zone: torch.Tensor               # i32 [B, 16, 4]        occupancy, entered, exited, loitering
    line: torch.Tensor               # i32 [B, 16, 2]        forward, backward


class Zones:
    """Up to 16 zones and 16 counting lines per stream, and up to 64 tracked ids per stream, resident on the device.

        tracker = Tracker(streams=1, frames=1)
        zones = Zones(streams=1, frames=1, max_gap=tracker.cfg.max_age, loiter=250)
        zones.set_zones(0, [[(40, 200), (340, 200), (340, 380), (40, 380)]])      # x, y in the network's input pixels
        zones.set_lines(0, [(0, 192, 384, 192)])                                  # from A to B; forward: from y < 192 to y >= 192
        for frame in camera:                                                      # u8 [1,S,S,3] on the device
            result, tracks, z = rt.inference_batch_zones(frame, model, tracker, zones, decoder)
            # z.zone[0, 0] = (occupancy, entered, exited, loitering) of zone 0 in this frame; z.line[0, 0] = (forward, backward)
        entered_exited, forward_backward = zones.totals()

    A person's anchor is the centre of its root box (``anchor="center"``; the tracker's smoothed centre when `update` gets
    one) or the middle of the box's lower edge (``"bottom"``: the feet).  An id is held for `max_gap` frames without being
    seen -- the person is taken to be still in its zones -- and a line is tested on the step from the anchor of the last
    frame the id was seen in.  A crossing counts as forward when the new anchor P has (B - A) x (P - A) >= 0, as backward
    otherwise.  `loiter` is the dwell, in frames, from which a person counts as loitering.  `update` takes the
    results of rt.inference_windows plus Tracker.update as they are: then the geometry is in frame pixels.

    Reset a stream (``reset([s])``) when its geometry changes: the state remembers who was inside the OLD zones."""

    def __init__(self, streams: int = 1, frames: int = 1, max_humans: int = 576, K: int = cfg.K, max_gap: int = 15,
                 anchor: str = "center", loiter: int = 1, device="cuda"):
        if streams < 1 or frames < 1 or not 1 <= max_humans <= L.PPN_MATCH_MAX_PEOPLE:
            raise ValueError(f"{streams} streams x {frames} frames x {max_humans} people: at least one each, at most "
                             f"{L.PPN_MATCH_MAX_PEOPLE} people")
        if not 1 <= K <= L.PPN_MAX_KP:
            raise ValueError(f"K {K} outside 1..{L.PPN_MAX_KP}")
        if max_gap < 0 or anchor not in ANCHORS or not 1 <= loiter < 2 ** 31:
            raise ValueError(f"Zones needs max_gap >= 0, anchor in {sorted(ANCHORS)} and loiter >= 1")
        self.streams, self.frames, self.max_humans, self.K = int(streams), int(frames), int(max_humans), int(K)
        self.cfg = L.ZoneCfg(self.K, int(max_gap), ANCHORS[anchor], int(loiter))
        dev = torch.device(device)
        S, B, M = self.streams, self.streams * self.frames, self.max_humans
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        NZ, NV, NL = L.PPN_ZONE_MAX, L.PPN_ZONE_MAX_VERT, L.PPN_LINE_MAX
        self.geom = dict(zone_n=torch.zeros(S, **i32), zone_nv=torch.zeros(S, NZ, **i32),
                         zone_xy=torch.zeros(S, NZ, NV, 2, **f32), line_n=torch.zeros(S, **i32),
                         line_xy=torch.zeros(S, NL, 4, **f32))
        self.state = dict(id=torch.zeros(S, SLOTS, **i32), gap=torch.zeros(S, SLOTS, **i32),
                          inside=torch.zeros(S, SLOTS, **i32), dwell=torch.zeros(S, SLOTS, NZ, **i32),
                          last=torch.zeros(S, SLOTS, 2, **f32), zone_total=torch.zeros(S, NZ, 2, **i32),
                          line_total=torch.zeros(S, NL, 2, **i32), flags=torch.zeros(S, **i32))
        self.device = self.state["id"].device                          # "cuda" resolved to the device the tensors are on
        self.slot = torch.full((B, M), -1, **i32)
        self.inside = torch.zeros(B, M, **i32)
        self.zone = torch.zeros(B, NZ, 4, **i32)
        self.line = torch.zeros(B, NL, 2, **i32)
        self._n_frames = torch.zeros(S, **i32)
        self._geom = L.ZoneGeom(*(self.geom[n].data_ptr() for n, _ in L.ZoneGeom._fields_))
        self._st = L.ZoneState(*(self.state[n].data_ptr() for n, _ in L.ZoneState._fields_))

    # ---- geometry ----------------------------------------------------------------------------------------------------
    def _stream(self, stream) -> int:
        if not 0 <= int(stream) < self.streams:
            raise ValueError(f"stream {stream} outside 0..{self.streams - 1}")
        return int(stream)

    def set_zones(self, stream: int, polygons: Sequence[Sequence[Tuple[float, float]]]):
        """The zones of one stream: at most 16 polygons of 3 to 8 finite (x, y) vertices each, either winding, convex or
        not (the even-odd rule decides).  Reset the stream when its geometry changes."""
        s = self._stream(stream)
        NZ, NV = L.PPN_ZONE_MAX, L.PPN_ZONE_MAX_VERT
        if len(polygons) > NZ:
            raise ValueError(f"{len(polygons)} zones, at most {NZ}")
        nv, xy = np.zeros(NZ, np.int32), np.zeros((NZ, NV, 2), np.float32)
        for z, poly in enumerate(polygons):
            pts = np.asarray(poly, np.float64)
            if pts.ndim != 2 or pts.shape[1] != 2 or not 3 <= pts.shape[0] <= NV:
                raise ValueError(f"zone {z}: 3 to {NV} vertices of (x, y), got an array of shape {pts.shape}")
            with np.errstate(over="ignore"):
                pts = pts.astype(np.float32)
            if not np.isfinite(pts).all():
                raise ValueError(f"zone {z}: a vertex is not a finite float32")
            nv[z], xy[z, :len(pts)] = len(pts), pts
        self.geom["zone_nv"][s].copy_(torch.from_numpy(nv))
        self.geom["zone_xy"][s].copy_(torch.from_numpy(xy))
        self.geom["zone_n"][s] = len(polygons)

    def set_lines(self, stream: int, segments: Sequence[Sequence[float]]):
        """The counting lines of one stream: at most 16 segments (ax, ay, bx, by) of finite values.  Reset the stream when
        its geometry changes."""
        s = self._stream(stream)
        NL = L.PPN_LINE_MAX
        if len(segments) > NL:
            raise ValueError(f"{len(segments)} lines, at most {NL}")
        xy = np.zeros((NL, 4), np.float32)
        for l, seg in enumerate(segments):
            v = np.asarray(seg, np.float64)
            if v.shape != (4,):
                raise ValueError(f"line {l}: (ax, ay, bx, by), got an array of shape {v.shape}")
            with np.errstate(over="ignore"):
                v = v.astype(np.float32)
            if not np.isfinite(v).all():
                raise ValueError(f"line {l}: a value is not a finite float32")
            xy[l] = v
        self.geom["line_xy"][s].copy_(torch.from_numpy(xy))
        self.geom["line_n"][s] = len(segments)

    # ---- the launch --------------------------------------------------------------------------------------------------
    def update(self, result: D.DecodeResult, tracks, n_frames=None, smoothed: bool = True) -> ZoneResult:
        """ppn_zone_update on the current stream.  `tracks`: the TrackResult of the same batch; with anchor "center" its
        smoothed root centre is the anchor when `smoothed` is true and it has one, otherwise the raw box centre.  `n_frames`
        as in Tracker.update."""
        dev = self.device
        if dev.type != "cuda":
            raise ValueError("Zones.update runs on the device: the zones live on " + str(dev))
        B, M, K = self.streams * self.frames, self.max_humans, self.K
        if result.max_humans != M:
            raise ValueError(f"result holds {result.max_humans} people per image, the zones {M}")
        _dense("result.count", result.count, (B,), torch.int32, dev)
        _dense("result.kp_cell", result.kp_cell, (B, M, K), torch.int32, dev)
        _dense("result.bbox", result.bbox, (B, M, K, 4), torch.float32, dev)
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
        L.check(L.load().ppn_zone_update(C.byref(self.cfg), C.byref(self._geom), C.byref(self._st), result.count.data_ptr(),
                                         result.kp_cell.data_ptr(), result.bbox.data_ptr(), tracks.ids.data_ptr(),
                                         xy.data_ptr() if xy is not None else None, self.streams, self.frames, M,
                                         nf.data_ptr() if nf is not None else None, self.slot.data_ptr(),
                                         self.inside.data_ptr(), self.zone.data_ptr(), self.line.data_ptr(),
                                         L.current_stream_ptr()), "ppn_zone_update")
        return ZoneResult(self.slot, self.inside, self.zone, self.line)

    # ---- the state ---------------------------------------------------------------------------------------------------
    def totals(self) -> Tuple[np.ndarray, np.ndarray]:
        """One D2H: (zone_total i32 [S, 16, 2] = entered, exited; line_total i32 [S, 16, 2] = forward, backward) since the
        last reset."""
        both = torch.stack((self.state["zone_total"], self.state["line_total"])).cpu().numpy()
        return both[0], both[1]

    def reset(self, streams: Optional[Sequence[int]] = None):
        """Forget every id, the totals and the flags: of all streams, or of the named ones.  The geometry stays."""
        if streams is None:
            for t in self.state.values():
                t.zero_()
            return
        for s in streams:
            self._stream(s)
            for t in self.state.values():
                t[int(s)].zero_()

    def flags(self) -> np.ndarray:
        """One D2H: per stream the OR of PPN_ZONE_FLAG_SLOT_OVERFLOW since the last reset (or clear_flags)."""
        return self.state["flags"].cpu().numpy()

    def clear_flags(self):
        self.state["flags"].zero_()

    def state_to_host(self) -> Dict[str, np.ndarray]:
        out = {n: t.cpu().numpy() for n, t in self.state.items()}
        out["inside"] = out["inside"].view(np.uint32)
        return out
