"""Drawing the decoded people on the device (reference: datatest.py:162-232, `draw_humans`) over csrc/render.hip.

* ``draw_people(frames_u8, result)``     -- the device path: u8 RGB frames [B,H,W,3] + the DecodeResult as it lives on the
                                            device -> drawn frames, on the current stream, no host synchronisation.
* ``Renderer(batch, max_humans)``        -- owns the workspace for a fixed geometry so repeated calls allocate nothing.
* ``Renderer.draw_yuv(raw, fmt, src_hw, result)`` / ``draw_people_yuv`` -- the same people painted straight onto raw NV12 /
                                            I420 / YUYV frames (ppn_draw_humans_yuv), in place or into a second surface.
* ``Overlay(frames, scale, tick, plates, colours)`` -- the monitoring picture on top of the people (ppn_draw_scene): pass
                                            ``overlay=`` with ``tracks=`` (ids as labels, boxes in the id's colour) and / or
                                            ``zones=`` (zones, counting lines, occupancy and running totals, coloured by
                                            this frame's ZoneResult) to ``Renderer.__call__`` / ``Renderer.draw_yuv``.
* ``draw_humans(keypoint_names, edges, pil_image, humans, ...)`` -- same name / arguments / return as datatest.py:162.

The pixels are the ones PIL's ImageDraw paints for the reference's calls (rules and deviations: include/ppn.h,
ppn_draw_humans; NumPy restatement tests/render_ref.py; the overlay's: tests/overlay_ref.py).  The reference's ``mask=``
paste is not built; nor are alpha-blended zone fill, trails and text other than the overlay's 16 glyphs.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import config as cfg
from . import decode as D
from . import lib as L


def default_palette(keypoint_names: Sequence[str] = cfg.KEYPOINT_NAMES):
    return [cfg.COLOR_MAP[n] for n in keypoint_names]


def make_cfg(visbbox: bool = False, grid: bool = False, grid_step: int = 16, palette=None, kp_order=None,
             edges=None, num_keypoints: Optional[int] = None) -> L.DrawCfg:
    """ppn_draw_cfg for the skeleton of config.py (or `edges` / `num_keypoints` / `kp_order` of another one)."""
    edges = cfg.EDGES if edges is None else [tuple(e) for e in edges]
    K = cfg.K if num_keypoints is None else int(num_keypoints)
    palette = default_palette() if palette is None else palette
    kp_order = (cfg.kp_paint_order() if K == cfg.K else list(range(K))) if kp_order is None else list(kp_order)
    if not 1 <= K <= L.PPN_MAX_KP or len(edges) > L.PPN_MAX_EDGES:
        raise ValueError(f"{K} keypoints / {len(edges)} edges: at most {L.PPN_MAX_KP} / {L.PPN_MAX_EDGES}")
    if len(palette) != K or any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in palette):
        raise ValueError(f"palette must hold {K} (r, g, b) triples in 0..255")
    if len(kp_order) != K or any(not 0 <= int(k) < K for k in kp_order):
        raise ValueError(f"kp_order must hold {K} keypoint indices")
    if any(not (0 <= int(s) < K and 0 <= int(t) < K) for s, t in edges):
        raise ValueError("edges must join keypoint indices")
    if grid and int(grid_step) < 1:
        raise ValueError(f"grid_step {grid_step} < 1")
    c = L.DrawCfg()
    c.K, c.E = K, len(edges)
    for i, (s, t) in enumerate(edges):
        c.edge_src[i], c.edge_dst[i] = int(s), int(t)
    for i in range(K):
        c.kp_order[i] = int(kp_order[i])
        for j in range(3):
            c.palette[i][j] = int(palette[i][j])
    c.visbbox, c.grid, c.grid_step = int(bool(visbbox)), int(bool(grid)), int(grid_step) if grid else 1
    return c


ID_COLOURS = [(230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240),
              (240, 50, 230), (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200),
              (128, 0, 0), (170, 255, 195)]
DEFAULT_COLOURS = dict(zone=(64, 160, 255), line=(255, 200, 0), id=ID_COLOURS, active=(0, 255, 0), alert=(255, 0, 0),
                       text=(255, 255, 255), plate=(0, 0, 0))


class Overlay:
    """What ppn_draw_scene paints over the people (include/ppn.h): per tracked person the root outline in the id's colour
    and the id as a label; per zone its outline and occupancy; per counting line the segment, a tick on the side a forward
    crossing ends on and the running totals "forward:backward".  `frames`: frames per stream in the batch (the tracker's and
    the zones'); `scale` 1..4: the size of a glyph pixel; `tick`: the tick's length in pixels; `plates`: a filled box under
    each text.  `colours`: a dict overriding DEFAULT_COLOURS -- "zone", "line" and "id" take one (r, g, b) or 16 of them
    (zone z, line l, id & 15); "active" marks an occupied zone or a line crossed in this frame, "alert" a zone somebody
    loiters in; "text" and "plate" are the labels'."""

    def __init__(self, frames: int = 1, scale: int = 1, tick: float = 8.0, plates: bool = True, colours=None):
        if int(frames) < 1 or not 1 <= int(scale) <= 4:
            raise ValueError(f"Overlay needs frames >= 1 and scale in 1..4, got {frames} and {scale}")
        tick = float(tick)
        if not 0.0 <= tick <= float(np.finfo(np.float32).max):
            raise ValueError(f"tick {tick} must be a finite float32 >= 0")
        unknown = set(colours or ()) - set(DEFAULT_COLOURS)
        if unknown:
            raise ValueError(f"unknown overlay colours {sorted(unknown)}: {sorted(DEFAULT_COLOURS)}")
        self.frames, self.scale, self.tick, self.plates = int(frames), int(scale), tick, bool(plates)
        self.colours = dict(DEFAULT_COLOURS, **(colours or {}))
        for name in ("zone", "line", "id"):
            v = self.colours[name]
            self.colours[name] = [tuple(v)] * 16 if len(v) == 3 and not hasattr(v[0], "__len__") else [tuple(c) for c in v]
            if len(self.colours[name]) != 16:
                raise ValueError(f"colours[{name!r}] must be one (r, g, b) or 16 of them")
        for name in ("active", "alert", "text", "plate"):
            self.colours[name] = tuple(self.colours[name])
        every = [c for n in ("zone", "line", "id") for c in self.colours[n]] + [self.colours[n] for n in
                                                                                 ("active", "alert", "text", "plate")]
        if any(len(c) != 3 or min(c) < 0 or max(c) > 255 for c in every):
            raise ValueError("overlay colours must be (r, g, b) triples in 0..255")

    def cfg(self) -> L.OverlayCfg:
        c = L.OverlayCfg(frames=self.frames, scale=self.scale, tick=self.tick, plates=int(self.plates))
        for name, field in (("zone", c.zone_colour), ("line", c.line_colour), ("id", c.id_colour)):
            for i in range(16):
                for j in range(3):
                    field[i][j] = int(self.colours[name][i][j])
        for name in ("active", "alert", "text", "plate"):
            for j in range(3):
                getattr(c, name)[j] = int(self.colours[name][j])
        return c


def _check_frames(frames_u8, out):
    if not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8:
        raise ValueError("frames must be a uint8 tensor [B,H,W,3]")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or not frames_u8.is_contiguous():
        raise ValueError(f"frames must be a contiguous [B,H,W,3] tensor, got {tuple(frames_u8.shape)}")
    if not frames_u8.is_cuda:
        raise ValueError("frames must live on the device")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != frames_u8.shape
                            or not out.is_contiguous() or out.device != frames_u8.device):
        raise ValueError("out must be a contiguous uint8 tensor of the frames' shape on their device")


class Renderer:
    """Owns the rasteriser's workspace (48 bytes per person and slot) for a fixed (batch, max_humans); a call only
    enqueues two launches on the current stream."""

    def __init__(self, batch: int, max_humans: int, device="cuda"):
        self.lib = L.load()
        self.batch, self.max_humans = int(batch), int(max_humans)
        ws = self.lib.ppn_draw_scene_workspace_bytes(C.byref(make_cfg()), self.batch, self.max_humans)   # people + overlay
        if ws == 0:
            raise ValueError(f"bad renderer geometry: batch {batch}, max_humans {max_humans}")
        self.workspace = torch.empty(ws // 4, dtype=torch.int32, device=torch.device(device))
        self._n_frames = None                                           # device copy of a host n_frames, made on first use

    def __call__(self, frames_u8: torch.Tensor, result: D.DecodeResult, visbbox: bool = False, gridOn: bool = False,
                 out: Optional[torch.Tensor] = None, palette=None, outsize=None, *, overlay: Optional[Overlay] = None,
                 tracks=None, zones=None, zone_result=None, n_frames=None) -> torch.Tensor:
        """Draw `result`'s people onto `frames_u8` (u8 RGB [B,H,W,3] on the device).  out=None: a new tensor; out=frames_u8:
        in place; any other `out` is overwritten entirely.  gridOn adds the reference's cell grid with step
        int(W / outW), `outsize` = (outW, outH) defaulting to config.OUTSIZE.  Returns the drawn tensor.

        With an `overlay` (an Overlay) the monitoring picture goes on top of the people (ppn_draw_scene, still two launches,
        nothing read back): `tracks` (a track.TrackResult of this batch) labels every tracked person with its id; `zones` (the
        zones.Zones that was updated with this batch, its geometry in the frames' pixels) draws zones, lines and counts from
        `zone_result` (default: the Zones' own output buffers, i.e. its last update); `n_frames` as in Tracker.update: an
        image that was not processed gets no overlay.  Either part may be absent."""
        _check_frames(frames_u8, out)
        step = int(frames_u8.shape[2] / (outsize if outsize is not None else cfg.OUTSIZE)[0]) if gridOn else 1
        scene = self._scene(frames_u8.shape[0], result, overlay, tracks, zones, zone_result, n_frames)
        return self._draw_rgb(frames_u8, result, make_cfg(visbbox, gridOn, step, palette), out, scene)

    def _scene(self, B: int, result: D.DecodeResult, overlay, tracks, zones, zone_result, n_frames):
        """(ppn_overlay_cfg, ppn_overlay_in) of a call, None without an overlay."""
        if overlay is None:
            if tracks is not None or zones is not None or zone_result is not None or n_frames is not None:
                raise ValueError("tracks, zones, zone_result and n_frames belong to an overlay: pass overlay=render.Overlay(...)")
            return None
        from .validate import _dense
        dev, M = self.workspace.device, self.max_humans
        if B % overlay.frames:
            raise ValueError(f"{B} images are no multiple of the overlay's {overlay.frames} frames per stream")
        S = B // overlay.frames
        oin = L.OverlayIn()
        if tracks is not None:
            oin.ids = _dense("tracks.ids", tracks.ids, (B, M), torch.int32, dev).data_ptr()
        if zones is not None:
            if zones.streams != S or zones.frames != overlay.frames:
                raise ValueError(f"the zones hold {zones.streams} streams x {zones.frames} frames, the overlay {S} x {overlay.frames}")
            zone = zones.zone if zone_result is None else zone_result.zone
            line = zones.line if zone_result is None else zone_result.line
            _dense("zone_result.zone", zone, (B, L.PPN_ZONE_MAX, 4), torch.int32, dev)
            _dense("zone_result.line", line, (B, L.PPN_LINE_MAX, 2), torch.int32, dev)
            for n, _ in L.ZoneGeom._fields_:
                if zones.geom[n].device != dev:
                    raise ValueError("the zones live on another device than the renderer")
                setattr(oin.geom, n, zones.geom[n].data_ptr())
            oin.out_zone, oin.out_line = zone.data_ptr(), line.data_ptr()
            oin.line_total = zones.state["line_total"].data_ptr()
        elif zone_result is not None:
            raise ValueError("zone_result needs the zones it came from (their geometry and totals)")
        if n_frames is not None:
            if isinstance(n_frames, torch.Tensor) and n_frames.device == dev:
                nf = _dense("n_frames", n_frames, (S,), torch.int32, dev)
            else:
                host = torch.as_tensor(n_frames, dtype=torch.int32).reshape(-1)
                if host.numel() != S:
                    raise ValueError(f"{host.numel()} frame counts for {S} streams")
                if self._n_frames is None or self._n_frames.numel() != S:
                    self._n_frames = torch.zeros(S, dtype=torch.int32, device=dev)
                self._n_frames.copy_(host)
                nf = self._n_frames
            oin.n_frames = nf.data_ptr()
        return overlay.cfg(), oin

    def _check_result(self, B: int, result: D.DecodeResult):
        m = result.max_humans
        if B != self.batch or m != self.max_humans:
            raise ValueError(f"renderer built for batch {self.batch} x {self.max_humans} people, got {B} x {m}")
        if tuple(result.count.shape) != (B,) or tuple(result.kp_cell.shape) != (B, m, cfg.K) or \
                tuple(result.bbox.shape) != (B, m, cfg.K, 4):
            raise ValueError("result does not hold count [B], kp_cell [B,M,K] and bbox [B,M,K,4]")

    def _draw_rgb(self, frames_u8: torch.Tensor, result: D.DecodeResult, c: L.DrawCfg, out: Optional[torch.Tensor],
                  scene=None):
        B, H, W, _ = frames_u8.shape
        self._check_result(B, result)
        m = result.max_humans
        if out is None:
            out = torch.empty_like(frames_u8)
        elif out.data_ptr() != frames_u8.data_ptr():
            lo, hi = sorted((out.data_ptr(), frames_u8.data_ptr()))
            if lo + frames_u8.numel() > hi:
                raise ValueError("out must be the frames themselves or not overlap them")
        people = (B, H, W, result.count.data_ptr(), result.kp_cell.data_ptr(), result.bbox.data_ptr(), m,
                  self.workspace.data_ptr(), L.current_stream_ptr())
        if scene is None:
            L.check(self.lib.ppn_draw_humans(C.byref(c), frames_u8.data_ptr(), out.data_ptr(), *people), "ppn_draw_humans")
        else:
            L.check(self.lib.ppn_draw_scene(C.byref(c), C.byref(scene[0]), C.byref(scene[1]), frames_u8.data_ptr(),
                                            out.data_ptr(), *people), "ppn_draw_scene")
        return out

    def draw_yuv(self, raw: torch.Tensor, fmt: str, src_hw, result: D.DecodeResult, visbbox: bool = False,
                 grid_step: int = 0, out: Optional[torch.Tensor] = None, palette=None, pitch: Optional[int] = None,
                 matrix: str = "bt601", full_range: bool = False, *, overlay: Optional[Overlay] = None, tracks=None,
                 zones=None, zone_result=None, n_frames=None) -> torch.Tensor:
        """Draw `result`'s people (frame pixels, e.g. ``rt.inference_windows``' result) straight onto raw video frames
        (ppn_draw_humans_yuv: no RGB intermediate, unpainted samples keep their bytes).  `raw`: u8 CUDA tensor [F, nbytes],
        one frame per row laid out as ``rt.yuv_frame_layout(fmt, src_hw, pitch)`` says (`fmt` "nv12", "i420" or "yuyv";
        rows may be longer than a frame); `matrix` / `full_range` name the surface's colour set as for ``rt.ingest_yuv``.
        out=raw: in place.  out=None: a new tensor of raw's shape -- a copy of raw (the bytes outside the frames' content
        included) that is then drawn in place.  Any other `out` must have raw's shape and not overlap it; the kernel writes
        every content byte of it and nothing else.  grid_step > 0 adds the grid at that step.  `fmt` "bgr": packed BGR
        frames [F, H * W * 3] (or [F, H, W, 3]) of tight pitch, served by the RGB rasteriser with the palette's channels
        swapped.  `overlay`, `tracks`, `zones`, `zone_result` and `n_frames` as in ``__call__`` (ppn_draw_scene_yuv; for
        "bgr" the overlay's colours are swapped like the palette's).  Returns the drawn tensor."""
        from . import rt
        if not (isinstance(raw, torch.Tensor) and raw.is_cuda and raw.dtype == torch.uint8):
            raise ValueError("draw_yuv expects a uint8 CUDA tensor")
        H, W = int(src_hw[0]), int(src_hw[1])
        grid_step = int(grid_step)
        if grid_step < 0:
            raise ValueError(f"grid_step {grid_step} < 0")
        if fmt == "bgr":
            if pitch is not None and int(pitch) != 3 * W:
                raise ValueError(f"bgr frames are drawn at the tight pitch {3 * W} only, not {pitch}")
            shape = (raw.shape[0], H, W, 3)
            if not raw.is_contiguous() or raw.numel() != raw.shape[0] * H * W * 3:
                raise ValueError(f"bgr frames must be contiguous with {H * W * 3} bytes each")
            if out is not None and (not isinstance(out, torch.Tensor) or out.shape != raw.shape):
                raise ValueError("out must have raw's shape")
            swapped = [tuple(c)[::-1] for c in (default_palette() if palette is None else palette)]
            frames, to = raw.view(shape), None if out is None else out.view(shape)
            _check_frames(frames, to)
            scene = self._scene(raw.shape[0], result, overlay, tracks, zones, zone_result, n_frames)
            if scene is not None:
                for name, _ in L.OverlayCfg._fields_[4:]:
                    field = getattr(scene[0], name)
                    for c4 in ([field] if name in ("active", "alert", "text", "plate") else field):
                        c4[0], c4[2] = c4[2], c4[0]
            drawn = self._draw_rgb(frames, result, make_cfg(visbbox, grid_step > 0, grid_step, swapped), to, scene)
            return drawn.view(raw.shape) if out is None else out
        if matrix not in rt._YUV_MATRICES:
            raise ValueError(f"matrix must be one of {sorted(rt._YUV_MATRICES)}, not {matrix!r}")
        nbytes, pitch, pitch_c, u_off, v_off = rt.yuv_frame_layout(fmt, (H, W), pitch)
        if raw.dim() != 2 or raw.stride(1) != 1 or raw.shape[1] < nbytes:
            raise ValueError(f"{fmt} frames of {(H, W)} with pitch {pitch} must be u8 [F, >= {nbytes}] with rows of unit stride")
        F, m = raw.shape[0], result.max_humans
        self._check_result(F, result)
        c = make_cfg(visbbox, grid_step > 0, grid_step, palette)
        if out is None:
            out = raw = raw.clone()
        elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.device == raw.device and
                  out.shape == raw.shape and out.stride(1) == 1):
            raise ValueError("out must be a uint8 tensor of raw's shape on its device with rows of unit stride")
        elif out.data_ptr() != raw.data_ptr() or out.stride(0) != raw.stride(0):
            span = lambda t: (t.data_ptr(), t.data_ptr() + (t.shape[0] - 1) * t.stride(0) + t.shape[1])
            (a0, a1), (b0, b1) = span(raw), span(out)
            if a0 < b1 and b0 < a1:
                raise ValueError("out must be raw itself or not overlap it")

        def surface(t):
            base = t.data_ptr()
            return L.YuvSurface(format=rt._PIX_FORMATS[fmt], height=H, width=W, pitch=pitch, pitch_c=pitch_c,
                                frame_stride=t.stride(0) if F > 1 else t.shape[1], y=base,
                                u=None if u_off is None else base + u_off, v=None if v_off is None else base + v_off,
                                matrix=rt._YUV_MATRICES[matrix], full_range=int(bool(full_range)))
        scene = self._scene(F, result, overlay, tracks, zones, zone_result, n_frames)
        people = (F, result.count.data_ptr(), result.kp_cell.data_ptr(), result.bbox.data_ptr(), m, self.workspace.data_ptr(),
                  L.current_stream_ptr())
        if scene is None:
            L.check(self.lib.ppn_draw_humans_yuv(C.byref(c), C.byref(surface(raw)), C.byref(surface(out)), *people),
                    "ppn_draw_humans_yuv")
        else:
            L.check(self.lib.ppn_draw_scene_yuv(C.byref(c), C.byref(scene[0]), C.byref(scene[1]), C.byref(surface(raw)),
                                                C.byref(surface(out)), *people), "ppn_draw_scene_yuv")
        return out


def draw_people_yuv(raw: torch.Tensor, fmt: str, src_hw, result: D.DecodeResult, visbbox: bool = False, grid_step: int = 0,
                    out: Optional[torch.Tensor] = None, palette=None, pitch: Optional[int] = None, matrix: str = "bt601",
                    full_range: bool = False) -> torch.Tensor:
    """One-off ``Renderer.draw_yuv`` call (allocates the workspace; keep a Renderer for repeated use).  Runs on the current
    stream without a host synchronisation."""
    if not (isinstance(raw, torch.Tensor) and raw.is_cuda and raw.dim() >= 2):
        raise ValueError("draw_people_yuv expects a uint8 CUDA tensor [F, nbytes]")
    return Renderer(raw.shape[0], result.max_humans, raw.device).draw_yuv(raw, fmt, src_hw, result, visbbox, grid_step, out,
                                                                          palette, pitch, matrix, full_range)


def draw_people(frames_u8: torch.Tensor, result: D.DecodeResult, visbbox: bool = False, gridOn: bool = False,
                out: Optional[torch.Tensor] = None, palette=None, outsize=None) -> torch.Tensor:
    """One-off Renderer call (allocates the workspace; keep a Renderer for repeated use).  Runs on the current stream
    without a host synchronisation."""
    _check_frames(frames_u8, out)
    return Renderer(frames_u8.shape[0], result.max_humans, frames_u8.device)(frames_u8, result, visbbox, gridOn, out,
                                                                            palette, outsize)


def pack_humans(humans, num_keypoints: int = cfg.K):
    """The reference's list of {keypoint: [ymin, xmin, ymax, xmax]} dicts -> (count i32[1], kp_cell i32[1,M,K],
    bbox f32[1,M,K,4]) NumPy arrays, M = max(len(humans), 1)."""
    n, K = len(humans), num_keypoints
    count = np.array([n], np.int32)
    kp_cell = np.full((1, max(n, 1), K), -1, np.int32)
    bbox = np.zeros((1, max(n, 1), K, 4), np.float32)
    for i, hm in enumerate(humans):
        for k, b in hm.items():
            if not 0 <= int(k) < K:
                raise ValueError(f"person {i}: keypoint {k} is not in 0..{K - 1}")
            kp_cell[0, i, int(k)] = 0
            bbox[0, i, int(k)] = np.asarray(b, np.float32)
    return count, kp_cell, bbox


def draw_humans(keypoint_names, edges, pil_image, humans, mask=None, visbbox=False, gridOn=False):
    """Drop-in for datatest.py:162-232: draws `humans` onto `pil_image` (a PIL image, updated and returned as the reference
    does; or a u8 HxWx3 array, then a new array is returned) with the HIP rasteriser -- the dicts are packed, one frame
    goes to the device and comes back.

    Keypoints are always painted in config.kp_paint_order(), the order get_humans_by_feature builds its dicts in, not in
    the dicts' own order; the grid step is int(width / decode.outsize[0]).  `mask` is not built."""
    if mask is not None:
        raise NotImplementedError("draw_humans: the mask= paste of the reference is not built")
    K = len(keypoint_names)
    c = make_cfg(visbbox, gridOn, 1, default_palette(keypoint_names), None, edges, K)   # validates before any device work
    is_array = isinstance(pil_image, np.ndarray)
    img = np.array(pil_image if is_array else pil_image.convert("RGB"), order="C")     # a writable copy
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError("draw_humans expects an RGB image (u8 HxWx3)")
    H, W, _ = img.shape
    if gridOn:
        c.grid_step = int(W / D.outsize[0])
        if c.grid_step < 1:
            raise ValueError(f"image width {W} is below the grid's {D.outsize[0]} cells")
    count, kp_cell, bbox = pack_humans(humans, K)
    lib = L.load()
    dev = torch.device("cuda")
    frame = torch.from_numpy(img).unsqueeze(0).to(dev)
    ws = torch.empty(max(lib.ppn_draw_workspace_bytes(C.byref(c), 1, kp_cell.shape[1]), 16) // 4, dtype=torch.int32,
                     device=dev)
    cd, kd, bd = (torch.from_numpy(a).to(dev) for a in (count, kp_cell, bbox))
    L.check(lib.ppn_draw_humans(C.byref(c), frame.data_ptr(), frame.data_ptr(), 1, H, W, cd.data_ptr(), kd.data_ptr(),
                                bd.data_ptr(), kp_cell.shape[1], ws.data_ptr(), L.current_stream_ptr()),
            "ppn_draw_humans")
    drawn = frame[0].cpu().numpy()
    if is_array:
        return drawn
    from PIL import Image
    pil_image.paste(Image.fromarray(drawn).convert(pil_image.mode))
    return pil_image
