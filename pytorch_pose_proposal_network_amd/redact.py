"""Redaction (no counterpart in the reference): the detected people -- by default their heads -- made unrecognisable in the
RAW frames before they leave the box, in the format the encoder takes, over csrc/redact.hip (ppn_redact_cells,
ppn_redact_yuv).

* ``Redactor(streams, frames, max_humans, src_hw, fmt, ..)`` -- owns the hold state, the masks and the flags of
                                  `streams` x `frames` images (image s * frames + t is frame t of stream s, the tracker's
                                  layout).  ``.cells(result)`` turns a DecodeResult's people into per-frame bit masks over
                                  a grid of `cell` x `cell` pixels (one launch); a cell stays masked for `hold` more frames
                                  after the last detection that covered it, from call to call.  ``.apply(raw, out)`` pixelates
                                  ("mosaic": every sample set of a masked cell becomes its rounded mean) or fills the masked
                                  cells of NV12 / I420 / YUYV / packed BGR frames, in place or into `out` (one launch).
                                  ``redactor(raw, result, out)`` does both; ``.reset()`` forgets the hold state.  No
                                  allocation, no host synchronisation, no D2H: the pair replays from a captured graph.
* ``redact_people_yuv(raw, fmt, src_hw, result, ..)`` -- a one-off with a fresh state.

The rules are include/ppn.h's; tests/redact_ref.py restates them in NumPy.  Not built: blur, ellipses, a per-track hold that
follows a moving person, MultiLaneInference integration.  No claim is made about how well the neck + top boxes cover a
face: the synthetic checkpoints say nothing about that.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import config as cfg
from . import decode as D
from . import lib as L
from .windows import _PIX_FORMATS, _YUV_MATRICES, _dense

BAD_BOX = L.PPN_REDACT_FLAG_BAD_BOX
CELLS = (8, 16, 32)
_FALLBACKS = {"person": L.PPN_REDACT_FALLBACK_PERSON, "none": L.PPN_REDACT_FALLBACK_NONE}
_MODES = {"mosaic": L.PPN_REDACT_MOSAIC, "fill": L.PPN_REDACT_FILL}
_EVEN = {"nv12": (2, 2), "i420": (2, 2), "yuyv": (1, 2), "bgr": (1, 1)}          # what the picture's size must divide by


def kp_mask_of(parts, K: int = cfg.K) -> int:
    """ppn_redact_cells_cfg.kp_mask for `parts`: "head" (neck and top), "person" (every keypoint) or a sequence of
    config.KEYPOINT_NAMES."""
    if isinstance(parts, str):
        if parts not in ("head", "person"):
            raise ValueError(f"parts must be 'head', 'person' or a sequence of keypoint names, not {parts!r}")
        names = ("neck", "top") if parts == "head" else cfg.KEYPOINT_NAMES[:K]
    else:
        names = tuple(parts)
    bits = 0
    for n in names:
        if n not in cfg.KEYPOINT_NAMES or cfg.KEYPOINT_NAMES.index(n) >= K:
            raise ValueError(f"parts: {n!r} is not one of the first {K} of config.KEYPOINT_NAMES")
        bits |= 1 << cfg.KEYPOINT_NAMES.index(n)
    if not bits:
        raise ValueError("parts names no keypoint")
    return bits


def grid_of(src_hw, cell: int):
    """(CH, CW, MW): rows and columns of cells and mask words per row."""
    ch, cw = -(-int(src_hw[0]) // cell), -(-int(src_hw[1]) // cell)
    return ch, cw, -(-cw // 32)


class Redactor:
    """Redacts the people of `streams` x `frames` raw frames.

        red = Redactor(1, 8, decoder.cfg.max_humans, (1080, 1920), "nv12", coords_hw=(384, 384))
        res = rt.inference_batch(rt.ingest_yuv(raw, "nv12", (1080, 1920)), model, decoder)
        red(raw, res, out=raw)                                          # heads pixelated in place, held for 8 frames

    `max_humans`: the people slots per image of the incoming DecodeResult; `src_hw`, `fmt`: the raw frames ("nv12", "i420",
    "yuyv" or "bgr"); `cell`: 8, 16 or 32 pixels; `parts`: "head" (neck and top), "person" or keypoint names; `margin`:
    added to each half size of the region as a fraction of it; `fallback`: what a person without any of `parts` gets --
    "person": the union of all its keypoints, "none": nothing; `hold`: 0..254 frames a cell stays masked after it was last
    covered; `mode` "mosaic" or "fill" with `fill_rgb`, converted once with the surface's `matrix` / `full_range`
    (ppn_rgb_to_yuv).  `coords_hw`: the space the boxes are in -- the network input for a plain decode, None (= `src_hw`)
    for a WindowMerger's result."""

    def __init__(self, streams: int, frames: int, max_humans: int, src_hw, fmt: str, cell: int = 16, parts="head",
                 margin: float = 0.25, fallback: str = "person", hold: int = 8, mode: str = "mosaic", fill_rgb=(0, 0, 0),
                 coords_hw=None, matrix: str = "bt601", full_range: bool = False, K: int = cfg.K, device=None):
        if fmt not in _EVEN:
            raise ValueError(f"fmt must be one of {sorted(_EVEN)}, not {fmt!r}")
        if fallback not in _FALLBACKS:
            raise ValueError(f"fallback must be one of {sorted(_FALLBACKS)}, not {fallback!r}")
        if mode not in _MODES:
            raise ValueError(f"mode must be one of {sorted(_MODES)}, not {mode!r}")
        if matrix not in _YUV_MATRICES:
            raise ValueError(f"matrix must be one of {sorted(_YUV_MATRICES)}, not {matrix!r}")
        if cell not in CELLS:
            raise ValueError(f"cell must be one of {CELLS}, not {cell!r}")
        if streams < 1 or frames < 1 or streams * frames > 65535 or not 1 <= max_humans <= L.PPN_MATCH_MAX_PEOPLE:
            raise ValueError(f"{streams} streams x {frames} frames x {max_humans} people: at least one each, at most 65535 "
                             f"images and {L.PPN_MATCH_MAX_PEOPLE} people")
        if not 1 <= K <= L.PPN_MAX_KP:
            raise ValueError(f"K {K} outside 1..{L.PPN_MAX_KP}")
        if not (isinstance(hold, int) and 0 <= hold <= 254):
            raise ValueError(f"hold {hold!r} outside 0..254")
        if not (math.isfinite(margin) and margin >= 0):
            raise ValueError(f"margin {margin} must be finite and not negative")
        fill_rgb = tuple(int(v) for v in fill_rgb)
        if len(fill_rgb) != 3 or min(fill_rgb) < 0 or max(fill_rgb) > 255:
            raise ValueError(f"fill_rgb must be (r, g, b) in 0..255, not {fill_rgb}")
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.coords_hw = self.src_hw if coords_hw is None else (int(coords_hw[0]), int(coords_hw[1]))
        ey, ex = _EVEN[fmt]
        if (min(self.src_hw) < 1 or max(self.src_hw) > 16384 or min(self.coords_hw) < 1 or self.src_hw[0] % ey
                or self.src_hw[1] % ex):
            raise ValueError(f"a {fmt} picture of {self.src_hw} with boxes in {self.coords_hw}: sizes must be in 1..16384 and "
                             "the picture even where the format shares chroma")
        self.streams, self.frames, self.batch = int(streams), int(frames), int(streams) * int(frames)
        self.max_humans, self.K, self.fmt, self.cell, self.hold = int(max_humans), int(K), fmt, int(cell), hold
        self.matrix, self.full_range = matrix, bool(full_range)
        f32 = np.float32
        self.cfg = L.RedactCellsCfg(self.K, self.max_humans, self.src_hw[0], self.src_hw[1], self.cell,
                                    float(f32(self.src_hw[0]) / f32(self.coords_hw[0])),
                                    float(f32(self.src_hw[1]) / f32(self.coords_hw[1])), kp_mask_of(parts, self.K),
                                    _FALLBACKS[fallback], float(margin), hold)
        self.lib = L.load()
        if fmt == "bgr":
            fill = fill_rgb[::-1]
        else:
            rgb = (C.c_uint8 * 3)(*fill_rgb)
            L.check(self.lib.ppn_rgb_to_yuv(_YUV_MATRICES[matrix], int(self.full_range), rgb, rgb, 1), "ppn_rgb_to_yuv")
            fill = tuple(rgb)
        self.fill = tuple(int(v) for v in fill)
        self.apply_cfg = L.RedactCfg(self.cell, _MODES[mode], (C.c_uint8 * 4)(*self.fill, 0))
        dev = torch.device("cuda" if device is None else device)
        self.CH, self.CW, self.MW = grid_of(self.src_hw, self.cell)
        self.ttl = torch.zeros(self.streams, self.CH, self.CW, dtype=torch.uint8, device=dev)
        self.mask = torch.zeros(self.batch, self.CH, self.MW, dtype=torch.int32, device=dev)     # the words' bits; u32 in C
        self.flags = torch.zeros(self.batch, dtype=torch.int32, device=dev)
        self.device = self.ttl.device

    def reset(self):
        """Forget the hold state: the next frame is the first."""
        self.ttl.zero_()

    def cells(self, result: D.DecodeResult) -> torch.Tensor:
        """ppn_redact_cells on the current stream: the masks of `result`'s people, the hold state moved on by `frames`
        frames per stream.  Returns the mask tensor i32 [streams * frames, CH, MW]."""
        dev, K, M, B = self.device, self.K, self.max_humans, self.batch
        if dev.type != "cuda":
            raise ValueError("Redactor runs on the device: its buffers live on " + str(dev))
        if result.max_humans != M:
            raise ValueError(f"result holds {result.max_humans} people per image, the redactor expects {M}")
        _dense("result.count", result.count, (B,), torch.int32, dev)
        _dense("result.kp_cell", result.kp_cell, (B, M, K), torch.int32, dev)
        _dense("result.bbox", result.bbox, (B, M, K, 4), torch.float32, dev)
        L.check(self.lib.ppn_redact_cells(C.byref(self.cfg), self.ttl.data_ptr() if self.hold else None,
                                          result.count.data_ptr(), result.kp_cell.data_ptr(), result.bbox.data_ptr(),
                                          self.streams, self.frames, self.mask.data_ptr(), self.flags.data_ptr(),
                                          L.current_stream_ptr()), "ppn_redact_cells")
        return self.mask

    def apply(self, raw: torch.Tensor, out: Optional[torch.Tensor] = None, pitch: Optional[int] = None) -> torch.Tensor:
        """ppn_redact_yuv on the current stream: the masked cells of `raw` redacted.  `raw` and `out` exactly as
        ``render.Renderer.draw_yuv`` takes them: u8 CUDA tensor [F, nbytes] laid out as ``rt.yuv_frame_layout(fmt, src_hw,
        pitch)`` says, for "bgr" packed frames [F, H * W * 3] or [F, H, W, 3] of tight pitch; out=raw: in place; out=None:
        a copy of raw that is redacted in place; any other `out` has raw's shape, does not overlap it, and gets every
        content byte written.  Returns the redacted tensor."""
        from . import rt
        if not (isinstance(raw, torch.Tensor) and raw.is_cuda and raw.dtype == torch.uint8 and raw.dim() >= 2):
            raise ValueError("apply expects a uint8 CUDA tensor [F, nbytes]")
        if raw.shape[0] != self.batch:
            raise ValueError(f"raw holds {raw.shape[0]} frames, the redactor {self.batch}")
        H, W = self.src_hw
        fmt, shape = self.fmt, raw.shape
        if out is not None and not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.device == raw.device
                                    and out.shape == raw.shape):
            raise ValueError("out must be a uint8 tensor of raw's shape on its device")
        if fmt == "bgr":
            if pitch is not None and int(pitch) != 3 * W:
                raise ValueError(f"bgr frames are redacted at the tight pitch {3 * W} only, not {pitch}")
            if not raw.is_contiguous() or raw.numel() != shape[0] * H * W * 3 or (out is not None and not out.is_contiguous()):
                raise ValueError(f"bgr frames must be contiguous with {H * W * 3} bytes each")
            raw = raw.view(shape[0], H * W * 3)
            out = None if out is None else out.view(shape[0], H * W * 3)
            nbytes, pitch, pitch_c, u_off, v_off = H * W * 3, 3 * W, 0, None, None
        else:
            nbytes, pitch, pitch_c, u_off, v_off = rt.yuv_frame_layout(fmt, (H, W), pitch)
        if raw.dim() != 2 or raw.stride(1) != 1 or raw.shape[1] < nbytes:
            raise ValueError(f"{fmt} frames of {(H, W)} with pitch {pitch} must be u8 [F, >= {nbytes}] with rows of unit stride")
        if out is None:
            out = raw = raw.clone()
        elif out.stride(1) != 1:
            raise ValueError("out must have rows of unit stride")
        elif out.data_ptr() != raw.data_ptr() or out.stride(0) != raw.stride(0):
            span = lambda t: (t.data_ptr(), t.data_ptr() + (t.shape[0] - 1) * t.stride(0) + t.shape[1])
            (a0, a1), (b0, b1) = span(raw), span(out)
            if a0 < b1 and b0 < a1:
                raise ValueError("out must be raw itself or not overlap it")
        F = self.batch

        def surface(t):
            base = t.data_ptr()
            return L.YuvSurface(format=_PIX_FORMATS[fmt], height=H, width=W, pitch=pitch, pitch_c=pitch_c,
                                frame_stride=t.stride(0) if F > 1 else t.shape[1], y=base,
                                u=None if u_off is None else base + u_off, v=None if v_off is None else base + v_off,
                                matrix=_YUV_MATRICES[self.matrix], full_range=int(self.full_range))
        L.check(self.lib.ppn_redact_yuv(C.byref(self.apply_cfg), C.byref(surface(raw)), C.byref(surface(out)), F,
                                        self.mask.data_ptr(), L.current_stream_ptr()), "ppn_redact_yuv")
        return out.view(shape)

    def __call__(self, raw: torch.Tensor, result: D.DecodeResult, out: Optional[torch.Tensor] = None,
                 pitch: Optional[int] = None) -> torch.Tensor:
        self.cells(result)
        return self.apply(raw, out, pitch)


def redact_people_yuv(raw: torch.Tensor, fmt: str, src_hw, result: D.DecodeResult, out: Optional[torch.Tensor] = None,
                      pitch: Optional[int] = None, streams: Optional[int] = None, **kw) -> torch.Tensor:
    """One-off ``Redactor`` call with a fresh hold state (allocates the state; keep a Redactor for a video).  The F frames
    of `raw` are F streams of one frame each unless `streams` says otherwise; `kw` are Redactor's keyword arguments.  Runs
    on the current stream without a host synchronisation."""
    if not (isinstance(raw, torch.Tensor) and raw.is_cuda and raw.dim() >= 2):
        raise ValueError("redact_people_yuv expects a uint8 CUDA tensor [F, nbytes]")
    F = raw.shape[0]
    streams = F if streams is None else int(streams)
    if streams < 1 or F % streams:
        raise ValueError(f"{F} frames do not split into {streams} streams")
    return Redactor(streams, F // streams, result.max_humans, src_hw, fmt, device=raw.device, **kw)(raw, result, out, pitch)
