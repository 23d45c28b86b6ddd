"""Windowed inference (no counterpart in the reference, whose rt_test.py squeezes every frame to the network's square
input): a big frame is cut into overlapping windows, every window runs as one image of the batch, and the people of the
windows are joined in frame pixels on the device, over csrc/ingest.hip (ppn_ingest_windows) and csrc/windows.hip
(ppn_merge_windows).

* ``WindowLayout(src_hw, windows)``        -- up to 16 windows (y0, x0, h, w) of a picture, validated on the host; one
                                              layout serves every frame of a call.  ``WindowLayout.tiles`` builds a grid.
* ``ingest_windows(raw, fmt, layout, ..)`` -- raw NV12 / I420 / YUYV / packed BGR frames -> u8 RGB [F * n, h, w, 3] in one
                                              launch; image f * n + i is window i of frame f.
* ``WindowMerger(layout, frames, ...)``    -- owns the merged buffers; ``merger(result)`` maps the DecodeResult of the F * n
                                              window images to frame pixels, drops the duplicates of the overlaps and fuses
                                              keypoints: one launch, no allocation, no host synchronisation, no D2H.

The rules are include/ppn.h's; tests/windows_ref.py restates them in NumPy.  Not built: letterboxing, more than 16 windows or
512 candidates per frame, InferencePipeline / MultiLaneInference integration, flip-averaging combined with windows.
Rectangles that differ per frame and come from the device are crops.py's (ppn_ingest_rois): a layout stays a host struct.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import torch

from . import config as cfg
from . import decode as D
from . import lib as L

MAX_WINDOWS = L.PPN_MAX_WINDOWS
MAX_CAND = L.PPN_MERGE_MAX_CAND
_PIX_FORMATS = {"nv12": L.PPN_PIX_NV12, "i420": L.PPN_PIX_I420, "yuyv": L.PPN_PIX_YUYV, "bgr": L.PPN_PIX_BGR24}
_YUV_MATRICES = {"bt601": 0, "bt709": 1}


def _dense(name, t, shape, dtype, device):
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()
            and t.device == device):
        raise ValueError(f"{name} must be a contiguous {dtype} tensor {tuple(shape)} on {device}")
    return t


class WindowLayout:
    """The windows of a picture of ``src_hw`` pixels: a sequence of 1..16 ``(y0, x0, h, w)`` in source pixels, each at least
    1 x 1 and inside the picture.  (The YUV formats also need even x0 and w, NV12 / I420 even y0 and h: ``ingest_windows``
    refuses a layout that does not fit its format.)  ``.n`` windows, ``.struct`` the ppn_window_layout."""

    def __init__(self, src_hw, windows: Sequence[Tuple[int, int, int, int]]):
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        H, W = self.src_hw
        if H < 1 or W < 1:
            raise ValueError(f"a picture of {H}x{W} pixels")
        wins = [tuple(int(v) for v in w) for w in windows]
        if not 1 <= len(wins) <= MAX_WINDOWS:
            raise ValueError(f"{len(wins)} windows outside 1..{MAX_WINDOWS}")
        for i, w in enumerate(wins):
            if len(w) != 4:
                raise ValueError(f"window {i} must be (y0, x0, h, w), not {w}")
            y0, x0, h, ww = w
            if h < 1 or ww < 1 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + ww > W:
                raise ValueError(f"window {i} (y0 {y0}, x0 {x0}, {h}x{ww}) is empty or leaves the {H}x{W} picture")
        self.windows = tuple(wins)
        self.n = len(wins)
        self.struct = L.WindowLayout()
        self.struct.n = self.n
        for i, (y0, x0, h, ww) in enumerate(wins):
            self.struct.win[i] = L.Window(y0, x0, h, ww)

    def flipped(self) -> "WindowLayout":
        """The layout of the picture turned by 180 degrees (both axes flipped, as ``ingest_windows(flip=True)`` turns every
        window image): window i (y0, x0, h, w) sits at (H - y0 - h, W - x0 - w) of the turned picture.  The people of
        images ingested with ``flip=True`` are merged with this layout and come out in pixels of the turned picture."""
        H, W = self.src_hw
        return WindowLayout(self.src_hw, [(H - y0 - h, W - x0 - w, h, w) for y0, x0, h, w in self.windows])

    @staticmethod
    def _axis(size: int, count: int, overlap: float):
        """`count` equal spans that cover [0, size): (origins, span).  Neighbours share at least overlap * span - 2."""
        if count == 1:
            return [0], size
        span = size / (count - (count - 1) * overlap)              # count * span - (count - 1) * overlap * span = size
        span = min(2 * math.ceil(span / 2), size)                  # up to an even number: the cover survives the rounding
        step = (size - span) / (count - 1)
        origins = [2 * int(i * step / 2) for i in range(count - 1)] + [size - span]
        return origins, span

    @classmethod
    def tiles(cls, src_hw, rows: int, cols: int, overlap: float = 0.25) -> "WindowLayout":
        """rows x cols equal windows that cover the picture; neighbours share `overlap` of their size (at least
        overlap * size - 2 pixels after the rounding).  Origins and sizes are even numbers, the last row and column end
        exactly at the picture's border; 1 x 1 is the whole picture.  An axis cut into several windows must have an even
        size (even windows cannot end at an odd border): for such a picture give ``WindowLayout`` the windows themselves."""
        rows, cols = int(rows), int(cols)
        if rows < 1 or cols < 1 or rows * cols > MAX_WINDOWS:
            raise ValueError(f"{rows} x {cols} windows: at least 1 x 1, at most {MAX_WINDOWS} in all")
        if not 0.0 <= overlap < 1.0:
            raise ValueError(f"overlap {overlap} outside [0, 1)")
        H, W = int(src_hw[0]), int(src_hw[1])
        if H < rows or W < cols:
            raise ValueError(f"a {H}x{W} picture cannot hold {rows} x {cols} windows")
        if (rows > 1 and H % 2) or (cols > 1 and W % 2):
            raise ValueError(f"a {H}x{W} picture has an odd size along an axis that is cut: even windows cannot end at its border")
        ys, h = cls._axis(H, rows, overlap)
        xs, w = cls._axis(W, cols, overlap)
        return cls((H, W), [(y, x, h, w) for y in ys for x in xs])


def _raw_planes(who: str, raw: torch.Tensor, fmt: str, src_hw, matrix: str, pitch: Optional[int]):
    """What ``ingest_windows`` and ``crops.ingest_rois`` share: the checks of the raw frames and the plane fields of the
    ppn_ingest_desc.  Returns (raw, planes): `raw` as it is read (made contiguous where its rows are not), `planes` the
    descriptor's pitch, pitch_c, frame_stride, y, u, v."""
    from . import rt
    if fmt not in _PIX_FORMATS:
        raise ValueError(f"fmt must be one of {sorted(_PIX_FORMATS)}, not {fmt!r}")
    if matrix not in _YUV_MATRICES:
        raise ValueError(f"matrix must be one of {sorted(_YUV_MATRICES)}, not {matrix!r}")
    if not (isinstance(raw, torch.Tensor) and raw.is_cuda and raw.dtype == torch.uint8):
        raise ValueError(f"{who} expects a uint8 CUDA tensor")
    H, W = int(src_hw[0]), int(src_hw[1])
    base = raw.data_ptr()
    if fmt == "bgr":
        if raw.dim() == 4 and tuple(raw.shape[1:]) == (H, W, 3):
            raw = raw.contiguous().view(raw.shape[0], H, 3 * W)
            base = raw.data_ptr()
        if raw.dim() != 3 or raw.shape[1] != H or raw.stride(2) != 1:
            raise ValueError(f"bgr frames must be u8 [F, {H}, pitch] with rows of unit stride")
        row = 3 * W
        pitch = raw.stride(1) if pitch is None else int(pitch)
        if pitch != raw.stride(1) or raw.shape[2] < row:
            raise ValueError(f"bgr rows hold {raw.shape[2]} bytes at pitch {raw.stride(1)}: need {row} and pitch {pitch}")
        stride = raw.stride(0) if raw.shape[0] > 1 else H * pitch
        planes = dict(pitch=pitch, pitch_c=0, frame_stride=stride, y=base, u=None, v=None)
    else:
        if raw.dim() != 2:
            raise ValueError(f"{fmt} frames must be u8 [F, nbytes]")
        if raw.stride(1) != 1:
            raw = raw.contiguous()
            base = raw.data_ptr()
        nbytes, pitch, pitch_c, u_off, v_off = rt.yuv_frame_layout(fmt, (H, W), pitch)
        if raw.shape[1] < nbytes:
            raise ValueError(f"a {fmt} frame of {(H, W)} with pitch {pitch} has {nbytes} bytes, raw rows have {raw.shape[1]}")
        planes = dict(pitch=pitch, pitch_c=pitch_c, frame_stride=raw.stride(0) if raw.shape[0] > 1 else raw.shape[1], y=base,
                      u=None if u_off is None else base + u_off, v=None if v_off is None else base + v_off)
    return raw, planes


def ingest_windows(raw: torch.Tensor, fmt: str, layout: WindowLayout, size=384, out: Optional[torch.Tensor] = None,
                   flip: bool = False, matrix: str = "bt601", full_range: bool = False,
                   pitch: Optional[int] = None) -> torch.Tensor:
    """The windows of raw video frames -> u8 RGB [F * n, h, w, 3] in one launch (ppn_ingest_windows): every image is what
    ``rt.ingest_yuv`` gives on the window's own crop of the planes.  `raw`: u8 CUDA tensor [F, nbytes] laid out as
    ``rt.yuv_frame_layout(fmt, layout.src_hw, pitch)`` says (`fmt` "nv12", "i420" or "yuyv"), or for `fmt` "bgr" packed
    BGR frames [F, H, pitch] with pitch >= 3 * W bytes per row (a [F, H, W, 3] tensor is taken as it is).  `out` may be
    ``model.input_buffer(F * n, h, w, ...)``."""
    raw, planes = _raw_planes("ingest_windows", raw, fmt, layout.src_hw, matrix, pitch)
    H, W = layout.src_hw
    h, w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    b = raw.shape[0] * layout.n
    if out is None:
        out = torch.empty(b, h, w, 3, dtype=torch.uint8, device=raw.device)
    if tuple(out.shape) != (b, h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor {(b, h, w, 3)}")
    d = L.IngestDesc(format=_PIX_FORMATS[fmt], batch=raw.shape[0], src_h=H, src_w=W, matrix=_YUV_MATRICES[matrix],
                     full_range=int(bool(full_range)), dst=out.data_ptr(), dst_h=h, dst_w=w, flip=int(bool(flip)), dst_bgr=0,
                     **planes)
    L.check(L.load().ppn_ingest_windows(C.byref(d), C.byref(layout.struct), L.current_stream_ptr()), "ppn_ingest_windows")
    return out


class WindowMerger:
    """Joins the people of the windows of `frames` frames (ppn_merge_windows).

        layout = WindowLayout.tiles((1080, 1920), 2, 2)
        merger = WindowMerger(layout, frames, (384, 384), decoder.cfg.max_humans)
        merged = merger(decoder.decode_fused(unary, keys))          # a DecodeResult of `frames` images in frame pixels

    `insize_hw`: the network input the window images were resized to; `max_humans`: the people slots per image of the
    incoming DecodeResult; `max_out`: the slots per frame of the merged one (default: all that can be kept, at most 512).
    `merge_thr`: root-box IoU from which two people of different windows are one; `fuse`: a kept person takes the
    higher-scoring keypoints of its duplicates.  The merged result has ``kp_cell`` = out_src (i * max_humans + p of the
    person a keypoint came from, -1: absent), ``limb_arg`` all -1 and ``max_humans`` = max_out; ``Tracker.update`` and
    ``draw_people`` read ``kp_cell`` only for its sign.  ``.flags``: i32 [frames], PPN_MERGE_FLAG_* of the last call."""

    def __init__(self, layout: WindowLayout, frames: int, insize_hw, max_humans: int, max_out: Optional[int] = None,
                 merge_thr: float = 0.3, fuse: bool = True, K: int = cfg.K, device=None):
        if frames < 1 or not 1 <= max_humans <= L.PPN_MATCH_MAX_PEOPLE:
            raise ValueError(f"{frames} frames x {max_humans} people: at least one each, at most {L.PPN_MATCH_MAX_PEOPLE} people")
        if not 1 <= K <= L.PPN_MAX_KP:
            raise ValueError(f"K {K} outside 1..{L.PPN_MAX_KP}")
        if math.isnan(merge_thr):
            raise ValueError("merge_thr is NaN")
        if max_out is None:
            max_out = min(layout.n * max_humans, MAX_CAND)
        if max_out < 1 or insize_hw[0] < 1 or insize_hw[1] < 1:
            raise ValueError(f"max_out {max_out} and the input size {tuple(insize_hw)} must be at least 1")
        self.layout, self.frames, self.max_humans, self.max_out, self.K = layout, int(frames), int(max_humans), int(max_out), K
        self.cfg = L.MergeCfg(K, int(insize_hw[0]), int(insize_hw[1]), self.max_humans, self.max_out, float(merge_thr),
                              int(bool(fuse)))
        dev = torch.device("cuda" if device is None else device)
        F, Mo = self.frames, self.max_out
        self.flags = torch.zeros(F, dtype=torch.int32, device=dev)
        self.device = self.flags.device
        self.out = D.DecodeResult(
            count=torch.zeros(F, dtype=torch.int32, device=dev),
            kp_cell=torch.full((F, Mo, K), -1, dtype=torch.int32, device=dev),
            limb_arg=torch.full((F, Mo, cfg.E), -1, dtype=torch.int32, device=dev),
            bbox=torch.zeros(F, Mo, K, 4, dtype=torch.float32, device=dev),
            score=torch.zeros(F, Mo, K, dtype=torch.float32, device=dev),
            max_humans=Mo)

    def __call__(self, result: D.DecodeResult) -> D.DecodeResult:
        dev, K, M = self.device, self.K, self.max_humans
        if dev.type != "cuda":
            raise ValueError("WindowMerger runs on the device: its buffers live on " + str(dev))
        B = self.frames * self.layout.n
        if result.max_humans != M:
            raise ValueError(f"result holds {result.max_humans} people per image, the merger expects {M}")
        _dense("result.count", result.count, (B,), torch.int32, dev)
        _dense("result.kp_cell", result.kp_cell, (B, M, K), torch.int32, dev)
        _dense("result.bbox", result.bbox, (B, M, K, 4), torch.float32, dev)
        _dense("result.score", result.score, (B, M, K), torch.float32, dev)
        o = self.out
        L.check(L.load().ppn_merge_windows(C.byref(self.cfg), C.byref(self.layout.struct), result.count.data_ptr(),
                                           result.kp_cell.data_ptr(), result.bbox.data_ptr(), result.score.data_ptr(),
                                           self.frames, o.count.data_ptr(), o.kp_cell.data_ptr(), o.bbox.data_ptr(),
                                           o.score.data_ptr(), self.flags.data_ptr(), L.current_stream_ptr()),
                "ppn_merge_windows")
        return o
