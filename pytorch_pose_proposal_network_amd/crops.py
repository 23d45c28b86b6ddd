"""Person crops (no counterpart in the reference, whose rt_test.py stops at the drawn frame): every detected person cut out
of the RAW frame as a fixed-size picture for a following model (re-identification, action recognition, a face or hand
network), over csrc/crops.hip (ppn_people_rois) and csrc/ingest.hip (ppn_ingest_rois).

* ``ingest_rois(raw, fmt, src_hw, roi, size, ..)`` -- raw NV12 / I420 / YUYV / packed BGR frames and a DEVICE table of
                                                      rectangles i32 [F, R, 4] (y0, x0, h, w) -> u8 RGB [F * R, h, w, 3] in
                                                      one launch; image f * R + r is rectangle r of frame f.  An all-zero
                                                      or bad rectangle gives a black image and a status bit, never a read.
* ``PersonCropper(frames, max_humans, src_hw, ..)`` -- owns the roi, status and crop buffers.  ``.rois(result)`` writes the
                                                      rectangles of a DecodeResult's people (one launch), ``.crop(raw)``
                                                      cuts them out (one launch), ``cropper(raw, result)`` does both: no
                                                      allocation, no host synchronisation, no D2H; the pair can be captured
                                                      into a graph and replayed on new frames and people.
* ``CropResult(crops, roi, status)``               -- views of the cropper's buffers; crop r of frame f is PERSON r of the
                                                      DecodeResult (and of a Tracker's ids), there is no sorting.

The rules are include/ppn.h's; tests/crops_ref.py restates them in NumPy.  A rectangle is the person's box with its margin
and the output's aspect, INTERSECTED with the picture: at a border it is neither shifted nor padded.  Not built: padding or
letterboxing, normalised float output, running the network on the crops, MultiLaneInference integration, flip-averaging
combined with crops.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from . import config as cfg
from . import decode as D
from . import lib as L
from .windows import _PIX_FORMATS, _YUV_MATRICES, _dense, _raw_planes

OK, EMPTY, DEGENERATE, BAD = L.PPN_ROI_OK, L.PPN_ROI_EMPTY, L.PPN_ROI_DEGENERATE, L.PPN_ROI_BAD
_MODES = {"root": L.PPN_ROI_MODE_ROOT, "people": L.PPN_ROI_MODE_PEOPLE}
_ALIGN = {"nv12": (2, 2), "i420": (2, 2), "yuyv": (1, 2), "bgr": (1, 1)}          # (align_y, align_x): where chroma is shared


def ingest_rois(raw: torch.Tensor, fmt: str, src_hw, roi: torch.Tensor, size, out: Optional[torch.Tensor] = None,
                status: Optional[torch.Tensor] = None, flip: bool = False, matrix: str = "bt601", full_range: bool = False,
                pitch: Optional[int] = None) -> torch.Tensor:
    """Rectangles of raw video frames -> u8 RGB [F * R, h, w, 3] in one launch (ppn_ingest_rois): every image is what
    ``windows.ingest_windows`` gives for a layout of that one rectangle.  `raw`, `fmt`, `matrix`, `full_range` and `pitch`
    as ``ingest_windows`` takes them; `roi`: i32 [F, R, 4] (y0, x0, h, w) in source pixels ON THE DEVICE, from any source --
    it is judged there: an all-zero rectangle (an empty slot) and a bad one (outside the picture, not even where the
    format shares chroma) give an all-zero image.  `status`: None, or i32 [F, R] into which PPN_ROI_EMPTY / PPN_ROI_BAD are
    OR-ed."""
    raw, planes = _raw_planes("ingest_rois", raw, fmt, src_hw, matrix, pitch)
    dev = raw.device
    if not (isinstance(roi, torch.Tensor) and roi.dim() == 3):
        raise ValueError("roi must be an int32 tensor [F, R, 4] on the device")
    F_, R = raw.shape[0], roi.shape[1]
    _dense("roi", roi, (F_, R, 4), torch.int32, dev)
    if status is not None:
        _dense("status", status, (F_, R), torch.int32, dev)
    h, w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if out is None:
        out = torch.empty(F_ * R, h, w, 3, dtype=torch.uint8, device=dev)
    if (out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev or out.numel() != F_ * R * h * w * 3
            or tuple(out.shape[-3:]) != (h, w, 3)):
        raise ValueError(f"out must be a contiguous uint8 tensor {(F_ * R, h, w, 3)} on {dev}")
    d = L.IngestDesc(format=_PIX_FORMATS[fmt], batch=F_, src_h=int(src_hw[0]), src_w=int(src_hw[1]),
                     matrix=_YUV_MATRICES[matrix], full_range=int(bool(full_range)), dst=out.data_ptr(), dst_h=h, dst_w=w,
                     flip=int(bool(flip)), dst_bgr=0, **planes)
    L.check(L.load().ppn_ingest_rois(C.byref(d), roi.data_ptr(), R, None if status is None else status.data_ptr(),
                                     L.current_stream_ptr()), "ppn_ingest_rois")
    return out


@dataclass
class CropResult:
    """Views of the PersonCropper's buffers, all on the device; the next call overwrites them."""
    crops: torch.Tensor              # u8  [F, max_crops, h, w, 3]  RGB; all zero where status != 0
    roi: torch.Tensor                # i32 [F, max_crops, 4]        (y0, x0, h, w) in source pixels, zeros where status != 0
    status: torch.Tensor             # i32 [F, max_crops]           0: a crop; PPN_ROI_EMPTY / _DEGENERATE / _BAD bits

    def to_host(self) -> List[Dict[str, np.ndarray]]:
        """One read-back: per frame the valid crops (status 0) as ``slot`` (the person's index), ``roi`` and ``crops``."""
        F_, R = self.status.shape
        flat = torch.cat([self.status.reshape(-1).view(torch.uint8), self.roi.reshape(-1).view(torch.uint8),
                          self.crops.reshape(-1)]).cpu().numpy()
        status = flat[:F_ * R * 4].view(np.int32).reshape(F_, R)
        roi = flat[F_ * R * 4:F_ * R * 20].view(np.int32).reshape(F_, R, 4)
        crops = flat[F_ * R * 20:].reshape(self.crops.shape)
        out = []
        for f in range(F_):
            slot = np.flatnonzero(status[f] == OK)
            out.append(dict(slot=slot, roi=roi[f, slot].copy(), crops=crops[f, slot].copy()))
        return out


class PersonCropper:
    """Cuts the people of `frames` frames out of the raw frames they were found in.

        cropper = PersonCropper(frames, decoder.cfg.max_humans, (1080, 1920), "nv12", (256, 128), coords_hw=(384, 384))
        res = rt.inference_batch(rt.ingest_yuv(raw, "nv12", (1080, 1920)), model, decoder)
        out = cropper(raw, res)                                        # out.crops[f, r]: person r of frame f, 256 x 128

    `max_humans`: the people slots per image of the incoming DecodeResult; `src_hw`, `fmt`: the raw frames; `out_hw`: the
    size of a crop; `max_crops`: the first so many people of a frame get one.  `mode` "people": the union of a person's
    keypoint boxes, "root": the root box.  `margin`: added to each half size as a fraction of it; `keep_aspect`: the
    rectangle is widened or heightened to out_hw's shape; `min_size`: a smaller rectangle gives no crop.  `coords_hw`: the
    space the boxes are in -- the network input for a plain decode, None (= `src_hw`) for a WindowMerger's result."""

    def __init__(self, frames: int, max_humans: int, src_hw, fmt: str, out_hw, max_crops: int = 16, mode: str = "people",
                 margin: float = 0.1, keep_aspect: bool = True, min_size: int = 8, coords_hw=None, K: int = cfg.K,
                 device=None):
        if fmt not in _ALIGN:
            raise ValueError(f"fmt must be one of {sorted(_ALIGN)}, not {fmt!r}")
        if mode not in _MODES:
            raise ValueError(f"mode must be one of {sorted(_MODES)}, not {mode!r}")
        if frames < 1 or max_crops < 1 or not 1 <= max_humans <= L.PPN_MATCH_MAX_PEOPLE:
            raise ValueError(f"{frames} frames x {max_humans} people x {max_crops} crops: at least one each, at most "
                             f"{L.PPN_MATCH_MAX_PEOPLE} people")
        if frames * max_crops > 65535:
            raise ValueError(f"{frames} frames x {max_crops} crops exceed 65535 images")
        if not 1 <= K <= L.PPN_MAX_KP:
            raise ValueError(f"K {K} outside 1..{L.PPN_MAX_KP}")
        self.src_hw = (int(src_hw[0]), int(src_hw[1]))
        self.out_hw = (int(out_hw[0]), int(out_hw[1]))
        self.coords_hw = self.src_hw if coords_hw is None else (int(coords_hw[0]), int(coords_hw[1]))
        ay, ax = _ALIGN[fmt]
        if min(self.src_hw) < 1 or min(self.out_hw) < 1 or min(self.coords_hw) < 1 or self.src_hw[0] % ay or self.src_hw[1] % ax:
            raise ValueError(f"a {fmt} picture of {self.src_hw}, crops of {self.out_hw}, boxes in {self.coords_hw}: sizes must be "
                             "at least 1 and the picture even where the format shares chroma")
        if not (math.isfinite(margin) and margin >= 0) or min_size < max(1, ay, ax):
            raise ValueError(f"margin {margin} must be finite and not negative, min_size {min_size} at least {max(1, ay, ax)}")
        self.frames, self.max_humans, self.max_crops, self.K, self.fmt = int(frames), int(max_humans), int(max_crops), K, fmt
        f32 = lambda v: np.float32(v)
        self.cfg = L.RoiCfg(K, self.max_humans, self.max_crops, self.src_hw[0], self.src_hw[1],
                            float(f32(self.src_hw[0]) / f32(self.coords_hw[0])), float(f32(self.src_hw[1]) / f32(self.coords_hw[1])),
                            _MODES[mode], float(margin), float(f32(self.out_hw[1]) / f32(self.out_hw[0])) if keep_aspect else 0.0,
                            ay, ax, int(min_size))
        dev = torch.device("cuda" if device is None else device)
        F_, R = self.frames, self.max_crops
        self.roi = torch.zeros(F_, R, 4, dtype=torch.int32, device=dev)
        self.status = torch.full((F_, R), EMPTY, dtype=torch.int32, device=dev)
        self.crops = torch.zeros(F_, R, self.out_hw[0], self.out_hw[1], 3, dtype=torch.uint8, device=dev)
        self.device = self.roi.device
        self.out = CropResult(self.crops, self.roi, self.status)

    def rois(self, result: D.DecodeResult) -> CropResult:
        """ppn_people_rois on the current stream: the rectangles and status of `result`'s people."""
        dev, K, M = self.device, self.K, self.max_humans
        if dev.type != "cuda":
            raise ValueError("PersonCropper runs on the device: its buffers live on " + str(dev))
        if result.max_humans != M:
            raise ValueError(f"result holds {result.max_humans} people per image, the cropper expects {M}")
        _dense("result.count", result.count, (self.frames,), torch.int32, dev)
        _dense("result.kp_cell", result.kp_cell, (self.frames, M, K), torch.int32, dev)
        _dense("result.bbox", result.bbox, (self.frames, M, K, 4), torch.float32, dev)
        L.check(L.load().ppn_people_rois(C.byref(self.cfg), result.count.data_ptr(), result.kp_cell.data_ptr(),
                                         result.bbox.data_ptr(), self.frames, self.roi.data_ptr(), self.status.data_ptr(),
                                         L.current_stream_ptr()), "ppn_people_rois")
        return self.out

    def crop(self, raw: torch.Tensor, flip: bool = False, matrix: str = "bt601", full_range: bool = False,
             pitch: Optional[int] = None) -> CropResult:
        """ppn_ingest_rois on the current stream: the rectangles ``rois`` wrote, cut out of `raw`."""
        if not (isinstance(raw, torch.Tensor) and raw.dim() >= 2 and raw.shape[0] == self.frames):
            raise ValueError(f"raw must hold {self.frames} frames")
        ingest_rois(raw, self.fmt, self.src_hw, self.roi, self.out_hw, self.crops, self.status, flip, matrix, full_range, pitch)
        return self.out

    def __call__(self, raw: torch.Tensor, result: D.DecodeResult, **kw) -> CropResult:
        self.rois(result)
        return self.crop(raw, **kw)
