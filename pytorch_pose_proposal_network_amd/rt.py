"""Mirror of the reference's realtime driver entry points (rt_test.py:52-147) over the HIP path.

    model, outsize, local_grid_size = network(resume="PPN_model_best.pth.tar", image_size=384)
    humans, scores = inference(image_u8_hwc, model, outsize, local_grid_size)

``inference`` keeps the reference's argument list; what it does differently is *where* things run: the
uint8 frame is uploaded once (442 KB), normalisation + the whole conv stack + head run as HIP kernels, the
head tensor never leaves the device (the reference copies all 17.5 MB of it to the host in seven slices,
rt_test.py:109-120) and only the compact people list (<= 80 KB) comes back.  Webcam capture and the matplotlib
animation (rt_test.py:150-205) are out of scope.  ``inference`` returns the reference's ``(humans, scores)`` instead of a
PIL image (pass ``draw=callable`` to post-process on the host); ``inference_drawn`` returns the drawn image as
rt_test.inference does and ``inference_batch_drawn`` the drawn batch, both painted on the device (render.py,
datatest.py:162-232).  ``inference_batch_tracked`` / ``inference_tracked`` add what the reference's loop lacks: ids that follow
a person from frame to frame (track.py), again without reading the people lists back.  ``inference_windows`` runs a big raw
frame as overlapping windows of the batch and joins the people in frame pixels on the device (windows.py);
``inference_windows_drawn`` paints them straight onto the raw frames (render.Renderer.draw_yuv);
``inference_batch_zones_drawn`` adds track ids, zones, counting lines and their counts to the picture (render.Overlay);
``inference_crops`` cuts
every detected person out of the raw frame as a fixed-size picture for a following model (crops.py).
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np
import torch

from . import config as cfg
from . import decode as D
from . import drn
from .model import PoseProposalNet


def network(resume: Optional[str] = None, image_size: int = 384, arch: str = "drn_d_22",
            compute_dtype: str = "float32", state_dict=None, latency: Optional[bool] = None):
    """rt_test.py:52-85: build D-22 PPN, derive ``outsize`` and load ``checkpoint['state_dict']``.

    The reference discovers ``outsize`` with a dummy forward (rt_test.py:65-68); the network is fully
    convolutional with total stride 16, so it is ``image_size // 16`` here.  ``latency=True``: low-latency plans for the
    reference's one-frame-at-a-time use (PoseProposalNet(latency=True); None: the PPN_LATENCY knob)."""
    local_grid_size = (21, 21)
    outsize = (image_size // 16, image_size // 16)
    model = PoseProposalNet(getattr(drn, arch)(), insize=(image_size, image_size), outsize=outsize,
                            local_grid_size=local_grid_size, compute_dtype=compute_dtype, latency=latency).cuda()
    if resume is not None:
        ckpt = torch.load(resume, map_location="cpu")
        state_dict = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
    if state_dict is not None:
        model.load_state_dict(state_dict)
    return model, outsize, local_grid_size


def ingest_frames(frames_bgr: torch.Tensor, size: int = 384, out: Optional[torch.Tensor] = None,
                  flip: bool = True, swap_rb: bool = True) -> torch.Tensor:
    """The cv2 calls of rt_test.py:150-157 on the device: u8 BGR camera frames [B,Hs,Ws,3] (CUDA) ->
    cv2.resize(dsize=(size,size)) -> flip both axes -> BGR2RGB -> u8 RGB [B,size,size,3].  `out` may be the model's
    own input buffer (``model.input_buffer(B, size, size, fused_decode=..., slot=...)``): forward_u8(out) then runs
    without any further copy."""
    from . import lib as L
    if not (frames_bgr.is_cuda and frames_bgr.dtype == torch.uint8 and frames_bgr.dim() == 4 and frames_bgr.shape[3] == 3):
        raise ValueError("ingest_frames expects a uint8 CUDA tensor [B,Hs,Ws,3]")
    x = frames_bgr.contiguous()
    b, hs, ws, _ = x.shape
    if out is None:
        out = torch.empty(b, size, size, 3, dtype=torch.uint8, device=x.device)
    if tuple(out.shape) != (b, size, size, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor {(b, size, size, 3)}")
    L.check(L.load().ppn_ingest_frames(x.data_ptr(), b, hs, ws, out.data_ptr(), size, size, int(flip), int(swap_rb),
                                       L.current_stream_ptr()), "ppn_ingest_frames")
    return out


def grab_frame(cap, size: int = 384, out: Optional[torch.Tensor] = None):
    """rt_test.py:150-157 with the resize / flips / colour conversion on the GPU: `cap` is anything with
    cv2.VideoCapture's ``read() -> (ret, frame_bgr_u8_hwc)``.  Returns ``(ret, frame)`` where frame is a u8 RGB
    [1,size,size,3] CUDA tensor (pass it to ``inference`` / ``model.forward_u8``)."""
    ret, frame = cap.read()
    if not ret or frame is None:
        return ret, None
    f = np.ascontiguousarray(np.asarray(frame))
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
        raise ValueError("cap.read() must deliver a uint8 HxWx3 BGR frame")
    return ret, ingest_frames(torch.from_numpy(f).unsqueeze(0).cuda(non_blocking=True), size, out)


_PIX_FORMATS = {"nv12": 0, "i420": 1, "yuyv": 2}        # lib.PPN_PIX_*
_YUV_MATRICES = {"bt601": 0, "bt709": 1}


def yuv_frame_layout(fmt: str, src_hw, pitch: Optional[int] = None):
    """Where the planes of one contiguous raw frame sit: ``(nbytes, pitch, pitch_c, u_offset, v_offset)`` (offsets in
    bytes from the frame's start, None for a plane the format lacks).  NV12: Y [h][pitch], then interleaved UV
    [h/2][pitch]; I420: Y [h][pitch], U and V [h/2][pitch/2]; YUYV: packed [h][pitch].  `pitch` defaults to tight."""
    if fmt not in _PIX_FORMATS:
        raise ValueError(f"fmt must be one of {sorted(_PIX_FORMATS)}, not {fmt!r}")
    h, w = int(src_hw[0]), int(src_hw[1])
    row = 2 * w if fmt == "yuyv" else w
    pitch = row if pitch is None else int(pitch)
    if h < 1 or w < 1 or w % 2 or (fmt != "yuyv" and h % 2):
        raise ValueError(f"{fmt} frames need an even width" + ("" if fmt == "yuyv" else " and height") + f", not {h}x{w}")
    if pitch < row:
        raise ValueError(f"pitch {pitch} is below the {row} bytes of a {fmt} row of width {w}")
    if fmt == "yuyv":
        return h * pitch, pitch, 0, None, None
    if fmt == "nv12":
        return h * pitch + (h // 2) * pitch, pitch, pitch, h * pitch, None
    if pitch % 2:
        raise ValueError("i420 needs an even pitch (the chroma pitch is pitch // 2)")
    pc = pitch // 2
    return h * pitch + 2 * (h // 2) * pc, pitch, pc, h * pitch, h * pitch + (h // 2) * pc


def _launch_ingest_yuv(raw: torch.Tensor, fmt: str, src_hw, out: torch.Tensor, flip: bool, matrix: str,
                       full_range: bool, pitch: Optional[int]):
    """ppn_ingest_yuv on the current stream: `raw` u8 [B,nbytes] on the device (rows of unit stride), `out` u8 [B,h,w,3]."""
    from . import lib as L
    if matrix not in _YUV_MATRICES:
        raise ValueError(f"matrix must be one of {sorted(_YUV_MATRICES)}, not {matrix!r}")
    nbytes, pitch, pitch_c, u_off, v_off = yuv_frame_layout(fmt, src_hw, pitch)
    if raw.shape[1] < nbytes:
        raise ValueError(f"a {fmt} frame of {tuple(src_hw)} with pitch {pitch} has {nbytes} bytes, raw rows have {raw.shape[1]}")
    base = raw.data_ptr()
    d = L.IngestDesc(format=_PIX_FORMATS[fmt], batch=raw.shape[0], src_h=int(src_hw[0]), src_w=int(src_hw[1]), pitch=pitch,
                     pitch_c=pitch_c, frame_stride=raw.stride(0) if raw.shape[0] > 1 else raw.shape[1], y=base,
                     u=None if u_off is None else base + u_off, v=None if v_off is None else base + v_off,
                     matrix=_YUV_MATRICES[matrix], full_range=int(bool(full_range)), dst=out.data_ptr(),
                     dst_h=out.shape[1], dst_w=out.shape[2], flip=int(bool(flip)), dst_bgr=0)
    L.check(L.load().ppn_ingest_yuv(d, L.current_stream_ptr()), "ppn_ingest_yuv")


def ingest_yuv(raw: torch.Tensor, fmt: str, src_hw, size=384, out: Optional[torch.Tensor] = None, flip: bool = False,
               matrix: str = "bt601", full_range: bool = False, pitch: Optional[int] = None) -> torch.Tensor:
    """Raw video frames -> u8 RGB [B,h,w,3] in one launch (ppn_ingest_yuv): colour conversion (OpenCV's fixed-point
    YUV -> RGB, `matrix` "bt601" / "bt709", limited or full range), the resize of ``ingest_frames`` and the optional flip
    of both axes, without a full-resolution RGB copy.  `raw`: u8 CUDA tensor [B, nbytes], one contiguous frame per row
    with the planes laid out as ``yuv_frame_layout(fmt, src_hw, pitch)`` says (`fmt` "nv12", "i420" or "yuyv"; `pitch`
    bytes per luma row, tight by default; rows may be longer than a frame).  `size`: an int or (h, w).  `out` may be
    ``model.input_buffer(...)`` exactly as for ``ingest_frames``."""
    if not (isinstance(raw, torch.Tensor) and raw.is_cuda and raw.dtype == torch.uint8 and raw.dim() == 2):
        raise ValueError("ingest_yuv expects a uint8 CUDA tensor [B, nbytes]")
    if raw.stride(1) != 1:
        raw = raw.contiguous()
    h, w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    b = raw.shape[0]
    if out is None:
        out = torch.empty(b, h, w, 3, dtype=torch.uint8, device=raw.device)
    if tuple(out.shape) != (b, h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor {(b, h, w, 3)}")
    _launch_ingest_yuv(raw, fmt, src_hw, out, flip, matrix, full_range, pitch)
    return out


def grab_frame_raw(cap, fmt: str, src_hw, size=384, out: Optional[torch.Tensor] = None, flip: bool = True,
                   matrix: str = "bt601", full_range: bool = False, pitch: Optional[int] = None):
    """``grab_frame`` for a capture that hands out raw frames (cv2 with CAP_PROP_CONVERT_RGB = 0, a pipe reader):
    ``cap.read() -> (ret, u8 array of the frame's bytes, any shape)`` -- cv2 gives [H,W,2] for YUYV and [H*3/2,W] for
    NV12 / I420.  Returns ``(ret, frame)``, frame a u8 RGB [1,h,w,3] CUDA tensor; `flip` defaults to grab_frame's."""
    ret, frame = cap.read()
    if not ret or frame is None:
        return ret, None
    f = np.ascontiguousarray(np.asarray(frame))
    if f.dtype != np.uint8:
        raise ValueError("cap.read() must deliver the raw frame as uint8")
    raw = torch.from_numpy(f.reshape(1, -1)).cuda(non_blocking=True)
    return ret, ingest_yuv(raw, fmt, src_hw, size, out, flip, matrix, full_range, pitch)


def _decode_flip_averaged(frames: torch.Tensor, model: PoseProposalNet, decoder: Optional[D.Decoder],
                          detection_thresh: float, merger=None) -> D.DecodeResult:
    """Horizontal-flip test-time averaging (tta.py): [frames | frames mirrored] staged straight into the plan's input of
    batch 2B, one forward with a materialised head pair, ppn_tta_merge, Decoder.decode_fused."""
    from .tta import FlipMerger
    frames = frames.contiguous()
    b, h, w, _ = frames.shape
    if merger is None:
        merger = FlipMerger(b, (h // 16, w // 16), model.local_grid_size, frames.device)
    pair = merger.stage(frames, out=model.input_buffer(2 * b, h, w))
    unary, keys = merger.merge(model.forward_u8(pair, fused_decode=False))
    if decoder is None:
        decoder = D.Decoder(b, (h // 16, w // 16), (h, w), model.local_grid_size, detection_thresh, device=frames.device)
    return decoder.decode_fused(unary, keys)


def inference(image, model: PoseProposalNet, outsize, local_grid_size, detection_thresh: float = 0.15,
              draw: Optional[Callable] = None, flip_tta: bool = False):
    """rt_test.py:87-147 for one RGB frame (u8 [S,S,3] array / PIL image / tensor).

    Returns ``(humans, scores)`` exactly as datatest.get_humans_by_feature does (lists of dicts
    keypoint -> [ymin,xmin,ymax,xmax] / keypoint -> delta), or ``draw(image, humans, scores)`` if given.
    ``flip_tta=True``: the people of the head averaged with the mirrored frame's head (tta.py)."""
    model.eval()
    if isinstance(image, torch.Tensor) and image.is_cuda:             # what grab_frame() returns: already on the device
        frames = image if image.dim() == 4 else image.unsqueeze(0)
        if frames.dtype != torch.uint8 or frames.shape[0] != 1 or frames.shape[3] != 3:
            raise ValueError("inference expects a uint8 [1,H,W,3] / [H,W,3] RGB frame")
        hw = (frames.shape[1], frames.shape[2])
    else:
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("inference expects a uint8 HxWx3 RGB frame")
        frames = torch.from_numpy(np.ascontiguousarray(img)).unsqueeze(0).cuda(non_blocking=True)
        hw = (img.shape[0], img.shape[1])
    outW, outH = outsize
    if flip_tta:
        res = _decode_flip_averaged(frames, model, None, detection_thresh)
    else:
        head = model.forward_u8(frames)
        res = D.decode_heads(head, insize_hw=hw, local_grid=local_grid_size,
                             detection_thresh=detection_thresh)
    humans, scores = res.to_humans()[0]
    if draw is not None:
        return draw(image, humans, scores)
    return humans, scores


def inference_batch(frames_u8: torch.Tensor, model: PoseProposalNet, decoder: Optional[D.Decoder] = None,
                    detection_thresh: float = 0.15, flip_tta: bool = False, merger=None) -> D.DecodeResult:
    """Batched device-side inference: u8 [B,S,S,3] CUDA tensor -> compact people lists on the device.
    ``flip_tta=True``: flip-averaged heads (two forwards per image in one doubled batch; pass a Decoder and a
    tta.FlipMerger as ``merger`` to allocate nothing per call)."""
    if flip_tta:
        return _decode_flip_averaged(frames_u8, model, decoder, detection_thresh, merger)
    unary, keys = model.forward_u8(frames_u8, fused_decode=True)     # the head tensor is never materialised
    if decoder is None:
        b, _, h, w = unary.shape
        decoder = D.Decoder(b, (h, w), (frames_u8.shape[1], frames_u8.shape[2]), model.local_grid_size,
                            detection_thresh, device=unary.device)
    return decoder.decode_fused(unary, keys)


def inference_drawn(image, model: PoseProposalNet, outsize, local_grid_size, detection_thresh: float = 0.15,
                    visbbox: bool = False, gridOn: bool = False, flip_tta: bool = False):
    """rt_test.py:87-147 including its last step (rt_test.py:135-147): the frame with the detected people drawn on it by
    the HIP rasteriser (render.py), as a PIL image -- a u8 [H,W,3] array where PIL is absent.  The people lists never
    leave the device; one frame goes up and one comes back."""
    from . import render as R
    model.eval()
    if isinstance(image, torch.Tensor) and image.is_cuda:
        frames = image if image.dim() == 4 else image.unsqueeze(0)
        if frames.dtype != torch.uint8 or frames.shape[0] != 1 or frames.shape[3] != 3:
            raise ValueError("inference_drawn expects a uint8 [1,H,W,3] / [H,W,3] RGB frame")
        frames = frames.contiguous()
    else:
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("inference_drawn expects a uint8 HxWx3 RGB frame")
        frames = torch.from_numpy(np.ascontiguousarray(img)).unsqueeze(0).cuda(non_blocking=True)
    if flip_tta:
        res = _decode_flip_averaged(frames, model, None, detection_thresh)
    else:
        head = model.forward_u8(frames)
        res = D.decode_heads(head, insize_hw=(frames.shape[1], frames.shape[2]), local_grid=local_grid_size,
                             detection_thresh=detection_thresh)
    drawn = R.draw_people(frames, res, visbbox=visbbox, gridOn=gridOn, outsize=outsize)[0].cpu().numpy()
    try:
        from PIL import Image
    except ImportError:
        return drawn
    return Image.fromarray(drawn)


def inference_batch_drawn(frames_u8: torch.Tensor, model: PoseProposalNet, decoder: Optional[D.Decoder] = None,
                          renderer=None, out: Optional[torch.Tensor] = None, detection_thresh: float = 0.15,
                          visbbox: bool = False, gridOn: bool = False, flip_tta: bool = False, merger=None):
    """inference_batch plus the drawing, all on the device: u8 [B,S,S,3] CUDA frames -> (DecodeResult, drawn u8 frames).
    `out` as in render.Renderer (None: a new tensor, `frames_u8` itself: in place); pass a Decoder and a render.Renderer to
    allocate nothing per call."""
    from . import render as R
    res = inference_batch(frames_u8, model, decoder, detection_thresh, flip_tta, merger)
    if renderer is None:
        renderer = R.Renderer(frames_u8.shape[0], res.max_humans, frames_u8.device)
    outW = frames_u8.shape[2] // 16
    return res, renderer(frames_u8, res, visbbox=visbbox, gridOn=gridOn, out=out, outsize=(outW, frames_u8.shape[1] // 16))


def inference_batch_tracked(frames_u8: torch.Tensor, model: PoseProposalNet, tracker, decoder: Optional[D.Decoder] = None,
                            detection_thresh: float = 0.15, flip_tta: bool = False, merger=None):
    """inference_batch plus the tracking, all on the device: u8 [B,S,S,3] CUDA frames with B = tracker.streams *
    tracker.frames (image s * frames + t is frame t of stream s) -> (DecodeResult, track.TrackResult).  `tracker` is a
    track.Tracker whose max_humans is the decoder's; it carries the tracks from call to call.  Nothing is read back."""
    res = inference_batch(frames_u8, model, decoder, detection_thresh, flip_tta, merger)
    return res, tracker.update(res)


def inference_batch_clips(frames_u8: torch.Tensor, model: PoseProposalNet, tracker, clips, decoder: Optional[D.Decoder] = None,
                          detection_thresh: float = 0.15, flip_tta: bool = False, merger=None, gather: bool = True):
    """inference_batch_tracked plus the skeleton clips, all on the device: -> (DecodeResult, track.TrackResult,
    clips.ClipRows, clips.ClipBatch or None).  `clips` is a clips.PoseClips of the tracker's streams, frames and max_humans
    (give it max_gap = the tracker's max_age and reset the two together: then every live track has its clip); it takes the
    tracker's smoothed centres.  ``gather=False`` only pushes the frames -- gather when the action model is due.  Nothing is
    read back."""
    res, tracks = inference_batch_tracked(frames_u8, model, tracker, decoder, detection_thresh, flip_tta, merger)
    rows = clips.push(res, tracks)
    return res, tracks, rows, clips.gather() if gather else None


def inference_batch_actions(frames_u8: torch.Tensor, model: PoseProposalNet, tracker, clips, actions,
                            decoder: Optional[D.Decoder] = None, detection_thresh: float = 0.15, flip_tta: bool = False,
                            merger=None):
    """inference_batch_clips plus the action model, all on the device: -> (DecodeResult, track.TrackResult, clips.ClipRows,
    clips.ClipBatch, actions.ActionResult).  `actions` is an actions.ActionModel of the clips' streams, length and K; it
    classifies every live clip that holds at least its ``min_len`` frames, the others get label -1.  Nothing is read back
    (``ActionResult.to_host()`` is the one read-back, when the labels are wanted on the host)."""
    if (actions.streams, actions.length, actions.spec.K) != (clips.streams, clips.length, clips.K):
        raise ValueError(f"the ActionModel takes {actions.streams} streams of clips [3, {actions.length}, {actions.spec.K}], "
                         f"the PoseClips hand out {clips.streams} of [3, {clips.length}, {clips.K}]")
    res, tracks, rows, batch = inference_batch_clips(frames_u8, model, tracker, clips, decoder, detection_thresh, flip_tta,
                                                     merger)
    return res, tracks, rows, batch, actions(batch)


def inference_batch_zones(frames_u8: torch.Tensor, model: PoseProposalNet, tracker, zones, decoder: Optional[D.Decoder] = None,
                          detection_thresh: float = 0.15, flip_tta: bool = False, merger=None):
    """inference_batch_tracked plus the zones and counting lines, all on the device: -> (DecodeResult, track.TrackResult,
    zones.ZoneResult).  `zones` is a zones.Zones of the tracker's streams, frames and max_humans (give it max_gap = the
    tracker's max_age and reset the two together: then its slots are the live tracks); its geometry is in the network's
    input pixels here, and it takes the tracker's smoothed centres.  For big frames, Zones.update takes the results of
    inference_windows plus Tracker.update as they are: then the geometry is in frame pixels.  Nothing is read back."""
    res, tracks = inference_batch_tracked(frames_u8, model, tracker, decoder, detection_thresh, flip_tta, merger)
    return res, tracks, zones.update(res, tracks)


def inference_batch_zones_drawn(frames_u8: torch.Tensor, model: PoseProposalNet, tracker, zones, overlay=None, renderer=None,
                                out: Optional[torch.Tensor] = None, decoder: Optional[D.Decoder] = None,
                                detection_thresh: float = 0.15, visbbox: bool = False, gridOn: bool = False,
                                flip_tta: bool = False, merger=None):
    """inference_batch_zones plus the monitoring picture, all on the device: -> (DecodeResult, track.TrackResult,
    zones.ZoneResult, drawn u8 frames).  The people, their track ids, the zones and lines with this frame's occupancy,
    crossings and running totals are painted onto the frames by ``render.Renderer`` with `overlay` (a render.Overlay whose
    `frames` is the tracker's; None: ``render.Overlay(frames=tracker.frames)``).  `out` as in render.Renderer (None: a new
    tensor, `frames_u8` itself: in place); pass a Decoder and a render.Renderer to allocate nothing per call.  Nothing is
    read back."""
    from . import render as R
    res, tracks, zr = inference_batch_zones(frames_u8, model, tracker, zones, decoder, detection_thresh, flip_tta, merger)
    if overlay is None:
        overlay = R.Overlay(frames=tracker.frames)
    if renderer is None:
        renderer = R.Renderer(frames_u8.shape[0], res.max_humans, frames_u8.device)
    outW = frames_u8.shape[2] // 16
    drawn = renderer(frames_u8, res, visbbox=visbbox, gridOn=gridOn, out=out, outsize=(outW, frames_u8.shape[1] // 16),
                     overlay=overlay, tracks=tracks, zones=zones, zone_result=zr)
    return res, tracks, zr, drawn


def inference_windows(raw: torch.Tensor, fmt: str, src_hw, model: PoseProposalNet, layout, decoder: Optional[D.Decoder] = None,
                      merger=None, detection_thresh: float = 0.15, size=384, flip: bool = False, matrix: str = "bt601",
                      full_range: bool = False, pitch: Optional[int] = None, merge_thr: float = 0.3,
                      fuse: bool = True) -> D.DecodeResult:
    """Windowed inference (windows.py): the F raw frames `raw` (as ``windows.ingest_windows`` takes them; `fmt` "nv12",
    "i420", "yuyv" or "bgr") are cut into the n windows of `layout` (a windows.WindowLayout of `src_hw`), ingested straight
    into the plan's input buffer of batch F * n, run through the forward with fused decode, and the people of the windows
    are joined on the device.  Returns the merged DecodeResult of F images in FRAME pixels (``kp_cell`` = the source person
    of a keypoint, -1: absent); ``Tracker.update``, ``draw_people``, ``draw_people_yuv`` and ``to_humans()`` take it as it is.  Pass a Decoder
    of batch F * n and a windows.WindowMerger to allocate nothing per call.  Nothing is read back.
    ``flip=True`` (as ``ingest_yuv``: every image turned by 180 degrees) gives the people of the TURNED frame: each window
    image is turned on its own, so window i lies at ``layout.flipped()``'s place in the turned frame and the merge runs
    with that layout -- a `merger` passed in must then have been built on ``layout.flipped()``, and on `layout` otherwise."""
    from . import windows as W
    if tuple(int(v) for v in src_hw) != layout.src_hw:
        raise ValueError(f"the layout cuts a {layout.src_hw} picture, the frames are {tuple(src_hw)}")
    placed = layout.flipped() if flip else layout                    # where the window images lie in the frame the people are in
    if merger is not None and (merger.layout.src_hw != placed.src_hw or merger.layout.windows != placed.windows):
        raise ValueError("the merger's layout is not " + ("layout.flipped(), which flip=True needs" if flip else "the layout"))
    h, w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    frames = raw.shape[0]
    buf = model.input_buffer(frames * layout.n, h, w, True, True)
    W.ingest_windows(raw, fmt, layout, (h, w), buf, flip, matrix, full_range, pitch)
    unary, keys = model.forward_u8(buf, fused_decode=True)
    if decoder is None:
        decoder = D.Decoder(frames * layout.n, (unary.shape[2], unary.shape[3]), (h, w), model.local_grid_size,
                            detection_thresh, device=unary.device)
    res = decoder.decode_fused(unary, keys)
    if merger is None:
        merger = W.WindowMerger(placed, frames, (h, w), res.max_humans, merge_thr=merge_thr, fuse=fuse, device=unary.device)
    return merger(res)


def inference_windows_drawn(raw: torch.Tensor, fmt: str, src_hw, model: PoseProposalNet, layout, decoder: Optional[D.Decoder] = None,
                            merger=None, detection_thresh: float = 0.15, size=384, flip: bool = False, matrix: str = "bt601",
                            full_range: bool = False, pitch: Optional[int] = None, merge_thr: float = 0.3, fuse: bool = True,
                            renderer=None, out: Optional[torch.Tensor] = None, visbbox: bool = False, overlay=None,
                            tracker=None, zones=None):
    """inference_windows plus the drawing, all on the device: the merged people painted straight onto the raw frames they
    were found in (``render.Renderer.draw_yuv``: NV12 / I420 / YUYV surfaces without an RGB intermediate, `matrix` and
    `full_range` naming the surface's colours as they do for the ingest; "bgr" through the RGB rasteriser) ->
    (DecodeResult, drawn raw frames).  `out` as in draw_yuv (None: a new tensor, `raw` itself: in place); pass a Decoder, a
    windows.WindowMerger and a render.Renderer of (F, merged max_humans) to allocate nothing per call.  Nothing is read back.
    ``flip=True`` raises ValueError: the people of a turned frame do not lie on the unturned surface.
    With `overlay` (a render.Overlay) the monitoring picture is painted too and the return value is (DecodeResult, drawn,
    TrackResult or None, ZoneResult or None): `tracker` (a track.Tracker) is updated with the merged people and labels them
    with their ids, `zones` (a zones.Zones, which needs the tracker; its geometry in FRAME pixels) is updated and drawn."""
    from . import render as R
    if flip:
        raise ValueError("inference_windows_drawn: flip=True gives the people of the turned frame, which do not lie on `raw`")
    if overlay is None and (tracker is not None or zones is not None):
        raise ValueError("inference_windows_drawn: tracker and zones are drawn by an overlay: pass overlay=render.Overlay(...)")
    if zones is not None and tracker is None:
        raise ValueError("inference_windows_drawn: zones count tracked people: pass the tracker too")
    res = inference_windows(raw, fmt, src_hw, model, layout, decoder, merger, detection_thresh, size, False, matrix,
                            full_range, pitch, merge_thr, fuse)
    if renderer is None:
        renderer = R.Renderer(raw.shape[0], res.max_humans, raw.device)
    if overlay is None:
        return res, renderer.draw_yuv(raw, fmt, src_hw, res, visbbox=visbbox, out=out, pitch=pitch, matrix=matrix,
                                      full_range=full_range)
    tracks = tracker.update(res) if tracker is not None else None
    zr = zones.update(res, tracks) if zones is not None else None
    drawn = renderer.draw_yuv(raw, fmt, src_hw, res, visbbox=visbbox, out=out, pitch=pitch, matrix=matrix,
                              full_range=full_range, overlay=overlay, tracks=tracks, zones=zones, zone_result=zr)
    return res, drawn, tracks, zr


def inference_crops(raw: torch.Tensor, fmt: str, src_hw, model: PoseProposalNet, cropper, layout=None, tracker=None,
                    decoder: Optional[D.Decoder] = None, merger=None, detection_thresh: float = 0.15, size=384,
                    matrix: str = "bt601", full_range: bool = False, pitch: Optional[int] = None, merge_thr: float = 0.3,
                    fuse: bool = True):
    """Detect the people of F raw frames and cut each of them out of the raw frame for a following model (crops.py), all on
    the device: ingest -> forward -> fused decode (-> window merge when `layout`, a windows.WindowLayout of `src_hw`, is
    given: ``inference_windows``) (-> `tracker`.update when given) -> rectangles -> crops.  `cropper` is a
    crops.PersonCropper of F frames on `src_hw` / `fmt` whose ``coords_hw`` is the space the people come out in: the frame
    with a layout, the network input (`size`) without.  Returns ``(DecodeResult, CropResult)``, with a tracker
    ``(DecodeResult, CropResult, TrackResult)``: crop r, bbox r and ids r of a frame are the same person.  Pass a Decoder
    (and a WindowMerger) to allocate nothing per call.  Nothing is read back."""
    from . import windows as W
    H, Wd = int(src_hw[0]), int(src_hw[1])
    h, w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    space = (H, Wd) if layout is not None else (h, w)
    if cropper.src_hw != (H, Wd) or cropper.fmt != fmt or cropper.coords_hw != space or cropper.frames != raw.shape[0]:
        raise ValueError(f"the cropper cuts {cropper.frames} {cropper.fmt} frames of {cropper.src_hw} with boxes in "
                         f"{cropper.coords_hw}; the call has {raw.shape[0]} {fmt} frames of {(H, Wd)} and people in {space}")
    if layout is not None:
        res = inference_windows(raw, fmt, src_hw, model, layout, decoder, merger, detection_thresh, size, False, matrix,
                                full_range, pitch, merge_thr, fuse)
    else:
        frames = raw.shape[0]
        buf = model.input_buffer(frames, h, w, True, True)
        W.ingest_windows(raw, fmt, W.WindowLayout((H, Wd), [(0, 0, H, Wd)]), (h, w), buf, False, matrix, full_range, pitch)
        unary, keys = model.forward_u8(buf, fused_decode=True)
        if decoder is None:
            decoder = D.Decoder(frames, (unary.shape[2], unary.shape[3]), (h, w), model.local_grid_size, detection_thresh,
                                device=unary.device)
        res = decoder.decode_fused(unary, keys)
    tracks = tracker.update(res) if tracker is not None else None
    out = cropper(raw, res, matrix=matrix, full_range=full_range, pitch=pitch)
    return (res, out) if tracker is None else (res, out, tracks)


def inference_redacted(raw: torch.Tensor, fmt: str, src_hw, model: PoseProposalNet, redactor, layout=None, tracker=None,
                       decoder: Optional[D.Decoder] = None, merger=None, detection_thresh: float = 0.15, size=384,
                       flip: bool = False, pitch: Optional[int] = None, merge_thr: float = 0.3, fuse: bool = True,
                       out: Optional[torch.Tensor] = None):
    """Detect the people of raw frames and redact them in those frames (redact.py), all on the device: ingest -> forward ->
    fused decode (-> window merge when `layout`, a windows.WindowLayout of `src_hw`, is given: ``inference_windows``)
    (-> `tracker`.update when given) -> cells -> apply.  `redactor` is a redact.Redactor of streams x frames = F images on
    `src_hw` / `fmt` whose ``coords_hw`` is the space the people come out in: the frame with a layout, the network input
    (`size`) without; it names the surface's matrix and range, which the ingest uses too, and carries the hold state from
    call to call.  `raw` must suit both ``windows.ingest_windows`` and ``Redactor.apply`` (packed BGR: [F, H, W, 3]); `out`
    as in ``Redactor.apply`` (None: a new tensor, `raw` itself: in place).  Returns ``(DecodeResult, redacted frames)``,
    with a tracker ``(DecodeResult, redacted frames, TrackResult)``.  Nothing is read back.  ``flip=True`` raises
    ValueError: the people of a turned frame do not lie on the unturned surface."""
    from . import windows as W
    if flip:
        raise ValueError("inference_redacted: flip=True gives the people of the turned frame, which do not lie on `raw`")
    H, Wd = int(src_hw[0]), int(src_hw[1])
    h, w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    space = (H, Wd) if layout is not None else (h, w)
    if redactor.src_hw != (H, Wd) or redactor.fmt != fmt or redactor.coords_hw != space or redactor.batch != raw.shape[0]:
        raise ValueError(f"the redactor takes {redactor.batch} {redactor.fmt} frames of {redactor.src_hw} with boxes in "
                         f"{redactor.coords_hw}; the call has {raw.shape[0]} {fmt} frames of {(H, Wd)} and people in {space}")
    matrix, full_range = redactor.matrix, redactor.full_range
    if layout is not None:
        res = inference_windows(raw, fmt, src_hw, model, layout, decoder, merger, detection_thresh, size, False, matrix,
                                full_range, pitch, merge_thr, fuse)
    else:
        frames = raw.shape[0]
        buf = model.input_buffer(frames, h, w, True, True)
        W.ingest_windows(raw, fmt, W.WindowLayout((H, Wd), [(0, 0, H, Wd)]), (h, w), buf, False, matrix, full_range, pitch)
        unary, keys = model.forward_u8(buf, fused_decode=True)
        if decoder is None:
            decoder = D.Decoder(frames, (unary.shape[2], unary.shape[3]), (h, w), model.local_grid_size, detection_thresh,
                                device=unary.device)
        res = decoder.decode_fused(unary, keys)
    tracks = tracker.update(res) if tracker is not None else None
    done = redactor(raw, res, out, pitch)
    return (res, done) if tracker is None else (res, done, tracks)


def inference_reid(raw: torch.Tensor, fmt: str, src_hw, model: PoseProposalNet, tracker, reid, layout=None,
                   decoder: Optional[D.Decoder] = None, merger=None, detection_thresh: float = 0.15, size=384,
                   flip: bool = False, pitch: Optional[int] = None, merge_thr: float = 0.3, fuse: bool = True):
    """Detect and track the people of raw frames and give them persistent ids by appearance (reid.py), all on the device:
    ingest -> forward -> fused decode (-> window merge when `layout`, a windows.WindowLayout of `src_hw`, is given:
    ``inference_windows``) -> `tracker`.update -> rectangles -> descriptors from `raw` -> gallery.  `reid` is a reid.ReId of
    streams x frames = F images on `src_hw` / `fmt` whose ``coords_hw`` is the space the people come out in: the frame with
    a layout, the network input (`size`) without; it names the surface's matrix and range, which the ingest uses too, and
    carries the gallery from call to call.  Returns ``(DecodeResult, TrackResult, ReIdResult)``; pass a Decoder (and a
    WindowMerger) to allocate nothing per call.  Nothing is read back.  ``flip=True`` raises ValueError: the people of a
    turned frame do not lie on the unturned surface."""
    from . import windows as W
    if flip:
        raise ValueError("inference_reid: flip=True gives the people of the turned frame, which do not lie on `raw`")
    H, Wd = int(src_hw[0]), int(src_hw[1])
    h, w = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    space = (H, Wd) if layout is not None else (h, w)
    if reid.src_hw != (H, Wd) or reid.fmt != fmt or reid.coords_hw != space or reid.batch != raw.shape[0]:
        raise ValueError(f"the ReId takes {reid.batch} {reid.fmt} frames of {reid.src_hw} with boxes in {reid.coords_hw}; "
                         f"the call has {raw.shape[0]} {fmt} frames of {(H, Wd)} and people in {space}")
    matrix, full_range = reid.matrix, reid.full_range
    if layout is not None:
        res = inference_windows(raw, fmt, src_hw, model, layout, decoder, merger, detection_thresh, size, False, matrix,
                                full_range, pitch, merge_thr, fuse)
    else:
        frames = raw.shape[0]
        buf = model.input_buffer(frames, h, w, True, True)
        W.ingest_windows(raw, fmt, W.WindowLayout((H, Wd), [(0, 0, H, Wd)]), (h, w), buf, False, matrix, full_range, pitch)
        unary, keys = model.forward_u8(buf, fused_decode=True)
        if decoder is None:
            decoder = D.Decoder(frames, (unary.shape[2], unary.shape[3]), (h, w), model.local_grid_size, detection_thresh,
                                device=unary.device)
        res = decoder.decode_fused(unary, keys)
    tracks = tracker.update(res)
    return res, tracks, reid.reid(raw, res, tracks, pitch=pitch)


def inference_tracked(image, model: PoseProposalNet, outsize, local_grid_size, tracker, detection_thresh: float = 0.15,
                      flip_tta: bool = False):
    """``inference`` for the frames of one video: returns ``(humans, scores, ids)`` -- the reference-style lists of
    ``inference`` and, per human, its track id (-1: untracked).  `tracker`: a track.Tracker(streams=1, frames=1,
    max_humans=outsize[0] * outsize[1]) kept by the caller from frame to frame.  The humans' boxes are the frame's own;
    the smoothed centres are ``tracker.xy[0]``."""
    model.eval()
    if isinstance(image, torch.Tensor) and image.is_cuda:
        frames = image if image.dim() == 4 else image.unsqueeze(0)
        if frames.dtype != torch.uint8 or frames.shape[0] != 1 or frames.shape[3] != 3:
            raise ValueError("inference_tracked expects a uint8 [1,H,W,3] / [H,W,3] RGB frame")
    else:
        img = np.asarray(image)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("inference_tracked expects a uint8 HxWx3 RGB frame")
        frames = torch.from_numpy(np.ascontiguousarray(img)).unsqueeze(0).cuda(non_blocking=True)
    if flip_tta:
        res = _decode_flip_averaged(frames, model, None, detection_thresh)
    else:
        res = D.decode_heads(model.forward_u8(frames), insize_hw=(frames.shape[1], frames.shape[2]),
                             local_grid=local_grid_size, detection_thresh=detection_thresh)
    tracks = tracker.update(res, want_xy=True)
    humans, scores = res.to_humans()[0]
    ids = tracks.ids[0, :len(humans)].cpu().numpy().tolist()
    return humans, scores, ids


class InferencePipeline:
    """Two-deep software pipeline for batched serving: the conv stack of batch i+1 runs on the caller's stream
    while the latency-bound NMS + limb-parse kernel of batch i (one workgroup per image, 32 of 256 CUs) runs on a
    side stream.  Each in-flight batch owns its plan outputs and its Decoder (slot 0 / 1); HIP events order the
    hand-over in both directions, nothing blocks the host.

        pipe = InferencePipeline(model, batch, (S, S))
        for frames in source:                       # u8 [B,S,S,3] on the device
            done = pipe.submit(frames)              # DecodeResult of THIS batch, valid once done.ready is reached
        pipe.flush()                                # or torch.cuda.synchronize()

    `submit` returns the DecodeResult object of the batch just submitted; call `result.ready.synchronize()` (or
    make a stream wait on it) before reading it.  A slot is reused two submits later."""

    def __init__(self, model: PoseProposalNet, batch: int, insize_hw, detection_thresh: float = 0.15, device=None):
        self.model = model
        dev = device if device is not None else model.device
        h, w = insize_hw[0] // 16, insize_hw[1] // 16
        self.decoders = [D.Decoder(batch, (h, w), insize_hw, model.local_grid_size, detection_thresh, device=dev)
                         for _ in range(2)]
        self.side = torch.cuda.Stream(device=dev)                  # (a high-priority stream measured no better)
        self.fwd_done = [torch.cuda.Event() for _ in range(2)]
        self.dec_done = [None, None]
        self.k = 0

    def submit(self, frames_u8: torch.Tensor) -> D.DecodeResult:
        k = self.k
        self.k ^= 1
        main = torch.cuda.current_stream(frames_u8.device)
        if self.dec_done[k] is not None:
            main.wait_event(self.dec_done[k])                  # slot k's previous outputs have been consumed
        unary, keys = self.model.forward_u8(frames_u8, fused_decode=True, slot=k)
        self.fwd_done[k].record(main)
        with torch.cuda.stream(self.side):
            self.side.wait_event(self.fwd_done[k])
            res = self.decoders[k].decode_fused(unary, keys)
            ev = torch.cuda.Event()
            ev.record(self.side)
        self.dec_done[k] = ev
        res.ready = ev
        return res

    def flush(self):
        self.side.synchronize()


_LANE_STREAMS: dict = {}


def _lane_streams(dev, lanes: int):
    """The lane streams of a device, created once per process and shared by every MultiLaneInference on it.  The runtime maps
    streams onto a handful of hardware queues (four by default); a pipeline whose lanes get fresh streams late in a process can
    find two of them on ONE queue, i.e. serialised: bench.py's `tile_policy_1` section, the third pipeline of its process, ran its
    two lanes at the one-lane rate (9.5 k instead of 11.6 k images/s, round 5).  Pipelines on the same device therefore reuse the
    first `lanes` streams of one pool (correct for any use -- a stream orders its work -- and what a server wants anyway)."""
    key = torch.device(dev)
    if key.index is None:
        key = torch.device(key.type, torch.cuda.current_device())
    pool = _LANE_STREAMS.setdefault(key, [])
    while len(pool) < lanes:
        pool.append(torch.cuda.Stream(device=key))
    return pool[:lanes]


class MultiLaneInference:
    """Independent inference lanes on separate HIP streams, batches go round-robin: while one lane is in a
    launch that cannot fill the GPU (the 14-22 us neck convolutions, the last partial round of workgroups of a
    layer, the one-workgroup-per-image parse kernel, the gap between two dependent launches) the other lane's
    workgroups take the idle CUs.  Each lane owns its plan outputs (slot) and Decoder; the input hand-over and the
    result hand-over are HIP events.  Results are bit-identical to the serial path."""

    def __init__(self, model: PoseProposalNet, batch: int, insize_hw, detection_thresh: float = 0.15, device=None,
                 lanes: int = 2, tile_policy: int = 0, shared_plan: Optional[bool] = None):
        self.model = model
        dev = device if device is not None else model.device
        h, w = insize_hw[0] // 16, insize_hw[1] // 16
        self.decoders = [D.Decoder(batch, (h, w), insize_hw, model.local_grid_size, detection_thresh, device=dev)
                         for _ in range(lanes)]
        self.streams = _lane_streams(dev, lanes)
        self._stages = [None] * lanes                     # pinned read-back buffers, created on first use
        self._raw = [None] * lanes                        # device staging of raw video frames (submit_raw), likewise
        self.insize_hw = (int(insize_hw[0]), int(insize_hw[1]))
        self.k = 0
        # tile_policy 1: conv tiles chosen by efficiency alone instead of whole rounds of workgroups (process-wide
        # setting of libppn, restored by close()); measured +4 % with two lanes, but the per-launch (one in flight)
        # durations of those tiles are worse, so the default keeps the single-stream choice
        from . import lib as L
        self._policy = tile_policy
        L.check(L.load().ppn_set_conv_tile_policy(tile_policy), "ppn_set_conv_tile_policy")
        # csrc/conv64.hip (64 -> 64 3x3 with the filter bank in registers) shortens layer3's launches by ~7 us each when
        # one launch is in flight, but its workgroups own a CU's whole LDS and register file, so another lane's kernels
        # cannot share the CU: with several lanes the generic kernel gives the higher throughput (same-box A/B: 11.04 k
        # vs 10.96 k images/s with three lanes).  The choice travels in THIS pipeline's plans (ppn_conv_desc.flags), so
        # other plans, trainers and pipelines of the process -- and a user's PPN_CONV64 setting -- are untouched;
        # results are bit-identical either way.
        # shared_plan=True with ONE lane: the multi-lane plan (same kernels, same tiles) with one launch in flight -- what a
        # profiler run needs so that its per-kernel durations describe the kernels the multi-lane headline ran
        shared = lanes > 1 if shared_plan is None else bool(shared_plan)
        self._conv_flags = (L.PPN_CONV_NO_FILTER_BANK | L.PPN_CONV_SHARED_GPU) if shared else 0
        import os
        if shared and os.environ.get("PPN_LANES_LONE_TILES") == "1":      # A/B knob: keep the tiles that shorten a lone launch
            self._conv_flags = L.PPN_CONV_NO_FILTER_BANK

    def close(self):
        from . import lib as L
        self.flush()
        L.check(L.load().ppn_set_conv_tile_policy(0), "ppn_set_conv_tile_policy")

    def submit(self, frames_u8: torch.Tensor, to_host: bool = False) -> D.DecodeResult:
        """Queue one batch on the next lane.  `frames_u8`: u8 [B,S,S,3] on the device, or in PINNED host memory -- then
        the H2D copy goes straight into the lane's own input buffer on the lane's stream (it overlaps the other
        lanes' kernels and needs no staging tensor).  `to_host=True` also queues the D2H of the compact result into the
        lane's pinned buffers behind the decode (no host synchronisation): after `result.ready.synchronize()`,
        `result.hosted.unpack()` gives the per-image arrays."""
        k = self.k
        self.k = (k + 1) % len(self.streams)
        st = self.streams[k]
        on_host = not frames_u8.is_cuda
        if on_host:
            if not frames_u8.is_pinned():
                raise ValueError("host frames must be in pinned memory (tensor.pin_memory())")
            b, h, w, _ = frames_u8.shape
        else:
            main = torch.cuda.current_stream(frames_u8.device)
            ready = torch.cuda.Event()
            ready.record(main)                               # the frames are complete on the caller's stream
        with torch.cuda.stream(st):
            if on_host:
                buf = self.model.input_buffer(b, h, w, True, True, slot=k, conv_flags=self._conv_flags)
                buf.copy_(frames_u8, non_blocking=True)
                frames_u8 = buf
            else:
                st.wait_event(ready)
            unary, keys = self.model.forward_u8(frames_u8, fused_decode=True, slot=k, conv_flags=self._conv_flags)
            res = self.decoders[k].decode_fused(unary, keys)
            if to_host:
                if self._stages[k] is None:
                    self._stages[k] = D.HostStage(self.decoders[k].batch, cap=min(64, self.decoders[k].out.max_humans))
                res.hosted = res.to_host_async(self._stages[k])
            ev = torch.cuda.Event()
            ev.record(st)
        res.ready = ev
        return res

    def submit_raw(self, raw: torch.Tensor, fmt: str, src_hw, to_host: bool = False, flip: bool = False,
                   matrix: str = "bt601", full_range: bool = False, pitch: Optional[int] = None) -> D.DecodeResult:
        """``submit`` for raw video frames (see ``ingest_yuv``): `raw` u8 [B, nbytes] on the device or in PINNED host
        memory, in any source size.  Host bytes go H2D on the lane's stream into a raw staging buffer the lane owns
        (1.5 or 2 bytes per source pixel instead of 3 per network pixel after a host conversion); ppn_ingest_yuv then
        writes the lane's own input buffer and the forward and decode follow as in ``submit``."""
        if not (isinstance(raw, torch.Tensor) and raw.dtype == torch.uint8 and raw.dim() == 2):
            raise ValueError("submit_raw expects a uint8 tensor [B, nbytes]")
        k = self.k
        self.k = (k + 1) % len(self.streams)
        st = self.streams[k]
        on_host = not raw.is_cuda
        if on_host:
            if not raw.is_pinned():
                raise ValueError("host frames must be in pinned memory (tensor.pin_memory())")
        else:
            if raw.stride(1) != 1:
                raw = raw.contiguous()
            ready = torch.cuda.Event()
            ready.record(torch.cuda.current_stream(raw.device))     # the frames are complete on the caller's stream
        b, (h, w) = raw.shape[0], self.insize_hw
        with torch.cuda.stream(st):
            buf = self.model.input_buffer(b, h, w, True, True, slot=k, conv_flags=self._conv_flags)
            if on_host:
                if self._raw[k] is None or self._raw[k].shape != raw.shape:
                    self._raw[k] = torch.empty(raw.shape, dtype=torch.uint8, device=buf.device)
                self._raw[k].copy_(raw, non_blocking=True)
                raw = self._raw[k]
            else:
                st.wait_event(ready)
            _launch_ingest_yuv(raw, fmt, src_hw, buf, flip, matrix, full_range, pitch)
            unary, keys = self.model.forward_u8(buf, fused_decode=True, slot=k, conv_flags=self._conv_flags)
            res = self.decoders[k].decode_fused(unary, keys)
            if to_host:
                if self._stages[k] is None:
                    self._stages[k] = D.HostStage(self.decoders[k].batch, cap=min(64, self.decoders[k].out.max_humans))
                res.hosted = res.to_host_async(self._stages[k])
            ev = torch.cuda.Event()
            ev.record(st)
        res.ready = ev
        return res

    def flush(self):
        for st in self.streams:
            st.synchronize()
