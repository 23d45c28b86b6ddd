"""Train-time augmentation on the device (reference: aug.py:13-160, `IAA` + `ToNormalizedTensor`).

    aug = TrainAugmenter(insize=(384, 384), seed=0, mode="train")
    x, targets = aug(src_u8, src_hw, packed, step)          # raw u8 pictures + packed annotations -> train_step's inputs
    trainer.train_step(x, targets)

Geometry.  Coordinates are pixel indices, pixel centres at integers.  For a picture of valid size h x w and an output of
outH x outW the forward map F (source point -> output point) is
  1. rotation by theta (positive = clockwise on the screen, y pointing down) and isotropic scale s about
     ((w-1)/2, (h-1)/2);
  2. crop: minus (left, top); w' = w - left - right, h' = h - top - bottom, each side int(0.1 * u * h) or int(0.1 * u * w)
     with its own uniform u (aug.py:50; order top, right, bottom, left as imgaug's `px`);
  3. centre-aligned resize x' = (x + 0.5) * outW / w' - 0.5 (the convention of csrc/ingest.hip).
mode="train" draws theta in [-40, 40] degrees, s in [0.35, 2.5] and the four u per image from prng's splitmix64 streams,
keyed by (seed, step, image index): the same seed gives the same batch on any box.  mode="val" is the resize alone
(aug.py:55-57).  F and F^-1 are built on the host in float64 and rounded to f32 [B,2,3]; the two kernels
(csrc/augment.hip) use only those twelve numbers per image.  This is not imgaug's pixel arithmetic:
one resampling pass instead of three, one half-pixel convention for pixels and labels, this project's interpolation rule.

Options the reference does not have (both off by default; mode="val" ignores them; rules in include/ppn.h):
  * mirror_p: with that probability an image is mirrored left-right.  The reflection x -> (w - 1) - x is a factor of F,
    applied before the rotation, so the image kernel needs nothing; the label kernel additionally swaps the left_* / right_*
    point slots and visible bits (tta.mirror_tables()).  This is the pixel-index convention of this file -- column i of a
    w-wide picture goes to column w - 1 - i -- not the 1 - x of the cell-relative offsets in tta.py.
  * color: a ColorJitter.  Saturation, contrast about 128, brightness, a per-channel cast and pixel noise, folded on the
    host into ten integers per image that the image kernel applies in i32 in front of its stores.
Their draws come from streams of their own, so the geometry of a (seed, step, image) does not depend on them:
  stream_seed(key, b)                        u[0..5]: theta, scale, crop top / right / bottom / left   (as before)
  stream_seed(stream_seed(key, b), 1)        u[0]: mirror iff u < mirror_p;  u[1]: grey iff u < gray_p;  u[2]: saturation;
                                             u[3]: contrast;  u[4]: brightness;  u[5..7]: cast r, g, b;  u[8]: noise sigma
                                             (all nine are drawn whatever the options, each uniform over its range)
  stream_seed(stream_seed(key, b), 2)        the image's noise key (splitmix64 start value; the kernel draws per pixel)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import config as cfg
from . import lib as L
from . import prng
from . import targets as T

ROTATE_DEG = (-40.0, 40.0)      # aug.py:46
SCALE = (0.35, 2.5)             # aug.py:47
CROP_FRAC = 0.1                 # aug.py:50
COLOR_IDENTITY = (256, 256, 256, 256, 0, 0, 0, 0, 0, 0)      # a `color` row that changes nothing


@dataclass
class ColorJitter:
    """Ranges of the photometric jitter (u8 units): brightness offset in [-brightness, brightness]; contrast (about 128)
    and saturation factors uniform in their ranges; each channel's gain times 1 + cast * [-1, 1]; noise sd uniform in
    `noise`; with probability gray_p the picture turns grey (saturation 0)."""
    brightness: float = 32
    contrast: Tuple[float, float] = (0.6, 1.4)
    saturation: Tuple[float, float] = (0.5, 1.5)
    cast: float = 0.1
    noise: Tuple[float, float] = (0.0, 8.0)
    gray_p: float = 0.1


def color_rows(u: np.ndarray, cj: ColorJitter, noise_keys: np.ndarray) -> np.ndarray:
    """i32 [B,10]: the ten integers of every image from its uniforms u f64[B,9] (columns 1..8, module docstring) and its
    noise key (u64), clamped to the kernel's ranges.  Rounding is to nearest, ties to even."""
    lerp = lambda r, t: float(r[0]) + (float(r[1]) - float(r[0])) * t
    sat = np.where(u[:, 1] < cj.gray_p, 0.0, lerp(cj.saturation, u[:, 2]))
    contrast = lerp(cj.contrast, u[:, 3])
    brightness = float(cj.brightness) * (2.0 * u[:, 4] - 1.0)
    rows = np.zeros((u.shape[0], 10), np.int32)
    rows[:, 0] = np.clip(np.rint(256.0 * sat), 0, 512)
    for c in range(3):
        cast = 1.0 + float(cj.cast) * (2.0 * u[:, 5 + c] - 1.0)
        rows[:, 1 + c] = np.clip(np.rint(256.0 * contrast * cast), 0, 1024)
        rows[:, 4 + c] = np.clip(np.rint(128.0 - 128.0 * contrast + brightness), -255, 255)
    rows[:, 7] = np.clip(np.rint(128.0 * lerp(cj.noise, u[:, 8])), 0, 4096)
    rows[:, 8:10] = np.ascontiguousarray(noise_keys, np.uint64).view(np.int32).reshape(-1, 2)      # little-endian: lo, hi
    return rows


def affine_matrices(theta_deg, scale, crop, src_hw, out_hw, mirror=None) -> Tuple[np.ndarray, np.ndarray]:
    """(F, F^-1) as float64 [B,3,3] homogeneous matrices acting on (x, y, 1).  crop is (top, right, bottom, left).
    mirror: a bool per image (or one for all); a mirrored image's source point is reflected, x -> (w - 1) - x, before the
    rotation.  None or False leaves the matrices bit for bit what they are without it."""
    theta, s = np.atleast_1d(np.asarray(theta_deg, np.float64)), np.atleast_1d(np.asarray(scale, np.float64))
    crop, hw = np.atleast_2d(np.asarray(crop, np.int64)), np.atleast_2d(np.asarray(src_hw, np.float64))
    flip = np.zeros(1, bool) if mirror is None else np.atleast_1d(np.asarray(mirror)).astype(bool)
    B = max(theta.shape[0], s.shape[0], crop.shape[0], hw.shape[0], flip.shape[0])     # scalars / single rows: every image
    theta, s, flip = np.broadcast_to(theta, (B,)), np.broadcast_to(s, (B,)), np.broadcast_to(flip, (B,))
    crop, hw = np.broadcast_to(crop, (B, 4)), np.broadcast_to(hw, (B, 2))
    outH, outW = float(out_hw[0]), float(out_hw[1])
    fwd, inv = np.zeros((B, 3, 3)), np.zeros((B, 3, 3))
    for b in range(B):
        h, w = hw[b]
        top, right, bottom, left = (float(v) for v in crop[b])
        wc, hc = w - left - right, h - top - bottom
        if wc < 1 or hc < 1 or s[b] <= 0:
            raise ValueError(f"image {b}: crop {crop[b].tolist()} leaves nothing of {int(h)}x{int(w)}, or scale <= 0")
        c, sn = np.cos(np.deg2rad(theta[b])), np.sin(np.deg2rad(theta[b]))
        c, sn = (0.0 if abs(c) < 1e-15 else c), (0.0 if abs(sn) < 1e-15 else sn)     # multiples of 90 degrees: exact
        cx, cy = (w - 1.0) / 2.0, (h - 1.0) / 2.0

        def about_centre(m):
            t_in = np.array([[1, 0, -cx], [0, 1, -cy], [0, 0, 1.0]])
            t_out = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
            return t_out @ m @ t_in

        rot = about_centre(np.array([[s[b] * c, -s[b] * sn, 0], [s[b] * sn, s[b] * c, 0], [0, 0, 1.0]]))
        rot_i = about_centre(np.array([[c / s[b], sn / s[b], 0], [-sn / s[b], c / s[b], 0], [0, 0, 1.0]]))
        cr = np.array([[1, 0, -left], [0, 1, -top], [0, 0, 1.0]])
        cr_i = np.array([[1, 0, left], [0, 1, top], [0, 0, 1.0]])
        kx, ky = outW / wc, outH / hc
        rz = np.array([[kx, 0, 0.5 * kx - 0.5], [0, ky, 0.5 * ky - 0.5], [0, 0, 1.0]])
        rz_i = np.array([[1 / kx, 0, 0.5 / kx - 0.5], [0, 1 / ky, 0.5 / ky - 0.5], [0, 0, 1.0]])
        fwd[b] = rz @ cr @ rot
        inv[b] = rot_i @ cr_i @ rz_i
        if flip[b]:
            refl = np.array([[-1, 0, w - 1.0], [0, 1, 0], [0, 0, 1.0]])      # its own inverse
            fwd[b] = fwd[b] @ refl
            inv[b] = refl @ inv[b]
    return fwd, inv


def sample_params(seed: int, step: int, src_hw, out_hw, mode: str = "train", mirror_p: float = 0.0,
                  color: Optional[ColorJitter] = None) -> Dict[str, np.ndarray]:
    """Per-image augmentation parameters (pure host code): theta f64[B] (degrees), scale f64[B], crop i32[B,4]
    (top, right, bottom, left), fwd / inv f32[B,2,3].  src_hw i32[B,2] holds each picture's valid (h, w).
    With mirror_p > 0 or a ColorJitter the dict also holds mirror bool[B] (already part of fwd / inv) and color
    i32[B,10] (None without a ColorJitter); a call without them returns the five keys it always returned.  mode="val"
    mirrors nobody and returns color None."""
    if mode not in ("train", "val"):
        raise ValueError(f"mode {mode!r}: 'train' or 'val'")
    if not 0.0 <= float(mirror_p) <= 1.0:
        raise ValueError(f"mirror_p {mirror_p}: a probability")
    hw = np.asarray(src_hw, np.int64).reshape(-1, 2)
    B = hw.shape[0]
    theta, scale, crop = np.zeros(B), np.ones(B), np.zeros((B, 4), np.int32)
    options = float(mirror_p) > 0.0 or color is not None
    mirror, rows = np.zeros(B, bool), None
    if mode == "train":
        key = prng.stream_seed(int(seed), int(step))
        kbs = np.zeros(B, np.uint64)
        for b in range(B):
            kbs[b] = kb = prng.stream_seed(key, b)
            u = prng.uniform01(kb, 6).astype(np.float64)
            theta[b] = ROTATE_DEG[0] + (ROTATE_DEG[1] - ROTATE_DEG[0]) * u[0]
            scale[b] = SCALE[0] + (SCALE[1] - SCALE[0]) * u[1]
            h, w = int(hw[b, 0]), int(hw[b, 1])
            crop[b] = [int(CROP_FRAC * u[2] * h), int(CROP_FRAC * u[3] * w), int(CROP_FRAC * u[4] * h),
                       int(CROP_FRAC * u[5] * w)]
        if options:                                                  # streams of their own (module docstring), all images at once
            u = prng.uniform01_rows(prng.stream_seeds(kbs, 1), 9).astype(np.float64)
            mirror = u[:, 0] < float(mirror_p)
            if color is not None:
                rows = color_rows(u, color, prng.stream_seeds(kbs, 2))
    fwd, inv = affine_matrices(theta, scale, crop, hw, out_hw, mirror if mirror.any() else None)
    p = dict(theta=theta, scale=scale, crop=crop, fwd=np.ascontiguousarray(fwd[:, :2, :], np.float32),
             inv=np.ascontiguousarray(inv[:, :2, :], np.float32))
    if options:
        p.update(mirror=mirror, color=rows)
    return p


_KP_MIRROR = []


def _default_kp_mirror():
    if not _KP_MIRROR:
        from . import tta
        _KP_MIRROR.extend(tta.mirror_tables()[0])
    return _KP_MIRROR


def _dev(a, dtype, device):
    """NumPy array or tensor -> contiguous device tensor of `dtype` (a device tensor of that dtype is passed through)."""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=device, dtype=dtype).contiguous()


def augment_images(src_u8, src_hw, inv, out_hw, out_u8: Optional[torch.Tensor] = None,
                   out_f32: Optional[torch.Tensor] = None, want_u8: bool = False, want_f32: bool = True, device="cuda",
                   color=None):
    """u8 [B,Hs,Ws,3] pictures (padded to a common size, valid sizes src_hw i32[B,2]) through inv f32[B,2,3]
    -> (u8 [B,outH,outW,3] or None, normalised f32 [B,3,outH,outW] or None).  Outputs given by the caller are reused.
    color: i32 [B,10] rows (sample_params, COLOR_IDENTITY) -> the colour / noise step of ppn_augment_images_color; None
    runs ppn_augment_images."""
    dev = torch.device(device)
    src = _dev(src_u8, torch.uint8, dev)
    if src.dim() != 4 or src.shape[3] != 3:
        raise ValueError(f"src_u8 must be [B,Hs,Ws,3], got {tuple(src.shape)}")
    B, Hs, Ws, _ = src.shape
    if not isinstance(src_hw, torch.Tensor):
        hw = np.asarray(src_hw).reshape(-1, 2)
        if hw.shape[0] != B or (hw < 1).any() or (hw[:, 0] > Hs).any() or (hw[:, 1] > Ws).any():
            raise ValueError(f"src_hw {hw.tolist()} does not fit {B} pictures padded to {Hs}x{Ws}")
    hwd, invd = _dev(src_hw, torch.int32, dev), _dev(inv, torch.float32, dev)
    if tuple(hwd.shape) != (B, 2) or tuple(invd.shape) != (B, 2, 3):
        raise ValueError("src_hw must be [B,2] and inv [B,2,3]")
    outH, outW = int(out_hw[0]), int(out_hw[1])
    if out_u8 is None and want_u8:
        out_u8 = torch.empty((B, outH, outW, 3), dtype=torch.uint8, device=dev)
    if out_f32 is None and want_f32:
        out_f32 = torch.empty((B, 3, outH, outW), dtype=torch.float32, device=dev)
    for t, shape, dt in ((out_u8, (B, outH, outW, 3), torch.uint8), (out_f32, (B, 3, outH, outW), torch.float32)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device.type != dev.type):
            raise ValueError(f"output buffer must be a contiguous {dt} {shape} tensor on {dev}")
    outs = (out_u8.data_ptr() if out_u8 is not None else None, out_f32.data_ptr() if out_f32 is not None else None)
    if color is None:
        L.check(L.load().ppn_augment_images(src.data_ptr(), hwd.data_ptr(), invd.data_ptr(), B, Hs, Ws, outH, outW, *outs,
                                            L.current_stream_ptr()), "ppn_augment_images")
    else:
        cold = _dev(color, torch.int32, dev)
        if tuple(cold.shape) != (B, 10):
            raise ValueError(f"color must be i32 [{B},10], got {tuple(cold.shape)}")
        L.check(L.load().ppn_augment_images_color(src.data_ptr(), hwd.data_ptr(), invd.data_ptr(), cold.data_ptr(), B, Hs,
                                                  Ws, outH, outW, *outs, L.current_stream_ptr()),
                "ppn_augment_images_color")
    return out_u8, out_f32


def augment_people(packed, fwd, out_hw, out=None, device="cuda", mirror=None, kp_mirror: Optional[Sequence[int]] = None):
    """The packed arrays of targets.pack_people (NumPy or device tensors) through fwd f32[B,2,3] -> (people, visible,
    count) device tensors, transformed and compacted, ready for targets.encode_targets.  `out`: three tensors to reuse.
    mirror: a flag per image (bool / int array or device tensor) whose fwd holds the reflection -> those images' left / right
    point slots and visible bits are swapped by ppn_augment_people_mirror through kp_mirror (default: the project
    skeleton's tta.mirror_tables(); another table sets K = len(kp_mirror)).  None runs ppn_augment_people."""
    dev = torch.device(device)
    people, visible, count = packed
    pd, vd, cd = _dev(people, torch.float32, dev), _dev(visible, torch.int32, dev), _dev(count, torch.int32, dev)
    fd = _dev(fwd, torch.float32, dev)
    B, pmax, row = pd.shape
    K = cfg.K
    if mirror is not None:
        if kp_mirror is None:
            kp_mirror = _default_kp_mirror()
        K = len(kp_mirror)
    elif kp_mirror is not None:
        raise ValueError("kp_mirror without mirror flags")
    if row != 5 + 2 * (K - 1) or tuple(vd.shape) != (B, pmax) or tuple(cd.shape) != (B,) or tuple(fd.shape) != (B, 2, 3):
        raise ValueError("packed must be (people [B,pmax,5+2(K-1)], visible [B,pmax], count [B]) and fwd [B,2,3]")
    if out is None:
        out = (torch.empty_like(pd), torch.empty_like(vd), torch.empty_like(cd))
    po, vo, co = out
    for t, ref in ((po, pd), (vo, vd), (co, cd)):
        if t.shape != ref.shape or t.dtype != ref.dtype or not t.is_contiguous() or t.device != ref.device:
            raise ValueError("out must match the packed arrays' shapes, dtypes and device")
    if mirror is None:
        L.check(L.load().ppn_augment_people(pd.data_ptr(), vd.data_ptr(), cd.data_ptr(), fd.data_ptr(), B, pmax, K,
                                            int(out_hw[0]), int(out_hw[1]), po.data_ptr(), vo.data_ptr(), co.data_ptr(),
                                            L.current_stream_ptr()), "ppn_augment_people")
    else:
        md = _dev(mirror, torch.int32, dev)
        if tuple(md.shape) != (B,):
            raise ValueError(f"mirror must hold {B} flags, got {tuple(md.shape)}")
        table = (C.c_int32 * K)(*[int(v) for v in kp_mirror])
        L.check(L.load().ppn_augment_people_mirror(pd.data_ptr(), vd.data_ptr(), cd.data_ptr(), fd.data_ptr(),
                                                   md.data_ptr(), table, B, pmax, K, int(out_hw[0]), int(out_hw[1]),
                                                   po.data_ptr(), vo.data_ptr(), co.data_ptr(), L.current_stream_ptr()),
                "ppn_augment_people_mirror")
    return po, vo, co


class TrainAugmenter:
    """Raw u8 pictures + packed annotations -> (x, targets) for PPNTrainer.train_step, without the host touching a pixel
    or a target.  insize is (width, height) like targets.encode_targets; the output grid is insize / 16.

    The outputs are buffers this object owns and reuses: after the first call of a given batch geometry a call allocates
    nothing on the device (device-tensor inputs; NumPy inputs cost their own upload) and only enqueues on the current
    stream, so use (x, targets) -- or copy them -- before the next call.

    mirror_p / color (a ColorJitter) switch on the left-right mirror and the colour / noise step (module docstring) in
    mode="train"; mode="val" ignores both.  Their per-image parameters ride in the same small upload as the matrices.  With
    both off the launches and every output bit are what they are without them."""

    def __init__(self, insize=(384, 384), seed: int = 0, mode: str = "train", local_grid=(21, 21), device="cuda",
                 mirror_p: float = 0.0, color: Optional[ColorJitter] = None):
        if mode not in ("train", "val"):
            raise ValueError(f"mode {mode!r}: 'train' or 'val'")
        if not 0.0 <= float(mirror_p) <= 1.0:
            raise ValueError(f"mirror_p {mirror_p}: a probability")
        self.mirror_p, self.color = (float(mirror_p), color) if mode == "train" else (0.0, None)
        self._kp_mirror = None
        if self.mirror_p > 0.0:
            self._kp_mirror = _default_kp_mirror()
        if insize[0] % 16 or insize[1] % 16:
            raise ValueError("insize must be a multiple of 16")
        self.insize, self.seed, self.mode, self.local_grid = (int(insize[0]), int(insize[1])), int(seed), mode, local_grid
        self.outsize = (self.insize[0] // 16, self.insize[1] // 16)
        self.out_hw = (self.insize[1], self.insize[0])
        self.device = torch.device(device)
        self._key, self._buf = None, None
        self.params = None              # sample_params of the last call

    def _buffers(self, B, pmax):
        if self._key != (B, pmax):
            dev, (outH, outW) = self.device, self.out_hw
            row = 5 + 2 * (cfg.K - 1)
            self._buf = dict(
                x=torch.empty((B, 3, outH, outW), dtype=torch.float32, device=dev),
                people=(torch.empty((B, pmax, row), dtype=torch.float32, device=dev),
                        torch.empty((B, pmax), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev)),
                # one upload per call: fwd | inv (f32 bits, 12 words per image), then color rows (10) and mirror flags (1)
                up=torch.empty((B * (12 + (10 if self.color is not None else 0) + (1 if self._kp_mirror else 0)),),
                               dtype=torch.int32, device=dev),
                hw=torch.empty((B, 2), dtype=torch.int32, device=dev), targets=None)
            self._key = (B, pmax)
        return self._buf

    def __call__(self, src_u8, src_hw, packed, step: int):
        """src_u8 u8[B,Hs,Ws,3], src_hw i32[B,2] valid (h, w) (a host array: the sampler runs on the host), packed =
        (people, visible, count) as NumPy arrays or device tensors -> (x f32[B,3,H,W], targets dict)."""
        hw_host = src_hw.cpu().numpy() if isinstance(src_hw, torch.Tensor) else np.asarray(src_hw)
        self.params = p = sample_params(self.seed, step, hw_host, self.out_hw, self.mode, self.mirror_p, self.color)
        B, pmax = int(packed[0].shape[0]), int(packed[0].shape[1])
        buf = self._buffers(B, pmax)
        parts = [p["fwd"].view(np.int32).reshape(-1), p["inv"].view(np.int32).reshape(-1)]
        if self.color is not None:
            parts.append(p["color"].reshape(-1))
        if self._kp_mirror:
            parts.append(p["mirror"].astype(np.int32))
        up = buf["up"]
        up.copy_(torch.from_numpy(np.concatenate(parts)))          # 48 .. 92 bytes per image, from pageable memory
        mats = up[:12 * B].view(torch.float32).view(2, B, 2, 3)
        fwd, inv = mats[0], mats[1]
        color = up[12 * B:22 * B].view(B, 10) if self.color is not None else None
        mirror = up[up.numel() - B:] if self._kp_mirror else None
        if not isinstance(src_hw, torch.Tensor):
            if hw_host.shape != (B, 2) or (hw_host < 1).any() or (hw_host[:, 0] > src_u8.shape[1]).any() or \
                    (hw_host[:, 1] > src_u8.shape[2]).any():
                raise ValueError(f"src_hw {hw_host.tolist()} does not fit pictures padded to {tuple(src_u8.shape[1:3])}")
            buf["hw"].copy_(torch.from_numpy(np.ascontiguousarray(hw_host, np.int32)))
            src_hw = buf["hw"]
        _, x = augment_images(src_u8, src_hw, inv, self.out_hw, out_f32=buf["x"], device=self.device, color=color)
        people = augment_people(packed, fwd, self.out_hw, out=buf["people"], device=self.device, mirror=mirror,
                                kp_mirror=self._kp_mirror)
        buf["targets"] = T.encode_targets(people, self.insize, self.outsize, self.local_grid, device=self.device,
                                          out=buf["targets"])
        return x, buf["targets"]
