"""NumPy restatement of the raw-video ingest (include/ppn.h: ppn_ingest_yuv), test infrastructure only.

Written from the rule in include/ppn.h and OpenCV's published source (modules/imgproc/src/color_yuv.simd.hpp, the
`YUV420p2RGB8Invoker` / `YUV422toRGB8Invoker` family): with int32 arithmetic

    y = max(0, Y - yoff) * CY;  uu = U - 128;  vv = V - 128;  h = 1 << 19
    R = sat8((y + h + CVR * vv) >> 20);  G = sat8((y + h + CVG * vv + CUG * uu) >> 20);  B = sat8((y + h + CUB * uu) >> 20)

and nearest-sample chroma: pixel (y, x) takes chroma sample (y >> 1, x >> 1) in NV12 / I420 and (y, x >> 1) in YUYV.
The coefficient sets are round(c * 2^20) of the usual three-decimal constants; row ("bt601", False) is OpenCV's
ITUR_BT_601_CY / CVR / CVG / CUG / CUB.  PARITY UNPINNED against cv2 itself (not installed here), as oracle/ingest_ref.py.

`ingest` = `to_rgb`, then oracle.ingest_ref.resize_linear_u8, then the flip of both axes.
"""
from __future__ import annotations

import numpy as np

from oracle import ingest_ref as I

# the real-valued constants (1.164 = 255/219, ...): (cy, cvr, cvg, cug, cub, yoff)
REAL = {
    ("bt601", False): (1.164, 1.596, -0.813, -0.391, 2.018, 16),
    ("bt709", False): (1.164, 1.793, -0.533, -0.213, 2.112, 16),
    ("bt601", True): (1.0, 1.402, -0.714136, -0.344136, 1.772, 0),
    ("bt709", True): (1.0, 1.5748, -0.468124, -0.187324, 1.8556, 0),
}
COEFF = {
    ("bt601", False): (1220542, 1673527, -852492, -409993, 2116026, 16),
    ("bt709", False): (1220542, 1880097, -558891, -223347, 2214593, 16),
    ("bt601", True): (1048576, 1470104, -748826, -360853, 1858077, 0),
    ("bt709", True): (1048576, 1651297, -490864, -196423, 1945738, 0),
}
FORMATS = ("nv12", "i420", "yuyv")


def frame_bytes(fmt: str, h: int, w: int, pitch=None) -> int:
    pitch = (2 * w if fmt == "yuyv" else w) if pitch is None else pitch
    if fmt == "yuyv":
        return h * pitch
    if fmt == "nv12":
        return h * pitch + (h // 2) * pitch
    return h * pitch + 2 * (h // 2) * (pitch // 2)


def planes(raw: np.ndarray, fmt: str, h: int, w: int, pitch=None):
    """Full-resolution (Y, U, V) u8 [h, w] arrays of one raw frame (a flat u8 array, planes as in the layouts above)."""
    raw = np.asarray(raw, dtype=np.uint8).reshape(-1)
    pitch = (2 * w if fmt == "yuyv" else w) if pitch is None else pitch
    if fmt == "yuyv":
        p = raw[:h * pitch].reshape(h, pitch)[:, :2 * w].reshape(h, w // 2, 4)
        Y = p[:, :, [0, 2]].reshape(h, w)
        return Y, np.repeat(p[:, :, 1], 2, axis=1), np.repeat(p[:, :, 3], 2, axis=1)
    Y = raw[:h * pitch].reshape(h, pitch)[:, :w]
    c = raw[h * pitch:]
    if fmt == "nv12":
        uv = c[:(h // 2) * pitch].reshape(h // 2, pitch)[:, :w].reshape(h // 2, w // 2, 2)
        U, V = uv[:, :, 0], uv[:, :, 1]
    elif fmt == "i420":
        pc, n = pitch // 2, (h // 2) * (pitch // 2)
        U = c[:n].reshape(h // 2, pc)[:, :w // 2]
        V = c[n:2 * n].reshape(h // 2, pc)[:, :w // 2]
    else:
        raise ValueError(fmt)
    up = lambda a: np.repeat(np.repeat(a, 2, axis=0), 2, axis=1)
    return Y, up(U), up(V)


def convert(Y, U, V, matrix: str = "bt601", full_range: bool = False) -> np.ndarray:
    """The pixel rule on arrays of equal shape: u8 [..., 3] RGB."""
    cy, cvr, cvg, cug, cub, yoff = COEFF[(matrix, bool(full_range))]
    # int32 as on the device: |y + h| <= 255 * 1220542 + 2^19 < 3.12e8 and the chroma terms stay below 2.84e8 together
    y = np.maximum(0, Y.astype(np.int32) - yoff) * np.int32(cy) + np.int32(1 << 19)
    uu, vv = U.astype(np.int32) - 128, V.astype(np.int32) - 128
    rgb = np.stack([(y + cvr * vv) >> 20, (y + cvg * vv + cug * uu) >> 20, (y + cub * uu) >> 20], axis=-1)
    assert rgb.dtype == np.int32
    return np.clip(rgb, 0, 255).astype(np.uint8)


def to_rgb(raw, fmt: str, h: int, w: int, pitch=None, matrix: str = "bt601", full_range: bool = False) -> np.ndarray:
    """The converted full-resolution picture, u8 [h, w, 3] RGB."""
    return convert(*planes(raw, fmt, h, w, pitch), matrix=matrix, full_range=full_range)


def ingest(raw, fmt: str, h: int, w: int, size_hw, pitch=None, matrix: str = "bt601", full_range: bool = False,
           flip: bool = False) -> np.ndarray:
    """to_rgb -> the project's resize rule -> optional flip of both axes: u8 [dst_h, dst_w, 3]."""
    r = I.resize_linear_u8(to_rgb(raw, fmt, h, w, pitch, matrix, full_range), tuple(size_hw))
    return np.ascontiguousarray(r[::-1, ::-1] if flip else r)


def pack(Y: np.ndarray, U: np.ndarray, V: np.ndarray, fmt: str, pitch=None, fill: int = 0xA5) -> np.ndarray:
    """One raw frame (flat u8) from Y [h, w] and 4:2:0 chroma U, V [h/2, w/2]; YUYV duplicates the chroma rows.  Bytes
    of a row beyond its content (a pitch wider than the row) hold `fill`."""
    h, w = Y.shape
    pitch = (2 * w if fmt == "yuyv" else w) if pitch is None else pitch
    if fmt == "yuyv":
        rows = np.full((h, pitch), fill, np.uint8)
        p = rows[:, :2 * w].reshape(h, w // 2, 4)
        p[:, :, 0], p[:, :, 2] = Y[:, 0::2], Y[:, 1::2]
        p[:, :, 1], p[:, :, 3] = np.repeat(U, 2, axis=0), np.repeat(V, 2, axis=0)
        return rows.reshape(-1)
    yp = np.full((h, pitch), fill, np.uint8)
    yp[:, :w] = Y
    if fmt == "nv12":
        cp = np.full((h // 2, pitch), fill, np.uint8)
        cp[:, 0:w:2], cp[:, 1:w:2] = U, V
        return np.concatenate([yp.reshape(-1), cp.reshape(-1)])
    up, vp = np.full((h // 2, pitch // 2), fill, np.uint8), np.full((h // 2, pitch // 2), fill, np.uint8)
    up[:, :w // 2], vp[:, :w // 2] = U, V
    return np.concatenate([yp.reshape(-1), up.reshape(-1), vp.reshape(-1)])
