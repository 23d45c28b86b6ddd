"""NumPy restatement of drawing onto raw video surfaces (include/ppn.h: ppn_rgb_to_yuv, ppn_draw_humans_yuv), test
infrastructure only.

The forward colour rule is written from the header: int32, arithmetic shift, sat8 = clamp to 0..255,

    Y = sat8((CYR R + CYG G + CYB B + (1 << 19) + (yoff << 20)) >> 20)
    U = sat8((CUR R + CUG G + CUB B + (1 << 19) + (128 << 20)) >> 20)
    V = sat8((CVR R + CVG G + CVB B + (1 << 19) + (128 << 20)) >> 20)

The paint rule stands on the UNCHANGED tests/render_ref.draw_ref: drawn on an all-0 and on an all-255 background, the two
outputs agree exactly where a pixel is painted, and there they hold its colour.  Luma takes its own pixel's colour; a
chroma sample the colour of the first painted pixel of its group in row-major order (2 x 2 in NV12 / I420, a row's pair in
YUYV); everything else keeps the source bytes.  `anchor` selects two deliberately WRONG chroma rules ("topleft": the
group's top-left pixel alone; "last": the last painted pixel of the group) so that a test can show that its cases tell the
rules apart.  Layouts are tests/yuv_ref.py's.
"""
from __future__ import annotations

import numpy as np

import render_ref as R
import yuv_ref as Y

# (matrix, full_range) -> ((CYR, CYG, CYB), (CUR, CUG, CUB), (CVR, CVG, CVB), yoff): the header's table
FORWARD = {
    ("bt601", False): ((269262, 528618, 102662), (-155423, -305128, 460551), (460551, -385654, -74897), 16),
    ("bt709", False): ((191455, 644067, 65019), (-105533, -355018, 460551), (460551, -418321, -42230), 16),
    ("bt601", True): ((313524, 615514, 119538), (-176932, -347356, 524288), (524288, -439026, -85262), 0),
    ("bt709", True): ((222927, 749942, 75707), (-120138, -404150, 524288), (524288, -476214, -48074), 0),
}
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
SETS = tuple(FORWARD)
GRID_GREY = (110, 110, 110)
ANCHORS = ("first", "topleft", "last")


def derive(matrix: str, full_range: bool):
    """The set from the exact definitions: round(c * 2^20), the G coefficient of U and V minus the sum of the other two."""
    kr, kb = KR_KB[matrix]
    sy, sc = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
    q = lambda c: int(round(c * (1 << 20)))
    cy = (q(kr * sy), q((1.0 - kr - kb) * sy), q(kb * sy))
    ur, ub = q(-kr / (2.0 * (1.0 - kb)) * sc), q(0.5 * sc)
    vr, vb = q(0.5 * sc), q(-kb / (2.0 * (1.0 - kr)) * sc)
    return cy, (ur, -(ur + ub), ub), (vr, -(vr + vb), vb), 0 if full_range else 16


def rgb_to_yuv(rgb, matrix: str = "bt601", full_range: bool = False) -> np.ndarray:
    """u8 [..., 3] RGB -> u8 [..., 3] (Y, U, V)."""
    cy, cu, cv, yoff = FORWARD[(matrix, bool(full_range))]
    c = np.asarray(rgb).astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    h = np.int32(1 << 19)
    out = np.stack([(cy[0] * r + cy[1] * g + cy[2] * b + h + np.int32(yoff << 20)) >> 20,
                    (cu[0] * r + cu[1] * g + cu[2] * b + h + np.int32(128 << 20)) >> 20,
                    (cv[0] * r + cv[1] * g + cv[2] * b + h + np.int32(128 << 20)) >> 20], axis=-1)
    assert out.dtype == np.int32
    return np.clip(out, 0, 255).astype(np.uint8)


def painted(B, H, W, count, kp_cell, bbox, kp_order, edges, palette, visbbox=False, grid_step=0):
    """(hit bool [B,H,W], colour u8 [B,H,W,3]) of ppn_draw_humans' decision P(y, x); grid_step 0: no grid."""
    kw = dict(visbbox=visbbox, grid=grid_step > 0, grid_step=max(int(grid_step), 1))
    lo = R.draw_ref(np.zeros((B, H, W, 3), np.uint8), count, kp_cell, bbox, kp_order, edges, palette, **kw)
    hi = R.draw_ref(np.full((B, H, W, 3), 255, np.uint8), count, kp_cell, bbox, kp_order, edges, palette, **kw)
    return (lo == hi).all(-1), lo


def _groups(a, gh, gw):
    """[H, W, ...] -> [H / gh, W / gw, gh * gw, ...], a group's pixels in row-major order."""
    H, W = a.shape[:2]
    a = a.reshape(H // gh, gh, W // gw, gw, *a.shape[2:])
    return np.moveaxis(a, 1, 2).reshape(H // gh, W // gw, gh * gw, *a.shape[4:])


def _write(buf, fmt, H, W, pitch, Yp, Uc, Vc):
    """The content bytes of one frame into `buf` (flat u8, modified): Y [H,W], chroma [H/2,W/2] (YUYV: [H,W/2])."""
    if fmt == "yuyv":
        p = buf[:H * pitch].reshape(H, pitch)[:, :2 * W].reshape(H, W // 2, 4)
        p[:, :, 0], p[:, :, 2], p[:, :, 1], p[:, :, 3] = Yp[:, 0::2], Yp[:, 1::2], Uc, Vc
        return
    n = Y.frame_bytes(fmt, H, W, pitch)
    content = Y.pack(np.ones((H, W), np.uint8), np.ones((H // 2, W // 2), np.uint8), np.ones((H // 2, W // 2), np.uint8), fmt,
                     pitch, fill=0).astype(bool)
    buf[:n][content] = Y.pack(Yp, Uc, Vc, fmt, pitch)[content]


def draw_surface(src, dst, fmt, H, W, hit, colour, pitch=None, matrix="bt601", full_range=False, anchor="first"):
    """One frame: `src`, `dst` flat u8 buffers holding the frame at offset 0 (dst is src for an in-place call); returns the
    drawn copy of `dst`.  Only content bytes change; every content byte comes from src or from a colour."""
    assert anchor in ANCHORS
    pitch = (2 * W if fmt == "yuyv" else W) if pitch is None else pitch
    Ys, Us, Vs = Y.planes(src, fmt, H, W, pitch)
    gh, gw = (1, 2) if fmt == "yuyv" else (2, 2)
    yuv = rgb_to_yuv(colour, matrix, full_range)
    Yn = np.where(hit, yuv[..., 0], Ys)
    hg, cg = _groups(hit, gh, gw), _groups(yuv, gh, gw)
    if anchor == "topleft":
        some, pick = hg[..., 0], np.zeros(hg.shape[:2], np.intp)
    elif anchor == "last":
        some, pick = hg.any(-1), hg.shape[2] - 1 - np.argmax(hg[..., ::-1], axis=-1)
    else:
        some, pick = hg.any(-1), np.argmax(hg, axis=-1)
    chosen = np.take_along_axis(cg, pick[..., None, None], axis=2)[:, :, 0]
    Un = np.where(some, chosen[..., 1], Us[::gh, ::gw])
    Vn = np.where(some, chosen[..., 2], Vs[::gh, ::gw])
    out = np.array(dst, np.uint8, copy=True).reshape(-1)
    _write(out, fmt, H, W, pitch, Yn.astype(np.uint8), Un.astype(np.uint8), Vn.astype(np.uint8))
    return out


def draw_rows(src, dst, fmt, H, W, hit, colour, **kw):
    """[F, nbytes] buffers, one frame per row: the drawn copy of `dst`."""
    return np.stack([draw_surface(src[f], dst[f], fmt, H, W, hit[f], colour[f], **kw) for f in range(len(src))])
