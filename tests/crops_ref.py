"""NumPy restatement of the person crops' two kernels (include/ppn.h: ppn_people_rois, ppn_ingest_rois), test
infrastructure only.

`people_rois` applies the header's eight rules with plain loops over frames and slots; every f32 step is a NumPy f32 scalar
operation that is rounded on its own, as the kernel's is.  `ingest_rois` judges every rectangle as the header says and hands
a good one to tests/windows_ref.ingest_window -- the header's normative rule, word for word."""
import numpy as np

import windows_ref as WR

F = np.float32
OK, EMPTY, DEGENERATE, BAD = 0, 1, 2, 4
MODE_ROOT, MODE_PEOPLE = 0, 1
ALIGN = {"nv12": (2, 2), "i420": (2, 2), "yuyv": (1, 2), "bgr": (1, 1)}
HALF = F(0.5)


def scales(src_hw, coords_hw):
    """(sy, sx) as the host passes them."""
    return F(src_hw[0]) / F(coords_hw[0]), F(src_hw[1]) / F(coords_hw[1])


def aspect_of(out_hw):
    return F(out_hw[1]) / F(out_hw[0])


def _span(lo, hi, margin):
    c = F(F(lo + hi) * HALF)
    half = F(F(hi - lo) * HALF)
    return c, F(half + F(half * margin))


def _edges(c, half, size, align):
    """(e0, e1) in pixels, or None when an edge is not finite."""
    lo, hi = np.floor(F(c - half)), np.ceil(F(c + half))
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return None
    fs = F(size)
    i0, i1 = int(min(max(lo, F(0)), fs)), int(min(max(hi, F(0)), fs))
    return i0 // align * align, (i1 + align - 1) // align * align


def person_box(kp_cell, bbox, mode):
    """Rule 2 for one person: (f32 [4], finite) -- the box and whether every number that went into it is finite."""
    b = np.array(bbox[0], F)
    fin = bool(np.isfinite(b).all())
    if mode == MODE_PEOPLE:
        for j in range(1, len(kp_cell)):
            if kp_cell[j] < 0:
                continue
            v = np.array(bbox[j], F)
            fin = fin and bool(np.isfinite(v).all())
            b[0] = v[0] if v[0] < b[0] else b[0]
            b[1] = v[1] if v[1] < b[1] else b[1]
            b[2] = v[2] if v[2] > b[2] else b[2]
            b[3] = v[3] if v[3] > b[3] else b[3]
    return b, fin


def person_roi(kp_cell, bbox, src_hw, sy, sx, mode=MODE_PEOPLE, margin=0.1, aspect=0.0, align=(1, 1), min_size=8):
    """Rules 2 to 8 for one person that exists: ((y0, x0, h, w), status)."""
    sy, sx, margin, aspect = F(sy), F(sx), F(margin), F(aspect)
    with np.errstate(all="ignore"):
        b, fin = person_box(kp_cell, bbox, mode)
        if not fin:
            return (0, 0, 0, 0), DEGENERATE
        cy, hh = _span(F(b[0] * sy), F(b[2] * sy), margin)
        cx, hw = _span(F(b[1] * sx), F(b[3] * sx), margin)
        if aspect > 0:
            want = F(hh * aspect)
            if hw < want:
                hw = want
            else:
                hh = F(hw / aspect)
        ey, ex = _edges(cy, hh, src_hw[0], align[0]), _edges(cx, hw, src_hw[1], align[1])
    if ey is None or ex is None:
        return (0, 0, 0, 0), DEGENERATE
    h, w = ey[1] - ey[0], ex[1] - ex[0]
    if not (h >= min_size and w >= min_size):
        return (0, 0, 0, 0), DEGENERATE
    return (ey[0], ex[0], h, w), OK


def people_rois(count, kp_cell, bbox, src_hw, sy, sx, max_rois, mode=MODE_PEOPLE, margin=0.1, aspect=0.0, align=(1, 1),
                min_size=8, out=None):
    """count i32 [F], kp_cell i32 [F, M, K], bbox f32 [F, M, K, 4] -> (roi i32 [F, max_rois, 4], status i32 [F, max_rois]).
    `out`: a (roi, status) pair that is written in place (rows beyond max_rois stay as they are)."""
    Fr, M, K = kp_cell.shape
    roi, status = out if out is not None else (np.zeros((Fr, max_rois, 4), np.int32), np.zeros((Fr, max_rois), np.int32))
    for f in range(Fr):
        P = min(max(int(count[f]), 0), M)
        for r in range(max_rois):
            if r < P and kp_cell[f, r, 0] >= 0:
                roi[f, r], status[f, r] = person_roi(kp_cell[f, r], bbox[f, r], src_hw, sy, sx, mode, margin, aspect, align,
                                                     min_size)
            else:
                roi[f, r], status[f, r] = (0, 0, 0, 0), EMPTY
    return roi, status


def judge(rect, fmt, src_hw):
    """The status bits ppn_ingest_rois gives a rectangle: 0 (good), EMPTY or BAD."""
    y0, x0, h, w = (int(v) for v in rect)
    if (y0, x0, h, w) == (0, 0, 0, 0):
        return EMPTY
    if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > src_hw[0] or x0 + w > src_hw[1]:
        return BAD
    ay, ax = ALIGN[fmt]
    if y0 % ay or h % ay or x0 % ax or w % ax:
        return BAD
    return OK


def ingest_rois(raw, fmt, h, w, roi, size_hw, pitch=None, status=None, **kw):
    """raw u8 [F, >= frame bytes], roi i32 [F, R, 4] -> (u8 [F * R, dst_h, dst_w, 3], status i32 [F, R]); `status`: the table
    the bits are OR-ed into (a copy is returned), None: zeros."""
    roi = np.asarray(roi)
    Fr, R, _ = roi.shape
    status = np.zeros((Fr, R), np.int32) if status is None else np.array(status, np.int32)
    out = np.zeros((Fr * R, size_hw[0], size_hw[1], 3), np.uint8)
    for f in range(Fr):
        for r in range(R):
            bits = judge(roi[f, r], fmt, (h, w))
            status[f, r] |= bits
            if bits == OK:
                out[f * R + r] = WR.ingest_window(raw[f], fmt, h, w, tuple(int(v) for v in roi[f, r]), size_hw, pitch, **kw)
    return out, status
