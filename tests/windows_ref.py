"""NumPy restatement of the windowed inference's two kernels (include/ppn.h: ppn_ingest_windows, ppn_merge_windows), test
infrastructure only.

`ingest_windows` crops the planes of a raw frame to the window and hands the crop to tests/yuv_ref.ingest (for "bgr":
oracle/ingest_ref) -- the header's normative rule, word for word.

`merge` applies the header's six rules with plain loops over candidates and keypoints; every f32 step is a NumPy f32 scalar
operation that is rounded on its own, as the kernel's is.  `fused_iou` / `recip_iou` / `fused_map` evaluate one step the way
a contracting compiler or a reciprocal divide would, emulated in float64; they are there only so that the knife-edge sweeps
can show that they tell the forms apart."""
import numpy as np

import yuv_ref as Y
from oracle import ingest_ref as I

F = np.float32
MAX_WINDOWS, MAX_CAND = 16, 512
CAND_OVERFLOW, OUT_OVERFLOW = 1, 2
FORMATS = Y.FORMATS + ("bgr",)


# ---- ingest ---------------------------------------------------------------------------------------------------------
def frame_bytes(fmt, h, w, pitch=None):
    if fmt == "bgr":
        return h * (3 * w if pitch is None else pitch)
    return Y.frame_bytes(fmt, h, w, pitch)


def crop(raw, fmt, h, w, win, pitch=None):
    """The window alone as a tight raw frame of its own (flat u8), (y0, x0, wh, ww) = win."""
    y0, x0, wh, ww = win
    raw = np.asarray(raw, dtype=np.uint8).reshape(-1)
    if fmt == "bgr":
        pitch = 3 * w if pitch is None else pitch
        return np.ascontiguousarray(raw[:h * pitch].reshape(h, pitch)[:, :3 * w].reshape(h, w, 3)[y0:y0 + wh, x0:x0 + ww])
    pitch = (2 * w if fmt == "yuyv" else w) if pitch is None else pitch
    if fmt == "yuyv":
        assert x0 % 2 == 0 and ww % 2 == 0
        rows = raw[:h * pitch].reshape(h, pitch)
        return np.ascontiguousarray(rows[y0:y0 + wh, 2 * x0:2 * (x0 + ww)]).reshape(-1)
    assert x0 % 2 == 0 and ww % 2 == 0 and y0 % 2 == 0 and wh % 2 == 0
    Yp = raw[:h * pitch].reshape(h, pitch)[y0:y0 + wh, x0:x0 + ww]
    c = raw[h * pitch:]
    if fmt == "nv12":
        uv = c[:(h // 2) * pitch].reshape(h // 2, pitch)[y0 // 2:(y0 + wh) // 2, x0:x0 + ww]
        return np.concatenate([Yp.reshape(-1), uv.reshape(-1)])
    pc, n = pitch // 2, (h // 2) * (pitch // 2)
    U = c[:n].reshape(h // 2, pc)[y0 // 2:(y0 + wh) // 2, x0 // 2:(x0 + ww) // 2]
    V = c[n:2 * n].reshape(h // 2, pc)[y0 // 2:(y0 + wh) // 2, x0 // 2:(x0 + ww) // 2]
    return np.concatenate([Yp.reshape(-1), U.reshape(-1), V.reshape(-1)])


def ingest_window(raw, fmt, h, w, win, size_hw, pitch=None, matrix="bt601", full_range=False, flip=False, dst_bgr=False):
    """One window of one raw frame: u8 [dst_h, dst_w, 3]."""
    c = crop(raw, fmt, h, w, win, pitch)
    if fmt == "bgr":
        r = I.resize_linear_u8(c, tuple(size_hw))
        r = np.ascontiguousarray(r[::-1, ::-1] if flip else r)
        return r if dst_bgr else np.ascontiguousarray(r[:, :, ::-1])        # ppn_ingest_frames with swap_rb = !dst_bgr
    r = Y.ingest(c, fmt, win[2], win[3], size_hw, None, matrix, full_range, flip)
    return np.ascontiguousarray(r[:, :, ::-1]) if dst_bgr else r


def ingest_windows(raw, fmt, h, w, windows, size_hw, pitch=None, **kw):
    """raw u8 [F, >= frame bytes] -> u8 [F * n, dst_h, dst_w, 3]; image f * n + i is window i of frame f."""
    return np.stack([ingest_window(raw[f], fmt, h, w, win, size_hw, pitch, **kw) for f in range(len(raw)) for win in windows])


# ---- merge ----------------------------------------------------------------------------------------------------------
def area(b):
    return F(F(b[2]) - F(b[0])) * F(F(b[3]) - F(b[1]))


def iou(bk, ak, bc, ac, fused=False, recip=False):
    """track_ref.iou; fused: inter / fma-style (ak + ac - inter) in one rounding; recip: inter * (1 / den)."""
    tl0, tl1 = max(F(bk[0]), F(bc[0])), max(F(bk[1]), F(bc[1]))
    br0, br1 = min(F(bk[2]), F(bc[2])), min(F(bk[3]), F(bc[3]))
    if not (tl0 < br0 and tl1 < br1):
        return F(0)                          # inter is (anything) * 0: the quotient is 0 or NaN, which counts as 0
    inter = F(F(br0 - tl0) * F(br1 - tl1)) * (F(1) if (tl0 < br0 and tl1 < br1) else F(0))
    with np.errstate(all="ignore"):
        if fused:
            den = F(np.float64(ak) + np.float64(ac) - np.float64(inter))
            v = F(inter) / den
        elif recip:
            v = F(inter * F(F(1) / F(F(ak + ac) - inter)))
        else:
            v = F(inter) / F(F(ak + ac) - inter)
    return F(v) if v > 0 else F(0)


def win_map(win, inH, inW):
    y0, x0, h, w = win
    return F(h) / F(inH), F(w) / F(inW), F(y0), F(x0)


def map_coord(v, s, o, fused=False):
    if fused:
        return F(np.float64(F(v)) * np.float64(s) + np.float64(o))         # fma: one rounding
    return F(F(F(v) * s) + o)


def map_box(b, m, fused=False):
    sy, sx, y0, x0 = m
    return np.array([map_coord(b[0], sy, y0, fused), map_coord(b[1], sx, x0, fused), map_coord(b[2], sy, y0, fused),
                     map_coord(b[3], sx, x0, fused)], F)


def fresh_outputs(frames, max_out, K, fill=None):
    """Arrays as a WindowMerger starts with, or filled with a sentinel byte so that untouched rows show."""
    if fill is None:
        return dict(count=np.zeros(frames, np.int32), src=np.full((frames, max_out, K), -1, np.int32),
                    bbox=np.zeros((frames, max_out, K, 4), F), score=np.zeros((frames, max_out, K), F),
                    flags=np.zeros(frames, np.int32))
    mk = lambda shape, dt: np.full(int(np.prod(shape)) * 4, fill, np.uint8).view(dt).reshape(shape)
    return dict(count=mk((frames,), np.int32), src=mk((frames, max_out, K), np.int32), bbox=mk((frames, max_out, K, 4), F),
                score=mk((frames, max_out, K), F), flags=mk((frames,), np.int32))


def merge(windows, inHW, count, kp_cell, bbox, score, frames, max_out, merge_thr=0.3, fuse=True, out=None, fused_iou=False,
          recip_iou=False, fused_map=False):
    """count i32 [F*n], kp_cell i32 [F*n, M, K], bbox f32 [F*n, M, K, 4], score f32 [F*n, M, K].  Returns (out, keeper):
    out as fresh_outputs, written as the kernel writes it; keeper[f] maps every candidate (i, p) to the (i, p) of the kept
    candidate it belongs to (itself when kept)."""
    n = len(windows)
    B, M, K = kp_cell.shape
    assert B == frames * n
    inH, inW = inHW
    thr = F(merge_thr)
    if out is None:
        out = fresh_outputs(frames, max_out, K)
    maps = [win_map(w, inH, inW) for w in windows]
    keepers = []
    for f in range(frames):
        flags = 0
        # 1
        cand = []
        for i in range(n):
            b = f * n + i
            for p in range(min(max(int(count[b]), 0), M)):
                if kp_cell[b, p, 0] >= 0 and not np.isnan(score[b, p, 0]):
                    cand.append((i, p))
        if len(cand) > MAX_CAND:
            flags |= CAND_OVERFLOW
            cand = cand[:MAX_CAND]
        # 2 (root boxes), 3
        root = {c: map_box(bbox[f * n + c[0], c[1], 0], maps[c[0]], fused_map) for c in cand}
        ar = {c: area(root[c]) for c in cand}
        order = sorted(cand, key=lambda c: (-float(F(score[f * n + c[0], c[1], 0])), c))    # -0.0 and +0.0: one value
        # 4
        kept, keeper = [], {}
        for c in order:
            k = next((k for k in kept if k[0] != c[0] and iou(root[k], ar[k], root[c], ar[c], fused_iou, recip_iou) >= thr), None)
            if k is None:
                kept.append(c)
                keeper[c] = c
            else:
                keeper[c] = k
        keepers.append(keeper)
        # 5, 6
        out["count"][f] = len(kept)
        if len(kept) > max_out:
            flags |= OUT_OVERFLOW
        out["flags"][f] = flags
        for r, k in enumerate(kept[:max_out]):
            members = [c for c in order if keeper[c] == k]                                    # walk order, k first
            assert members[0] == k
            for j in range(K):
                best = None
                for c in (members if (fuse and j >= 1) else [k]):
                    b = f * n + c[0]
                    if kp_cell[b, c[1], j] < 0:
                        continue
                    if best is None or F(score[b, c[1], j]) > F(score[f * n + best[0], best[1], j]):
                        best = c
                if best is None:
                    out["src"][f, r, j], out["bbox"][f, r, j], out["score"][f, r, j] = -1, 0, 0
                else:
                    b = f * n + best[0]
                    out["src"][f, r, j] = best[0] * M + best[1]
                    out["bbox"][f, r, j] = map_box(bbox[b, best[1], j], maps[best[0]], fused_map)
                    out["score"][f, r, j] = score[b, best[1], j]
    return out, keepers
