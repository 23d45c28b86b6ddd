"""NumPy restatement of the redaction's two kernels (include/ppn.h: ppn_redact_cells, ppn_redact_yuv), test infrastructure
only, written from the header on tests/yuv_ref.py's frame layouts (packed BGR: rows of `pitch` >= 3 * w bytes).

`cells` walks images, people and cells with plain loops, every f32 step a NumPy f32 scalar operation rounded on its own;
`redact` builds each masked cell's sample sets as lists of byte offsets into the flat frame and replaces them by their
rounded mean or the fill byte.  `rule=` selects a deliberately WRONG variant, so that the tests can show that the cases tell
it from the right one:
    "ttl_reload"   a covered cell's ttl becomes hold instead of hold + 1            (cells)
    "last_col"     the last covered column is r / cell instead of (r - 1) / cell    (cells)
    "trunc"        the mean is s / n, not (s + (n >> 1)) / n                        (redact)
    "full_n"       n is the whole cell's sample count even at the picture's border  (redact)
    "uv_together"  U and V are averaged together                                    (redact)
"""
import numpy as np

F = np.float32
HALF = F(0.5)
FALLBACK_PERSON, FALLBACK_NONE = 0, 1
FLAG_BAD_BOX = 1
MOSAIC, FILL = 0, 1
CELLS_RULES = (None, "ttl_reload", "last_col")
REDACT_RULES = (None, "trunc", "full_n", "uv_together")


def scales(src_hw, coords_hw):
    """(sy, sx) as the host passes them."""
    return F(src_hw[0]) / F(coords_hw[0]), F(src_hw[1]) / F(coords_hw[1])


def grid_of(src_hw, cell):
    """(CH, CW, MW)."""
    ch, cw = -(-src_hw[0] // cell), -(-src_hw[1] // cell)
    return ch, cw, -(-cw // 32)


def _span(lo, hi, margin):
    c = F(F(lo + hi) * HALF)
    half = F(F(hi - lo) * HALF)
    return c, F(half + F(half * margin))


def _edges(c, half, size):
    """(e0, e1) in pixels, limited to the picture, or None when an edge is not finite."""
    lo, hi = np.floor(F(c - half)), np.ceil(F(c + half))
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return None
    fs = F(size)
    return int(min(max(lo, F(0)), fs)), int(min(max(hi, F(0)), fs))


def person_cells(kp_cell, bbox, src_hw, cell, sy, sx, kp_mask, fallback=FALLBACK_PERSON, margin=0.25, rule=None):
    """Rules 1 to 5 for one person that takes part: ((row0, row1, col0, col1) in cells, both ends included, or None for
    nothing; bad; why) -- `why` names the rule that decided: "ok", "fallback" (ok through FALLBACK_PERSON), "none",
    "box" (a number of a used box is not finite), "edge", "empty" (t >= b or l >= r)."""
    sy, sx, margin = F(sy), F(sx), F(margin)
    K = len(kp_cell)
    chosen = [j for j in range(K) if (kp_mask >> j) & 1 and kp_cell[j] >= 0]
    why = "ok"
    if not chosen:
        if fallback == FALLBACK_NONE:
            return None, False, "none"
        chosen = [j for j in range(K) if kp_cell[j] >= 0]
        why = "fallback"
    b = np.array(bbox[chosen[0]], F)
    fin = bool(np.isfinite(b).all())
    for j in chosen[1:]:
        v = np.array(bbox[j], F)
        fin = fin and bool(np.isfinite(v).all())
        b[0] = v[0] if v[0] < b[0] else b[0]
        b[1] = v[1] if v[1] < b[1] else b[1]
        b[2] = v[2] if v[2] > b[2] else b[2]
        b[3] = v[3] if v[3] > b[3] else b[3]
    if not fin:
        return None, True, "box"
    with np.errstate(all="ignore"):
        cy, hh = _span(F(b[0] * sy), F(b[2] * sy), margin)
        cx, hw = _span(F(b[1] * sx), F(b[3] * sx), margin)
        ey, ex = _edges(cy, hh, src_hw[0]), _edges(cx, hw, src_hw[1])
    if ey is None or ex is None:
        return None, True, "edge"
    (t, bt), (l, r) = ey, ex
    if t >= bt or l >= r:
        return None, False, "empty"
    last = r // cell if rule == "last_col" else (r - 1) // cell
    return (t // cell, (bt - 1) // cell, l // cell, last), False, why


def cells(count, kp_cell, bbox, ttl, streams, frames, src_hw, cell, sy, sx, kp_mask, fallback=FALLBACK_PERSON, margin=0.25,
          hold=0, rule=None):
    """count i32 [S * T], kp_cell i32 [S * T, M, K], bbox f32 [S * T, M, K, 4], ttl u8 [S, CH, CW] (None with hold 0) ->
    (mask u32 [S * T, CH, MW], flags i32 [S * T], ttl' u8 [S, CH, CW] or None).  `ttl` itself is left as it is."""
    assert rule in CELLS_RULES
    B, M, K = kp_cell.shape
    assert B == streams * frames
    CH, CW, MW = grid_of(src_hw, cell)
    mask, flags = np.zeros((B, CH, MW), np.uint32), np.zeros(B, np.int32)
    life = None if hold == 0 else np.array(ttl, np.int32).reshape(streams, CH, CW)
    for s in range(streams):
        for t in range(frames):
            b = s * frames + t
            covered = np.zeros((CH, CW), bool)
            for p in range(min(max(int(count[b]), 0), M)):
                if kp_cell[b, p, 0] < 0:
                    continue
                rect, bad, _ = person_cells(kp_cell[b, p], bbox[b, p], src_hw, cell, sy, sx, kp_mask, fallback, margin, rule)
                if bad:
                    flags[b] |= FLAG_BAD_BOX
                if rect is not None:
                    covered[rect[0]:rect[1] + 1, rect[2]:min(rect[3], CW - 1) + 1] = True     # (the min: rule "last_col" only)
            if hold == 0:
                on = covered
            else:
                reload = hold if rule == "ttl_reload" else hold + 1
                life[s] = np.where(covered, reload, np.maximum(life[s] - 1, 0))
                on = life[s] > 0
            for cy, cx in zip(*np.nonzero(on)):
                mask[b, cy, cx >> 5] |= np.uint32(1 << (cx & 31))
    return mask, flags, None if hold == 0 else life.astype(np.uint8)


def bit(mask_frame, cy, cx):
    return bool(int(mask_frame[cy, cx >> 5]) >> (cx & 31) & 1)


def frame_bytes(fmt, h, w, pitch=None):
    """Bytes of one frame; tests/yuv_ref.frame_bytes with packed BGR added."""
    if fmt == "bgr":
        return h * (3 * w if pitch is None else pitch)
    pitch = (2 * w if fmt == "yuyv" else w) if pitch is None else pitch
    if fmt == "yuyv":
        return h * pitch
    return h * pitch + (h // 2) * pitch if fmt == "nv12" else h * pitch + 2 * (h // 2) * (pitch // 2)


def content_offsets(fmt, h, w, pitch=None):
    """The byte offsets of a frame that hold content (everything but the bytes between a row's content and its pitch)."""
    if fmt == "bgr":
        pitch = 3 * w if pitch is None else pitch
        return (np.arange(h)[:, None] * pitch + np.arange(3 * w)[None, :]).reshape(-1)
    pitch = (2 * w if fmt == "yuyv" else w) if pitch is None else pitch
    if fmt == "yuyv":
        return (np.arange(h)[:, None] * pitch + np.arange(2 * w)[None, :]).reshape(-1)
    luma = (np.arange(h)[:, None] * pitch + np.arange(w)[None, :]).reshape(-1)
    if fmt == "nv12":
        return np.concatenate([luma, h * pitch + (np.arange(h // 2)[:, None] * pitch + np.arange(w)[None, :]).reshape(-1)])
    pc = pitch // 2
    c = (np.arange(h // 2)[:, None] * pc + np.arange(w // 2)[None, :]).reshape(-1)
    return np.concatenate([luma, h * pitch + c, h * pitch + (h // 2) * pc + c])


def sample_sets(fmt, h, w, pitch, cell, cy, cx):
    """The sample sets of cell (cy, cx): a list of (byte offsets into the flat frame, index into `fill`, the number of
    samples the set of a WHOLE cell has)."""
    ys = np.arange(cy * cell, min((cy + 1) * cell, h))
    xs = np.arange(cx * cell, min((cx + 1) * cell, w))
    half = cell // 2
    grid = lambda rows, cols, base, rp, step, off: (base + rows[:, None] * rp + cols[None, :] * step + off).reshape(-1)
    if fmt == "bgr":
        pitch = 3 * w if pitch is None else pitch
        return [(grid(ys, xs, 0, pitch, 3, c), c, cell * cell) for c in range(3)]
    pitch = (2 * w if fmt == "yuyv" else w) if pitch is None else pitch
    js = np.arange(cx * half, min((cx + 1) * half, w // 2))
    if fmt == "yuyv":
        return [(grid(ys, xs, 0, pitch, 2, 0), 0, cell * cell), (grid(ys, js, 0, pitch, 4, 1), 1, cell * half),
                (grid(ys, js, 0, pitch, 4, 3), 2, cell * half)]
    is_ = np.arange(cy * half, min((cy + 1) * half, h // 2))
    out = [(grid(ys, xs, 0, pitch, 1, 0), 0, cell * cell)]
    if fmt == "nv12":
        return out + [(grid(is_, js, h * pitch, pitch, 2, 0), 1, half * half), (grid(is_, js, h * pitch, pitch, 2, 1), 2, half * half)]
    pc = pitch // 2
    return out + [(grid(is_, js, h * pitch, pc, 1, 0), 1, half * half),
                  (grid(is_, js, h * pitch + (h // 2) * pc, pc, 1, 0), 2, half * half)]


def redact(raw, fmt, h, w, mask_frame, cell, mode=MOSAIC, fill=(0, 0, 0), pitch=None, rule=None):
    """One frame (flat u8) and its mask u32 [CH, MW] -> the redacted frame (a new array of raw's size: everything that is
    not a sample of a masked cell keeps its byte).  Bits at and above CW are ignored."""
    assert rule in REDACT_RULES
    out = np.array(raw, np.uint8).reshape(-1)
    src = out.copy()
    CH, CW, _ = grid_of((h, w), cell)
    for cy in range(CH):
        for cx in range(CW):
            if not bit(mask_frame, cy, cx):
                continue
            sets = sample_sets(fmt, h, w, pitch, cell, cy, cx)
            if mode == FILL:
                for idx, which, _ in sets:
                    out[idx] = fill[which]
                continue
            means = []
            for idx, which, whole in sets:
                s, n = int(src[idx].astype(np.int64).sum()), (whole if rule == "full_n" else len(idx))
                means.append(s // n if rule == "trunc" else (s + (n >> 1)) // n)
            if rule == "uv_together" and fmt != "bgr":
                both = np.concatenate([sets[1][0], sets[2][0]])
                s, n = int(src[both].astype(np.int64).sum()), len(both)
                means[1] = means[2] = (s + (n >> 1)) // n
            for (idx, _, _), m in zip(sets, means):
                out[idx] = min(m, 255)
    return out


def redact_frames(raw, fmt, h, w, mask, cell, mode=MOSAIC, fill=(0, 0, 0), pitch=None, rule=None):
    """raw u8 [F, nbytes], mask u32 [F, CH, MW] -> the redacted frames u8 [F, nbytes]."""
    return np.stack([redact(raw[f], fmt, h, w, mask[f], cell, mode, fill, pitch, rule) for f in range(len(raw))])


# the forward colour rule of include/ppn.h (ppn_rgb_to_yuv): rows (matrix, full_range) -> 9 coefficients and yoff
_RGB2YUV = {
    ("bt601", False): (269262, 528618, 102662, -155423, -305128, 460551, 460551, -385654, -74897, 16),
    ("bt709", False): (191455, 644067, 65019, -105533, -355018, 460551, 460551, -418321, -42230, 16),
    ("bt601", True): (313524, 615514, 119538, -176932, -347356, 524288, 524288, -439026, -85262, 0),
    ("bt709", True): (222927, 749942, 75707, -120138, -404150, 524288, 524288, -476214, -48074, 0),
}


def fill_bytes(fmt, rgb, matrix="bt601", full_range=False):
    """The three FILL bytes of a colour: packed BGR takes (b, g, r), the YUV formats the header's forward colour rule."""
    r, g, b = (int(v) for v in rgb)
    if fmt == "bgr":
        return (b, g, r)
    k = _RGB2YUV[(matrix, bool(full_range))]
    sat = lambda v: min(max(v, 0), 255)
    return (sat((k[0] * r + k[1] * g + k[2] * b + (1 << 19) + (k[9] << 20)) >> 20),
            sat((k[3] * r + k[4] * g + k[5] * b + (1 << 19) + (128 << 20)) >> 20),
            sat((k[6] * r + k[7] * g + k[8] * b + (1 << 19) + (128 << 20)) >> 20))
