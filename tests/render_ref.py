"""NumPy restatement of the drawing rules of ppn_draw_humans (csrc/render.hip, contract in include/ppn.h): what PIL's
ImageDraw does for the calls of the reference's draw_humans (datatest.py:162-232), as integer raster rules.  Written from
the contract, not from the kernel; tests/test_render_cpu.py pins it against the frames the reference itself drew
(tests/golden/draw_cases.npz) and against the installed Pillow, tests/test_render_gpu.py compares the kernel with it bit
for bit.

Every f32 product / sum below is ONE NumPy f32 operation, in the order the contract writes them."""
import math

import numpy as np

F32 = np.float32
LIMIT = float(2 ** 20)          # a primitive with a non-finite coordinate or |v| >= LIMIT is skipped
GRID_COLOUR = (110, 110, 110)
DISC_STAMPS = {                 # by (bx1 - bx0, by1 - by0); rows top to bottom
    (3, 3): (".##.", "####", "####", ".##."),
    (3, 4): (".##.", "####", "####", "####", ".##."),
    (4, 3): (".###.", "#####", "#####", ".###."),
    (4, 4): (".###.", "#####", "#####", "#####", ".###."),
}


def T(v):
    """Truncation toward zero of an f32."""
    return int(F32(v))


def RU(f):
    f = F32(f)
    return int(math.floor(F32(f + F32(0.5)))) if f >= 0 else -int(math.floor(F32(abs(f) + F32(0.5))))


def RD(f):
    f = F32(f)
    return int(math.ceil(F32(f - F32(0.5)))) if f >= 0 else -int(math.ceil(F32(abs(f) - F32(0.5))))


def usable(box):
    """The out-of-range rule: all four values finite and |v| < 2**20."""
    b = np.asarray(box, np.float64)
    return bool(np.all(np.isfinite(b)) and np.all(np.abs(b) < LIMIT))


def centre(box):
    """f32 midpoints (x, y) of a box (ymin, xmin, ymax, xmax)."""
    ymin, xmin, ymax, xmax = (F32(v) for v in box)
    return F32(F32(xmin + xmax) / F32(2)), F32(F32(ymin + ymax) / F32(2))


def _hline(mask, xa, y, xb):
    H, W = mask.shape
    if 0 <= y < H:
        if xa > xb:
            xa, xb = xb, xa
        xa, xb = max(xa, 0), min(xb, W - 1)
        if xa <= xb:
            mask[y, xa:xb + 1] = True


def rect_mask(H, W, x0, y0, x1, y1):
    """One-pixel outline of [x0, y0, x1, y1]; nothing when x1 < x0 or y1 < y0."""
    m = np.zeros((H, W), bool)
    if x1 < x0 or y1 < y0:
        return m
    _hline(m, x0, y0, x1)
    _hline(m, x0, y1, x1)
    for y in range(max(y0, 0), min(y1, H - 1) + 1):
        _hline(m, x0, y, x0)
        _hline(m, x1, y, x1)
    return m


def disc_mask(H, W, x, y):
    """The disc of a keypoint whose box centre is the f32 pair (x, y)."""
    m = np.zeros((H, W), bool)
    bx0, by0, bx1, by1 = T(F32(x) - F32(2)), T(F32(y) - F32(2)), T(F32(x) + F32(2)), T(F32(y) + F32(2))
    stamp = DISC_STAMPS[(bx1 - bx0, by1 - by0)]
    for j, row in enumerate(stamp):
        for i, ch in enumerate(row):
            if ch == "#" and 0 <= by0 + j < H and 0 <= bx0 + i < W:
                m[by0 + j, bx0 + i] = True
    return m


def quad(x0, y0, x1, y1):
    """The four vertices of the width-2 line (x0, y0) -> (x1, y1), a non-zero vector."""
    dx, dy = x1 - x0, y1 - y0
    hyp = math.hypot(dx, dy)
    dxmax, dymax = _rd64(dy / hyp), _ru64(dx / hyp)
    return [(x0, y0 + dymax), (x1, y1 + dymax), (x1 + dxmax, y1), (x0 + dxmax, y0)]


def _ru64(f):
    return int(math.floor(f + 0.5)) if f >= 0 else -int(math.floor(abs(f) + 0.5))


def _rd64(f):
    return int(math.ceil(f - 0.5)) if f >= 0 else -int(math.ceil(abs(f) - 0.5))


def line_mask(H, W, x0, y0, x1, y1):
    """PIL's width-2 line between integer end points, evaluated in frame coordinates."""
    m = np.zeros((H, W), bool)
    if x0 == x1 and y0 == y1:
        if 0 <= y0 < H and 0 <= x0 < W:
            m[y0, x0] = True
        return m
    V = quad(x0, y0, x1, y1)
    edges, ymin, ymax = [], H - 1, 0
    for i in range(4):
        (ax, ay), (bx, by) = V[i], V[(i + 1) % 4]
        e = dict(xmin=min(ax, bx), xmax=max(ax, bx), ymin=min(ay, by), ymax=max(ay, by), x0=ax, y0=ay)
        ymin, ymax = min(ymin, e["ymin"]), max(ymax, e["ymax"])
        if ay == by:
            _hline(m, e["xmin"], ay, e["xmax"])
            continue
        e["dx"] = F32(F32(bx - ax) / F32(by - ay))
        edges.append(e)
    ymin, ymax = max(ymin, 0), min(ymax, H)
    for y in range(ymin, ymax + 1):
        xs = []
        for e in edges:
            if e["ymin"] <= y <= e["ymax"]:
                xs.append(F32(F32(F32(y - e["y0"]) * e["dx"]) + F32(e["x0"])))
                if y == e["ymax"] and y < ymax:
                    xs.append(xs[-1])
        xs.sort()
        for i in range(1, len(xs), 2):
            _hline(m, RU(xs[i - 1]), y, RD(xs[i]))
    return m


def draw_ref(frames, count, kp_cell, bbox, kp_order, edges, palette, visbbox=False, grid=False, grid_step=16,
             max_humans=None):
    """frames u8 [B,H,W,3], count i[B], kp_cell i[B,M,K], bbox f32[B,M,K,4] (ymin, xmin, ymax, xmax) -> drawn copy."""
    out = np.array(frames, np.uint8, copy=True)
    B, H, W, _ = out.shape
    kp_cell, bbox = np.asarray(kp_cell), np.asarray(bbox, F32)
    M = kp_cell.shape[1] if max_humans is None else int(max_humans)
    pal = np.asarray(palette, np.uint8)
    for b in range(B):
        img = out[b]
        for p in range(min(max(int(count[b]), 0), M)):
            present = [int(kp_cell[b, p, k]) >= 0 for k in range(kp_cell.shape[2])]
            ok = [present[k] and usable(bbox[b, p, k]) for k in range(len(present))]
            for k in kp_order:
                if not ok[k]:
                    continue
                ymin, xmin, ymax, xmax = bbox[b, p, k]
                if k == 0:
                    x0, y0, x1, y1 = T(xmin), T(ymin), T(xmax), T(ymax)
                    img[rect_mask(H, W, x0, y0, x1, y1)] = pal[0]
                    img[rect_mask(H, W, x0 + 1, y0 + 1, x1 - 1, y1 - 1)] = pal[0]
                elif visbbox:
                    img[rect_mask(H, W, T(xmin), T(ymin), T(xmax), T(ymax))] = pal[k]
                else:
                    img[disc_mask(H, W, *centre(bbox[b, p, k]))] = pal[k]
            for s, t in edges:
                if ok[s] and ok[t]:
                    (bx, by), (ex, ey) = centre(bbox[b, p, s]), centre(bbox[b, p, t])
                    img[line_mask(H, W, T(bx), T(by), T(ex), T(ey))] = pal[s]
        if grid:
            img[:, 0:W:grid_step] = GRID_COLOUR
            img[0:H:grid_step, :] = GRID_COLOUR
    return out
