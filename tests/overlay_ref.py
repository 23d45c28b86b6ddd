"""NumPy restatement of the monitoring overlay (include/ppn.h: ppn_draw_scene, ppn_draw_scene_yuv), test infrastructure only.
Written from the header, not from the kernel.

Lines, outlines, the people under the overlay and the surface rule are tests/render_ref.py's and tests/render_yuv_ref.py's,
imported; this file adds the font, the number formatting, the slot order and the suffix-corrected running totals.  `wrong`
selects deliberately WRONG rules so that a test can show that its cases tell them from the right ones:
    "under"         the overlay painted before the people instead of after them
    "active_first"  `active` beating `alert` in a zone's colour
    "no_flip"       an id label kept above the box when it leaves the frame at the top
    "tick_back"     the tick on the side a backward crossing ends on
    "no_suffix"     a line's label showing the totals after the whole batch on every frame
"""
from __future__ import annotations

import numpy as np

import render_ref as R
import render_yuv_ref as RY

F32 = np.float32
NZ, NV, NL = 16, 8, 16
WRONG = ("under", "active_first", "no_flip", "tick_back", "no_suffix")
KINDS = ("zone_edge", "zone_plate", "zone_text", "line_seg", "line_tick", "line_plate", "line_text", "id_root", "id_plate",
         "id_text")

# seven row bytes per glyph code, bit 4 the leftmost column: the header's table
FONT = (
    (0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E), (0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E),
    (0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F), (0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E),
    (0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02), (0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E),
    (0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E), (0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08),
    (0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E), (0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C),
    (0x00, 0x04, 0x04, 0x00, 0x04, 0x04, 0x00), (0x00, 0x00, 0x00, 0x1F, 0x00, 0x00, 0x00),
    (0x0A, 0x0A, 0x1F, 0x0A, 0x1F, 0x0A, 0x0A), (0,) * 7, (0,) * 7, (0,) * 7,
)
GLYPHS = "0123456789:-# "                     # glyph code = index


def codes_of(text: str):
    return [GLYPHS.index(ch) for ch in text]


def count_text(v: int) -> str:
    """A count: min(max(v, 0), 999999) in decimal, no leading zeros."""
    return str(min(max(int(v), 0), 999999))


def id_text(v: int) -> str:
    """An id in full (positive, at most 10 digits)."""
    return str(int(v))


def wrap32(v: int) -> int:
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def usable(*values) -> bool:
    v = np.asarray(values, np.float64)
    return bool(np.all(np.abs(v) < R.LIMIT))                         # False for NaN


def text_mask(H, W, x0, y0, scale, codes):
    """The glyph coverage rule, pixel by pixel."""
    y, x = np.mgrid[0:H, 0:W]
    u, v, s, n = x - x0, y - y0, int(scale), len(codes)
    ok = (u >= 0) & (v >= 0) & (v < 7 * s)
    u, v = np.where(ok, u, 0), np.where(ok, v, 0)
    c, col = u // (6 * s), (u % (6 * s)) // s
    ok &= (c < n) & (col < 5)
    if n == 0:
        return np.zeros((H, W), bool)
    rows = np.asarray(FONT, np.int64)[np.asarray(codes, np.int64)[np.minimum(c, n - 1)], v // s]
    return ok & ((rows >> (4 - np.minimum(col, 4))) & 1).astype(bool)


def fill_mask(H, W, x0, y0, x1, y1):
    m = np.zeros((H, W), bool)
    xa, xb, ya, yb = max(x0, 0), min(x1, W - 1), max(y0, 0), min(y1, H - 1)
    if xa <= xb and ya <= yb:
        m[ya:yb + 1, xa:xb + 1] = True
    return m


def root_mask(H, W, x0, y0, x1, y1):
    return R.rect_mask(H, W, x0, y0, x1, y1) | R.rect_mask(H, W, x0 + 1, y0 + 1, x1 - 1, y1 - 1)


def running_totals(line_total, out_line, frames, s, t, l, suffix=True):
    """(F, B) of line l as of frame t of stream s: the totals after the batch less the later frames' crossings, wrapping."""
    tot = [int(line_total[s][l][d]) for d in range(2)]
    if suffix:
        for t2 in range(t + 1, frames):
            for d in range(2):
                tot[d] = wrap32(tot[d] - int(out_line[s * frames + t2][l][d]))
    return tot[0], tot[1]


def overlay_prims(b, H, W, M, count, kp_cell, bbox, ov, ids=None, zones=None, n_frames=None, wrong=None):
    """[(slot, kind, mask bool [H,W], colour)] of image b in slot = paint order (empty masks included)."""
    frames, sc, col = int(ov["frames"]), int(ov["scale"]), ov["colours"]
    s, t = divmod(b, frames)
    out = []
    if n_frames is not None and t >= int(n_frames[s]):
        return out

    def label(slot, kind, x0, y0, text):
        n = len(text)
        plate = fill_mask(H, W, x0 - 1, y0 - 1, x0 + 6 * sc * n - sc, y0 + 7 * sc) if ov["plates"] else np.zeros((H, W), bool)
        out.append((slot, kind + "_plate", plate, col["plate"]))
        out.append((slot + 1, kind + "_text", text_mask(H, W, x0, y0, sc, codes_of(text)), col["text"]))

    if zones is not None:
        zone_n = min(max(int(zones["zone_n"][s]), 0), NZ)
        for z in range(zone_n):
            nv = min(max(int(zones["zone_nv"][s][z]), 0), NV)
            xy = np.asarray(zones["zone_xy"][s][z], F32)
            if nv < 3 or not usable(xy[:nv]):
                continue
            oz = zones["out_zone"][b][z]
            first, second = ("alert", 3), ("active", 0)
            if wrong == "active_first":
                first, second = second, first
            c = col[first[0]] if oz[first[1]] > 0 else col[second[0]] if oz[second[1]] > 0 else col["zone"][z]
            for i in range(nv):
                j = (i + 1) % nv
                out.append((10 * z + i, "zone_edge",
                            R.line_mask(H, W, R.T(xy[i][0]), R.T(xy[i][1]), R.T(xy[j][0]), R.T(xy[j][1])), c))
            label(10 * z + 8, "zone", R.T(xy[0][0]) + 3, R.T(xy[0][1]) + 3, count_text(oz[0]))
        line_n = min(max(int(zones["line_n"][s]), 0), NL)
        for l in range(line_n):
            ax, ay, bx, by = (F32(v) for v in zones["line_xy"][s][l])
            if not usable(ax, ay, bx, by):
                continue
            ol = zones["out_line"][b][l]
            c = col["active"] if wrap32(int(ol[0]) + int(ol[1])) > 0 else col["line"][l]
            slot = 160 + 4 * l
            out.append((slot, "line_seg", R.line_mask(H, W, R.T(ax), R.T(ay), R.T(bx), R.T(by)), c))
            dx, dy = F32(bx - ax), F32(by - ay)
            length = np.sqrt(F32(F32(dx * dx) + F32(dy * dy)))
            mx, my = F32(F32(ax + bx) / F32(2)), F32(F32(ay + by) / F32(2))
            if length != 0:
                q = F32(F32(ov["tick"]) / length)
                if wrong == "tick_back":
                    ex, ey = F32(mx + F32(dy * q)), F32(my + F32(F32(-dx) * q))
                else:
                    ex, ey = F32(mx + F32(F32(-dy) * q)), F32(my + F32(dx * q))
                if usable(ex, ey):
                    out.append((slot + 1, "line_tick", R.line_mask(H, W, R.T(mx), R.T(my), R.T(ex), R.T(ey)), c))
            f, bk = running_totals(zones["line_total"], zones["out_line"], frames, s, t, l, suffix=wrong != "no_suffix")
            label(slot + 2, "line", R.T(mx) + 3, R.T(my) + 3, count_text(f) + ":" + count_text(bk))
    if ids is not None:
        for p in range(min(max(int(count[b]), 0), M)):
            i = int(ids[b][p])
            if i <= 0 or int(kp_cell[b, p, 0]) < 0 or not R.usable(bbox[b, p, 0]):
                continue
            ymin, xmin, ymax, xmax = bbox[b, p, 0]
            x0, y0 = R.T(xmin), R.T(ymin)
            slot = 224 + 3 * p
            out.append((slot, "id_root", root_mask(H, W, x0, y0, R.T(xmax), R.T(ymax)), col["id"][i & 15]))
            ty = y0 - 7 * sc - 1
            if ty - 1 < 0 and wrong != "no_flip":
                ty = y0 + 3
            label(slot + 1, "id", x0, ty, id_text(i))
    return sorted(out, key=lambda e: e[0])


def scene_ref(frames, count, kp_cell, bbox, kp_order, edges, palette, visbbox=False, grid=False, grid_step=16, *, overlay,
              ids=None, zones=None, n_frames=None, wrong=None, stats=None, max_humans=None):
    """frames u8 [B,H,W,3] -> the drawn copy: render_ref.draw_ref's people, the overlay, then the grid.  `overlay`:
    dict(frames, scale, tick, plates, colours=dict(zone[16], line[16], id[16], active, alert, text, plate)); `zones`:
    dict(zone_n, zone_nv, zone_xy, line_n, line_xy, out_zone, out_line, line_total) of host arrays; `stats`: a dict that
    receives the number of pixels each primitive kind covers in the frame."""
    assert wrong is None or wrong in WRONG
    frames = np.asarray(frames, np.uint8)
    B, H, W, _ = frames.shape
    M = np.asarray(kp_cell).shape[1] if max_humans is None else int(max_humans)
    assert B % int(overlay["frames"]) == 0

    def lay(img_batch):
        for b in range(B):
            for _, kind, mask, colour in overlay_prims(b, H, W, M, count, np.asarray(kp_cell), np.asarray(bbox, F32), overlay,
                                                       ids, zones, n_frames, wrong):
                img_batch[b][mask] = colour
                if stats is not None:
                    stats[kind] = stats.get(kind, 0) + int(mask.sum())

    if wrong == "under":
        out = frames.copy()
        lay(out)
        out = R.draw_ref(out, count, kp_cell, bbox, kp_order, edges, palette, visbbox, False, 1, max_humans)
    else:
        out = R.draw_ref(frames, count, kp_cell, bbox, kp_order, edges, palette, visbbox, False, 1, max_humans)
        lay(out)
    if grid:
        out[:, :, 0:W:grid_step] = R.GRID_COLOUR
        out[:, 0:H:grid_step, :] = R.GRID_COLOUR
    return out


def painted_scene(B, H, W, *args, **kw):
    """(hit bool [B,H,W], colour u8 [B,H,W,3]): the scene's decision per pixel, as render_yuv_ref.painted finds the people's."""
    lo = scene_ref(np.zeros((B, H, W, 3), np.uint8), *args, **kw)
    hi = scene_ref(np.full((B, H, W, 3), 255, np.uint8), *args, **kw)
    return (lo == hi).all(-1), lo


def scene_rows(src, dst, fmt, H, W, hit, colour, **kw):
    """Raw surfaces [F, nbytes]: render_yuv_ref's surface rule on the scene's decision."""
    return RY.draw_rows(src, dst, fmt, H, W, hit, colour, **kw)
