"""Shared inputs of tests/test_overlay_cpu.py and tests/test_overlay_gpu.py: scenes for the monitoring overlay (include/ppn.h:
ppn_draw_scene).  A case is a dict: name, H, W, frames (per stream), people = (count, kp_cell, bbox), ids i32 [B,M] or None,
zones (the tables and results of overlay_ref.scene_ref) or None, n_frames or None, overlay (scene_ref's dict), visbbox,
grid_step, claims (the primitive kinds the case must paint) and tells (the wrong rules of overlay_ref.WRONG it exposes)."""
import numpy as np

import render_cases as RC
import render_yuv_cases as YC

K = RC.K
NZ, NV, NL = 16, 8, 16
ZONE_KINDS = {"zone_edge", "zone_plate", "zone_text"}
LINE_KINDS = {"line_seg", "line_tick", "line_plate", "line_text"}
ID_KINDS = {"id_root", "id_plate", "id_text"}

# colours that are neither a palette colour, the grid's grey nor a value of RC.gradient (whose channels stay below 100)
COLOURS = dict(zone=[(120 + 5 * z, 200, 130 + 3 * z) for z in range(16)], line=[(200, 120 + 4 * l, 240 - 2 * l) for l in range(16)],
               id=[(140 + 6 * i, 101 + 9 * i, 250 - 7 * i) for i in range(16)], active=(1, 254, 2), alert=(253, 3, 4),
               text=(251, 252, 249), plate=(5, 6, 7))


def overlay(frames=1, scale=1, tick=6.0, plates=True):
    return dict(frames=frames, scale=scale, tick=tick, plates=plates, colours=COLOURS)


def tables(S, B, zones=(), lines=()):
    """Geometry of S streams (`zones`: per stream a list of polygons, `lines`: per stream a list of (ax, ay, bx, by)) and
    all-zero results of B images."""
    g = dict(zone_n=np.zeros(S, np.int32), zone_nv=np.zeros((S, NZ), np.int32), zone_xy=np.zeros((S, NZ, NV, 2), np.float32),
             line_n=np.zeros(S, np.int32), line_xy=np.zeros((S, NL, 4), np.float32), out_zone=np.zeros((B, NZ, 4), np.int32),
             out_line=np.zeros((B, NL, 2), np.int32), line_total=np.zeros((S, NL, 2), np.int32))
    for s, polys in enumerate(zones):
        g["zone_n"][s] = len(polys)
        for z, poly in enumerate(polys):
            g["zone_nv"][s, z] = len(poly)
            g["zone_xy"][s, z, :len(poly)] = np.asarray(poly, np.float32)
    for s, segs in enumerate(lines):
        g["line_n"][s] = len(segs)
        g["line_xy"][s, :len(segs)] = np.asarray(segs, np.float32).reshape(-1, 4)
    return g


def person(x0, y0, x1, y1, extra=()):
    """A person whose root outline is the pixel box [x0, y0, x1, y1]; `extra`: {keypoint: box}."""
    p = {0: YC.span(x0, y0, x1, y1)}
    p.update(extra)
    return p


def pack(images, M=None):
    """[[person dict] per image] -> (count [B], kp_cell [B,M,K], bbox [B,M,K,4])."""
    M = max(max(len(p) for p in images), 1) if M is None else M
    parts = [YC.pack_people(p, M) for p in images]
    return tuple(np.concatenate([q[i] for q in parts]) for i in range(3))


def case(name, H, W, images, ids=None, zones=None, frames=1, n_frames=None, ov=None, visbbox=False, grid_step=0, claims=(),
         tells=()):
    people = pack(images) if isinstance(images, list) else images
    return dict(name=name, H=H, W=W, frames=frames, people=people, ids=None if ids is None else np.asarray(ids, np.int32),
                zones=zones, n_frames=n_frames, overlay=overlay(frames) if ov is None else ov, visbbox=visbbox,
                grid_step=grid_step, claims=set(claims), tells=set(tells))


def scene(H, W, n_zones, n_lines, nv, scale, seed, B=2, M=4):
    """A random scene on an H x W frame: polygons and lines all over (and beyond) the frame, random results, tracked people
    over every border; stream s = image s."""
    rng = np.random.default_rng(seed)
    pt = lambda: (rng.uniform(-6, W + 6), rng.uniform(-6, H + 6))
    g = tables(B, B, [[[pt() for _ in range(nv)] for _ in range(n_zones)] for _ in range(B)],
               [[pt() + pt() for _ in range(n_lines)] for _ in range(B)])
    g["out_zone"][:, :n_zones] = rng.integers(0, 3, (B, n_zones, 4)) * rng.integers(0, 2, (B, n_zones, 4))
    g["out_line"][:, :n_lines] = rng.integers(0, 2, (B, n_lines, 2))
    g["line_total"][:, :n_lines] = rng.choice([0, 7, 42, 999999, 1200000, 123456], (B, n_lines, 2))
    people = RC.people(rng, B, M, H, W, garbage=True)
    ids = rng.choice([-1, 0, 1, 5, 16, 17, 300, 2 ** 31 - 1], (B, M)).astype(np.int32)
    ids[:, 0] = [3 + b for b in range(B)]
    return case(f"scene {n_zones}z {n_lines}l nv{nv} s{scale}", H, W, people, ids, g, ov=overlay(1, scale),
                visbbox=bool(seed & 1), grid_step=7 if seed & 2 else 0)


def knife_edges():
    """Hand-placed cases on a 40 x 64 frame (24 x 40 and 8 x 40 where noted)."""
    H, W = 40, 64
    cases = []
    # y0 = T(ymin) - 7 s - 1: T(ymin) = 9 gives y0 - 1 == 0 (stays above), T(ymin) = 8 gives -1 (moves inside)
    cases.append(case("label at the top border", H, W, [[person(4, 9, 20, 30), person(34, 8, 50, 30)]], [[7, 8]],
                      claims=ID_KINDS, tells={"no_flip", "under"}))
    big = tables(1, 1, [[[(10, 5), (float(2 ** 20), 8), (20, 30)], [(30, 5), (float(2 ** 20 - 1), 8), (40, 30)],
                         [(3, 3), (np.nan, 9), (9, 9)]]])
    cases.append(case("zone vertex at 2^20", H, W, [[]], None, big, claims={"zone_edge", "zone_text"}))
    zero = tables(1, 1, lines=[[(12.5, 9.5, 12.5, 9.5), (30.2, 20.1, 30.7, 20.6), (50, 30, 40, 12)]])
    cases.append(case("zero-length line", H, W, [[]], None, zero, claims=LINE_KINDS, tells={"tick_back"}))
    gon = [(4, 4), (30, 8), (56, 4), (48, 20), (58, 36), (30, 28), (6, 36), (14, 20)]
    conc = tables(1, 1, [[gon]])
    conc["out_zone"][0, 0] = (2, 1, 0, 0)
    cases.append(case("concave 8-gon", H, W, [[person(20, 12, 40, 26, {3: RC.box(8, 8, 4, 4), 4: RC.box(50, 30, 4, 4)})]], None,
                      conc, claims=ZONE_KINDS))
    four = [[person(2, 10, 12, 30), person(16, 10, 26, 30), person(30, 10, 40, 30), person(44, 10, 62, 30)]]
    cases.append(case("ids 1, 16, 17 and 2^31 - 1", H, W, four, [[1, 16, 17, 2 ** 31 - 1]], claims=ID_KINDS, tells={"under"}))
    # one tile (8 rows x 40 columns): 16 zones x 10 + 16 lines x 4 + 16 people x 3 = 272 overlay slots behind 560 people's
    rng = np.random.default_rng(5)
    h, w = 8, 40
    pt = lambda: (rng.uniform(0, w - 1), rng.uniform(0, h - 1))
    full = tables(1, 1, [[[pt() for _ in range(8)] for _ in range(16)]], [[pt() + pt() for _ in range(16)]])
    full["out_zone"][0, :, 0] = rng.integers(0, 3, 16)
    full["out_zone"][0, :, 3] = rng.integers(0, 2, 16)
    full["out_line"][0] = rng.integers(0, 2, (16, 2))
    full["line_total"][0] = rng.integers(0, 50, (16, 2))
    crowd = RC.people(rng, 1, 16, h, w, spread=(20.0, 4.0, 3.5), missing=0.0)
    cases.append(case("more than 256 overlay primitives on a tile", h, w, crowd, [list(range(1, 17))], full, ov=overlay(1, 1, 3.0),
                      claims=ZONE_KINDS | LINE_KINDS | ID_KINDS, tells={"under"}))
    return cases


def reactive():
    """Zone 0 idle, 1 occupied, 2 occupied with a loiterer, 3 loitering only; line 0 idle, 1 crossed forward, 2 backward;
    image 1 of the two (one stream each) is cut out by n_frames."""
    H, W = 40, 64
    polys = [[(2 + 15 * z, 3), (13 + 15 * z, 3), (13 + 15 * z, 16), (2 + 15 * z, 16)] for z in range(4)]
    segs = [(4 + 20 * l, 22, 4 + 20 * l, 38) for l in range(3)]
    g = tables(2, 2, [polys, polys], [segs, segs])
    for b in range(2):
        g["out_zone"][b, :4] = [(0, 0, 1, 0), (2, 1, 0, 0), (1, 0, 0, 1), (0, 0, 0, 3)]
        g["out_line"][b, :3] = [(0, 0), (1, 0), (0, 2)]
    g["line_total"][:, :3] = [(5, 6), (10, 0), (999999, 1000000)]
    both = case("reactive colours", H, W, [[person(40, 20, 60, 36)], [person(40, 20, 60, 36)]], [[4], [5]], g,
                claims=ZONE_KINDS | LINE_KINDS | ID_KINDS, tells={"active_first", "tick_back", "under"})
    cut = dict(both, name="n_frames cuts image 1 out", n_frames=np.array([1, 0], np.int32))
    return [both, cut]


def running():
    """One stream of three frames; line 0 is crossed forward in frame 0 and backward twice in frame 2: the labels read
    1:0, 1:0, 1:2 on top of 10:20 from before the batch."""
    H, W = 24, 64
    g = tables(1, 3, lines=[[(6, 4, 50, 4)]])
    g["out_line"][0, 0], g["out_line"][2, 0] = (1, 0), (0, 2)
    g["line_total"][0, 0] = (11, 22)
    return case("running totals", H, W, [[], [], []], None, g, frames=3, claims=LINE_KINDS, tells={"no_suffix", "tick_back"})


def all_cases():
    return knife_edges() + reactive() + [running()]
