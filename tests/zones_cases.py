"""Builders of zone cases, shared by the CPU and the GPU tests: count / kp_cell / bbox / ids / xy arrays built directly, no
network and no tracker involved (the ids are planted; positive ids are distinct within an image, as the tracker's are).

A case is dict(cfg=zones_ref.make_cfg(..), geom=the tables of zones_ref.make_geom, streams, frames, M, calls=[dict(count,
kp_cell, bbox, ids, xy, n_frames)]): the calls run in order on one Zones.  `run_ref` runs a case through the NumPy
restatement once and keeps the result, so the CPU tests and the GPU tests share one reference per case; it also holds
every state it passes to the invariant entered - exited == slots inside."""
import numpy as np

import zones_ref as R

F = np.float32
SIZE = 100.0                           # the random cases live in [0, 100]^2
SQUARE = [(10, 10), (30, 10), (30, 30), (10, 30)]
DIAMOND = [(20, 10), (30, 20), (20, 30), (10, 20)]
U_SHAPE = [(0, 0), (30, 0), (30, 30), (20, 30), (20, 10), (10, 10), (10, 30), (0, 30)]      # a concave 8-gon, the notch on top
COLLINEAR = [(0, 0), (10, 10), (20, 20)]


def blank(M, K):
    """One image whose every entry is garbage that must not matter: rows claim present roots inside every zone of the
    hand-made cases and positive ids."""
    return dict(count=0, kp_cell=np.full((M, K), 7, np.int32), bbox=np.full((M, K, 4), 20.25, F),
                ids=np.arange(1, M + 1, dtype=np.int32), xy=np.full((M, K, 2), 20.75, F))


def put(img, p, pid, x, y):
    """Person `pid` into row p with its anchor at (x, y) under either anchor rule and with or without xy: the root box is
    (y - 6, x - 3, y, x + 3) for BOTTOM and (y - 3, x - 3, y + 3, x + 3) otherwise -- see `play`."""
    img["ids"][p] = pid
    img["kp_cell"][p, 0] = 100
    lo, hi = (6, 0) if img.get("bottom") else (3, 3)
    img["bbox"][p, 0] = (y - lo, x - 3, y + hi, x + 3)
    img["xy"][p, 0] = (x, y)
    return img


def pack(images, n_frames=None, with_xy=True):
    call = {k: np.stack([np.asarray(img[k]) for img in images]) for k in ("kp_cell", "bbox", "ids", "xy")}
    call["count"] = np.array([img["count"] for img in images], np.int32)
    if not with_xy:
        call["xy"] = None
    call["n_frames"] = None if n_frames is None else np.asarray(n_frames, np.int32)
    return call


def _case(cfg, geom, streams, frames, M, calls):
    return dict(cfg=cfg, geom=geom, streams=streams, frames=frames, M=M, calls=calls)


def play(frames, zones=(), lines=(), M=4, K=2, max_gap=2, anchor=R.ANCHOR_CENTER, loiter=1, with_xy=True):
    """One stream, one frame per call: frames = [[(id, x, y), ..], ..], the people in rows 0, 1, .. of each image."""
    calls = []
    for people in frames:
        img = blank(M, K)
        img["bottom"] = anchor == R.ANCHOR_BOTTOM
        img["count"] = len(people)
        for p, (pid, x, y) in enumerate(people):
            put(img, p, pid, x, y)
        calls.append(pack([img], with_xy=with_xy))
    return _case(R.make_cfg(K, max_gap, anchor, loiter), R.make_geom([list(zones)], [list(lines)]), 1, 1, M, calls)


# ---- hand-checked scenarios: the CPU tests assert their outcome on the restatement, the GPU tests run them through the kernel
LINE = (0, 50, 100, 50)                # A -> B along +x: side(P) is true for P.y >= 50, so a step to larger y is forward


def scenarios():
    one = lambda *steps, **kw: play([[(5, x, y)] if x is not None else [] for x, y in steps], **kw)
    gone = (None, None)
    return {
        "enter_stay_leave": one((5, 20), (20, 20), (22, 20), (40, 20), zones=[SQUARE]),
        "born_inside": one((20, 20), (21, 20), zones=[SQUARE]),
        "freed_inside": one((20, 20), gone, gone, gone, zones=[SQUARE], max_gap=1),
        "dwell_unseen": one((20, 20), gone, gone, (21, 20), zones=[SQUARE], max_gap=2, loiter=3),
        "forward_backward": one((20, 40), (20, 60), (20, 40), lines=[LINE]),
        "across_gap": one((20, 40), gone, gone, (20, 60), lines=[LINE], max_gap=2),
        "two_lines": one((20, 40), (20, 60), lines=[LINE, (0, 55, 100, 55)]),
        "past_the_end": one((120, 40), (120, 60), lines=[LINE]),
        "through_endpoints": play([[(5, 100, 40), (6, 0, 40)], [(5, 100, 60), (6, 0, 60)]], lines=[LINE]),
        "on_the_line": one((20, 40), (20, 50), (20, 60), (20, 50), (20, 40), lines=[LINE]),
        "along_the_line": one((20, 50), (60, 50), (10, 50), lines=[LINE]),
        "zero_length": one((20, 40), (80, 60), (50, 50), (20, 40), lines=[(50, 50, 50, 50)]),
        "bottom_anchor": one((5, 20), (20, 20), (40, 20), zones=[SQUARE], anchor=R.ANCHOR_BOTTOM),
        "box_centres": one((5, 20), (20, 20), (40, 20), zones=[SQUARE], with_xy=False),
    }


KNIFE_ZONES = [SQUARE, SQUARE[::-1], DIAMOND, U_SHAPE, U_SHAPE[::-1], COLLINEAR]
KNIFE_POINTS = [(10, 10), (30, 10), (10, 30), (30, 30),             # the square's vertices
                (20, 10), (20, 30),                                 # on its horizontal edges
                (10, 20), (30, 20),                                 # on its left and its right edge
                (5, 20), (20, 20), (35, 20),                        # the ray runs through the diamond's vertices
                (15, 20), (25, 20), (15, 5), (15, 10),              # the 8-gon: in the notch, in an arm, below, on the notch's edge
                (5, 5), (3, 5), (5, 3)]                             # on and beside the collinear polygon
# by hand, with the rule's half-open edges (left and upper edges belong to a zone, right and lower ones do not)
KNIFE_INSIDE = {
    "square": {(10, 10), (20, 10), (10, 20), (20, 20), (15, 20), (25, 20), (15, 10)},
    "diamond": {(10, 20), (20, 20), (15, 20), (25, 20)},            # the apex (20, 10) and the right vertex are outside
    "u": {(20, 10), (5, 20), (20, 20), (25, 20), (15, 5), (5, 5), (3, 5), (5, 3)},
    "collinear": set(),
}


def knife_edges(with_xy=True, anchor=R.ANCHOR_CENTER):
    """Every knife-edge point as a person of one frame, against every knife-edge polygon as a zone."""
    M = len(KNIFE_POINTS)
    img = blank(M, 1)
    img["bottom"] = anchor == R.ANCHOR_BOTTOM
    img["count"] = M
    for p, (x, y) in enumerate(KNIFE_POINTS):
        put(img, p, p + 1, x, y)
    return _case(R.make_cfg(1, 0, anchor), R.make_geom([KNIFE_ZONES], [[]]), 1, 1, M, [pack([img], with_xy=with_xy)])


def bystanders(with_xy):
    """People that take no part, all with their anchor in the square: a NaN and an infinite anchor, an absent root, ids of
    0 and below (they are counted, but not tracked), rows at and past the count; then counts below 0 and above M."""
    M, K = 8, 2
    img = blank(M, K)
    img["count"] = 6
    for p, pid in enumerate((11, 12, 13, 0, -4, 14, 15, 16)):
        put(img, p, pid, 20, 20)
    img["bbox"][0, 0, 1], img["xy"][0, 0, 0] = np.nan, np.nan
    img["bbox"][1, 0, 2], img["xy"][1, 0, 1] = np.inf, np.inf
    img["kp_cell"][2, 0] = -1
    below, above = dict(img, count=-3), dict(img, count=M + 5)
    return _case(R.make_cfg(K, 0), R.make_geom([[SQUARE]], [[LINE]]), 1, 1, M,
                 [pack([i], with_xy=with_xy) for i in (img, below, above)])


# ---- seeded random cases ----------------------------------------------------------------------------------------------
def random_geom(seed, streams, nz, nl):
    """Per stream nz polygons and nl segments in [0, SIZE]^2.  nz == 1: a large triangle; otherwise 3 and 8 vertices in turn (then
    4..7), star-shaped around a random centre with random radii (so mostly concave), either winding; every other polygon and
    line has whole-numbered coordinates, so that the walkers on the lattice meet vertices and edges.  The lines include a
    horizontal, a vertical and a zero-length one when there are 16."""
    rng = np.random.default_rng(seed)
    zones, lines = [], []
    for s in range(streams):
        zs, ls = [], []
        for z in range(nz):
            nv = 3 if nz == 1 else (3, 8, 4, 8, 5, 3, 6, 7)[z % 8]
            c = rng.uniform(25.0, 75.0, 2)
            ang = np.sort(rng.uniform(0.0, 2 * np.pi, nv))[::(-1 if z % 3 == 1 else 1)]
            if nz == 1:
                ang = 2 * np.pi * np.arange(3) / 3 + rng.uniform(-0.3, 0.3, 3)
            rad = rng.uniform(30.0 if nz == 1 else 8.0, 45.0, nv)
            pts = np.stack([c[0] + rad * np.cos(ang), c[1] + rad * np.sin(ang)], 1)
            zs.append((np.rint(pts) if z % 2 == 0 else pts).astype(F).tolist())
        for l in range(nl):
            seg = rng.uniform(0.0, SIZE, 4)
            if l % 2 == 0:
                seg = np.rint(seg)
            if nl == 16 and l == 3:
                seg[3] = seg[1]
            if nl == 16 and l == 5:
                seg[2] = seg[0]
            if nl == 16 and l == 7:
                seg[2:] = seg[:2]
            ls.append(seg.astype(F).tolist())
        zones.append(zs)
        lines.append(ls)
    return R.make_geom(zones, lines)


def random_image(rng, M, K, count):
    """M random people, none of whom takes part yet: ids of 0 and below in the rows < count, positive ids past them (they must
    not matter).  The root is present with probability 0.9; root boxes are proper boxes of uniform doubles rounded to f32;
    NaN is planted at the absent roots and in a few present ones (such a person is not valid)."""
    here = rng.random((M, K)) < 0.7
    here[:, 0] = rng.random(M) < 0.9
    kp_cell = np.where(here, rng.integers(0, 500, (M, K)), rng.choice((-1, -7, -2 ** 31), (M, K))).astype(np.int32)
    bbox = rng.uniform(0.0, SIZE, (M, K, 4)).astype(F)
    lo = rng.uniform(-10.0, SIZE - 10.0, (M, 2))
    bbox[:, 0] = np.concatenate([lo, lo + rng.uniform(1.0, 40.0, (M, 2))], 1).astype(F)
    xy = rng.uniform(0.0, SIZE, (M, K, 2)).astype(F)
    xy[~here], bbox[~here] = np.nan, np.nan
    bad = rng.random(M) < 0.05
    xy[bad, 0, rng.integers(0, 2)] = rng.choice((np.nan, np.inf, -np.inf))
    bbox[bad, 0, rng.integers(0, 4)] = rng.choice((np.nan, np.inf, -np.inf))
    ids = rng.choice((0, -1, -5), M).astype(np.int32)
    ids[max(count, 0):] = np.arange(1, M + 1)[max(count, 0):]
    return dict(count=count, kp_cell=kp_cell, bbox=bbox, ids=ids, xy=xy)


POOL = (1, 2, 3, 7, 2 ** 31 - 1, 64, 65, 1000, 11, 12, 13, 14)


def video(seed, n, M, K, p_here=0.7):
    """n images of one stream: a random-walk crowd of up to min(M, 12) identities that come and go in runs (gaps both within
    and beyond a small max_gap occur), at random rows among people with ids of 0 and below.  The even identities walk on the
    whole-numbered lattice, the odd ones anywhere; a walker's box centre and its xy differ slightly (the smoothed centre is
    not the raw one).  Counts are small, one image in six lists up to M people."""
    rng = np.random.default_rng(seed)
    pool = POOL[:min(M, len(POOL))]
    on = rng.random(len(pool)) < 0.7
    pos = np.rint(rng.uniform(10.0, SIZE - 10.0, (len(pool), 2)))
    images = []
    for t in range(n):
        on = np.where(rng.random(len(pool)) < 0.35, rng.random(len(pool)) < p_here, on)
        on[0] = True
        step = rng.uniform(-12.0, 12.0, pos.shape)
        step[::2] = np.rint(step[::2])
        pos = np.clip(pos + step, -5.0, SIZE + 5.0)
        here = [i for i, o in enumerate(on) if o]
        rng.shuffle(here)
        top = M if rng.random() < 1 / 6 else min(M, len(here) + 5)
        count = int(rng.integers(len(here), top + 1))
        rows = np.sort(rng.choice(count, len(here), replace=False)).astype(int)
        img = random_image(rng, M, K, count)
        for row, i in zip(rows, here):
            x, y = F(pos[i, 0]), F(pos[i, 1])
            h, w = F(rng.uniform(2.0, 30.0)), F(rng.uniform(2.0, 20.0))
            img["ids"][row], img["kp_cell"][row, 0] = pool[i], 3
            img["bbox"][row, 0] = (y - h, x - w, y + h, x + w) if i % 2 == 0 else (y - h, x - w, y + F(0.7) * h, x + F(1.1) * w)
            img["xy"][row, 0] = (x, y)
        images.append(img)
    return images


def geometry(M, K, nz, nl, anchor=R.ANCHOR_CENTER, with_xy=True, n=8, max_gap=1, loiter=2):
    """Three streams of one frame per call with n_frames (1, 0, -2): a random-walk crowd before nz zones and nl lines."""
    seed = 10000 * M + 100 * K + 10 * nz + nl
    vids = [video(seed + s, n, M, K) for s in range(3)]
    calls = [pack([vids[s][t] for s in range(3)], (1, 0, -2), with_xy) for t in range(n)]
    return _case(R.make_cfg(K, max_gap, anchor, loiter), random_geom(seed, 3, nz, nl), 3, 1, M, calls)


def frames3(M, K=3, anchor=R.ANCHOR_CENTER, with_xy=True, nz=4, nl=4):
    """Three streams of three frames per call, n_frames (3, 0, -1), (2, 3, 1) and (0, 1, 3): frames of one stream in one
    call, images that are not processed, a stream idle in one call and busy in the next; counts below 0 and above M (at
    M = 300 the latter brings 150 ids at once: the slots overflow)."""
    vids = [video(50 + M + s, 9, M, K) for s in range(3)]
    over = vids[1][3]                                               # count > M: every row is listed; the upper half takes part
    over["ids"][M // 2:] = 2000 + np.arange(M // 2, M)              # distinct, and none of the video's
    over["ids"][over["count"]:M // 2] = 3000 + np.arange(over["count"], max(M // 2, over["count"]))   # the rows that were not listed
    over["kp_cell"][M // 2:, 0] = 5
    over["bbox"][M // 2:, 0] = np.nan_to_num(over["bbox"][M // 2:, 0], nan=33.0, posinf=44.0, neginf=22.0)
    over["xy"][M // 2:, 0] = np.nan_to_num(over["xy"][M // 2:, 0], nan=33.0, posinf=44.0, neginf=22.0)
    vids[0][1]["count"], over["count"], vids[2][4]["count"] = -3, M + 100, 0
    nf = ((3, 0, -1), (2, 3, 1), (0, 1, 3))
    calls = [pack([vids[s][3 * c + t] for s in range(3) for t in range(3)], nf[c], with_xy) for c in range(3)]
    return _case(R.make_cfg(K, 1, anchor, 2), random_geom(77 + M, 3, nz, nl), 3, 3, M, calls)


def clamped():
    """Tables as no host would upload them: zone_n and line_n beyond 16 and below 0, vertex numbers below 3, beyond 8 and
    below 0; NaN in every vertex and line that must not be read as geometry.  The kernel clamps, it does not validate."""
    case = geometry(7, 2, 16, 16, n=4)
    g = case["geom"]
    g["zone_n"][:], g["line_n"][:] = (99, 5, -3), (40, -1, 2)
    g["zone_nv"][0] = (3, 8, 2, 0, -5, 9, 1000, 8, 4, 1, 3, 8, 5, 6, 7, 2 ** 31 - 1)
    for z in range(16):
        nv = int(g["zone_nv"][0, z])
        if 0 <= nv < 8:
            g["zone_xy"][0, z, nv:] = np.nan
    case["calls"] = [dict(c, n_frames=np.array((1, 1, 1), np.int32)) for c in case["calls"]]
    return case


# ---- chunking: the same three videos cut three ways -------------------------------------------------------------------
N_CHUNK = 12
CUTS = ((5, 5, 2, 0), (3, 4, 5, 0), (0, 5, 5, 2))                   # per stream the frames it takes of each mixed call


def chunking(M, layout, K=3):
    """`frames`: 12 calls of (1, 1) per video; `triples`: 4 calls of (1, 3); `sequence`: one call of (1, 12) per video;
    `mixed`: four calls of (3, 5) with n_frames = CUTS[.][call], the images past n_frames holding other frames of the video
    (they must not matter).  All three videos share one geometry."""
    vids = [video(900 + M + s, N_CHUNK, M, K) for s in range(3)]
    cfg = R.make_cfg(K, 1, R.ANCHOR_CENTER, 2)
    g3 = random_geom(900 + M, 1, 5, 5)
    one = g3
    three = {k: np.concatenate([v] * 3) for k, v in g3.items()}
    if layout == "frames":
        return [_case(cfg, one, 1, 1, M, [pack([img]) for img in v]) for v in vids]
    if layout == "triples":
        return [_case(cfg, one, 1, 3, M, [pack(v[i:i + 3]) for i in range(0, N_CHUNK, 3)]) for v in vids]
    if layout == "sequence":
        return [_case(cfg, one, 1, N_CHUNK, M, [pack(v)]) for v in vids]
    assert layout == "mixed"
    calls, done = [], [0, 0, 0]
    for c in range(4):
        images = []
        for s in range(3):
            images += [vids[s][(done[s] + t) % N_CHUNK] for t in range(5)]
            done[s] += CUTS[s][c]
        calls.append(pack(images, [CUTS[s][c] for s in range(3)]))
    return [_case(cfg, three, 3, 5, M, calls)]


# ---- running ----------------------------------------------------------------------------------------------------------
_REF = {}


def run_case(case, update, state):
    """Every call of the case: update(call) -> dict(slot, inside, zone, line), state() -> [(outputs, state copy)]."""
    return [(update(c), state()) for c in case["calls"]]


def assert_invariant(st):
    """zone_total's entered - exited == the live slots with the bit, for every stream and zone (rules d and f)."""
    for s in range(st["id"].shape[0]):
        for z in range(R.ZONE_MAX):
            assert int(st["zone_total"][s, z, 0]) - int(st["zone_total"][s, z, 1]) == R.slots_inside(st, s, z), (s, z)


def ref_steps(case, state=None):
    """The restatement's (outputs, state copy) after every call of the case, the invariant checked after each.  `state`: the
    state before the first call (default: fresh)."""
    cfg, S = case["cfg"], case["streams"]
    st = R.fresh_state(S) if state is None else R.copy_state(state)

    def update(c):
        out = R.zone_update(cfg, case["geom"], st, c["count"], c["kp_cell"], c["bbox"], c["ids"], c["xy"], S, case["frames"],
                            c["n_frames"])
        if state is None:
            assert_invariant(st)
        return out

    return run_case(case, update, lambda: R.copy_state(st))


def run_ref(name, case):
    """ref_steps of the case from a fresh state, computed once per `name`."""
    if name not in _REF:
        _REF[name] = ref_steps(case)
    return _REF[name]


LAYOUTS = ("frames", "triples", "sequence", "mixed")


def chunking_views(M, run):
    """Per layout and video: the final state of its stream.  `run(name, case)` gives the steps of a case."""
    views = {}
    for layout in LAYOUTS:
        cases = chunking(M, layout)
        for i in range(3):
            mixed = layout == "mixed"
            steps = run(f"chunk/{layout}/{M}" if mixed else f"chunk/{layout}{i}/{M}", cases[0 if mixed else i])
            views[layout, i] = {k: v[i if mixed else 0] for k, v in steps[-1][1].items()}
    return views


def assert_chunking_invariant(views):
    for i in range(3):
        ref = views["frames", i]
        assert (ref["id"] != 0).any() and ref["zone_total"].any() and ref["line_total"].any() and ref["dwell"].any()
        for layout in LAYOUTS[1:]:
            for k, v in ref.items():
                assert np.asarray(views[layout, i][k]).tobytes() == np.asarray(v).tobytes(), (layout, i, k)
