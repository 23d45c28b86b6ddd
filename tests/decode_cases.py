"""Deterministic edge cases for the decode family (csrc/decode.hip: limb arg-max, root candidates, root-box NMS, greedy
limb parse, ppn_nms) and their expected results.  Plain helper module (no tests): tests/test_decode_edges_cpu.py checks
that the inputs are what they claim, tests/test_decode_edges_gpu.py runs the kernels on them.

    heads = build("g11x13", "ties")                 # f32 [B, 6K + E*sH*sW, H, W], shared: do not modify
    exp = expected("g11x13", "ties")                # per image oracle.decode_ref.decode_ref(...)

Expected results come from oracle.decode_ref alone and are computed once per (case, thresholds); callers must not modify
what they get.  Nothing here needs a GPU; `unary_and_keys` works on whatever device its input lives on.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import decode_ref as D
from pytorch_pose_proposal_network_amd import prng

K, E = D.K, D.E
CELL = 16                                            # pixels per grid cell in both directions (input = grid * 16)

#             grid H, W   window sH, sW
GEOMS = {
    "g11x13": ((11, 13), (7, 11)),
    "g16x16": ((16, 16), (9, 9)),
    "g10x20": ((10, 20), (21, 21)),
    "g26x26": ((26, 26), (5, 5)),
    "g22x32": ((22, 32), (5, 7)),
    "g24x24": ((24, 24), (21, 21)),
}
VARIANTS = ("ties", "iou_edge", "hops", "counts")
FULL_HOPS = ("g11x13", "g16x16")                      # every (cell, s) pair; the others: images 0..6 (see hops_images)
IOU_THRS = (0.5, 0.25)                               # exact in f32
LADDER = (0, 1, 63, 64, 65, 127, 128, 129)           # + ncell - 1, ncell


class Geom:
    def __init__(self, name):
        (self.H, self.W), (self.sH, self.sW) = GEOMS[name]
        self.name = name
        self.ncell, self.S = self.H * self.W, self.sH * self.sW
        self.C = 6 * K + E * self.S
        self.inW, self.inH = self.W * CELL, self.H * CELL
        self.insize = (self.inW, self.inH)           # W first: oracle.decode_ref
        self.insize_hw = (self.inH, self.inW)        # H first: decode.Decoder
        self.local_grid = (self.sW, self.sH)         # W first for both


def geom(name) -> Geom:
    return Geom(name)


def _base(g: Geom, seed: int, quantised=False) -> np.ndarray:
    """Random head: keypoint deltas on both sides of any threshold, boxes up to 0.3 of the frame.  `quantised` limb
    values take four levels only, so every window holds many ties and the first-index rule decides."""
    n = g.ncell
    st = lambda i: prng.stream_seed(seed, i)
    head = np.empty((g.C, g.H, g.W), np.float32)
    head[0:K] = prng.uniform(st(1), K * n, 0.3, 1.0).reshape(K, g.H, g.W)
    head[K:2 * K] = prng.uniform01(st(2), K * n).reshape(K, g.H, g.W)
    head[2 * K:4 * K] = prng.uniform01(st(3), 2 * K * n).reshape(2 * K, g.H, g.W)
    head[4 * K:6 * K] = prng.uniform(st(4), 2 * K * n, 0.02, 0.3).reshape(2 * K, g.H, g.W)
    e = prng.uniform01(st(5), E * g.S * n)
    e = np.floor(e * 4) / np.float32(8) if quantised else e * np.float32(0.5)
    head[6 * K:] = e.astype(np.float32).reshape(E * g.S, g.H, g.W)
    return head


def _set_root(head, resp, conf, x, y, w, h):
    for ch, v in zip((0, K, 2 * K, 3 * K, 4 * K, 5 * K), (resp, conf, x, y, w, h)):
        head[ch] = np.asarray(v, np.float32).reshape(head.shape[1:]) if np.ndim(v) else np.float32(v)


# ----------------------------------------------------------------------------------------------
# ties: root deltas take a handful of exactly representable values
# ----------------------------------------------------------------------------------------------
# (resp, conf) pairs whose f32 product is exact: 1.0, 0.75 (two ways), 0.5 (two ways), and 0.125 (below any threshold)
_LEVELS = ((1.0, 1.0), (1.0, 0.75), (0.75, 1.0), (0.5, 1.0), (1.0, 0.5), (0.25, 0.5))


def _ties_image(g: Geom, mode: int) -> np.ndarray:
    head = _base(g, 1000 + 10 * mode + g.ncell)
    c = np.arange(g.ncell)
    row = c // g.W
    rnd = prng.raw_u64(prng.stream_seed(1100 + mode, g.ncell), 2 * g.ncell) >> np.uint64(33)
    if mode == 0:                                    # three tied levels and some non-candidates
        lv = (rnd[:g.ncell] % np.uint64(6)).astype(np.int64)
    elif mode == 1:                                  # fully tied: every cell a candidate with delta == 1.0
        lv = np.zeros(g.ncell, np.int64)
    else:                                            # two levels, boxes off the cell centres
        lv = (c + row) % 2
    lev = np.asarray(_LEVELS, np.float32)
    # square boxes of 1, 2 or 3 cells (2.5 in mode 2): equal neighbours of side a have IoU (a-1)/(a+1) along a row, so
    # side 2 suppresses its row neighbour at 0.3 and side 1 never does; random sides keep the pattern from being symmetric
    side = np.asarray([1.0, 2.0, 3.0], np.float32)[(rnd[g.ncell:] % np.uint64(3)).astype(np.int64)] if mode < 2 else np.full(g.ncell, 2.5, np.float32)
    x = np.full(g.ncell, 0.5, np.float32) if mode < 2 else np.float32(0.25) * (c % 3).astype(np.float32)
    y = np.full(g.ncell, 0.5, np.float32) if mode < 2 else np.float32(0.25) * (row % 3).astype(np.float32)
    _set_root(head, lev[lv, 0], lev[lv, 1], x, y, side / np.float32(g.W), side / np.float32(g.H))
    return head


# ----------------------------------------------------------------------------------------------
# iou_edge: hand-placed pairs of root boxes
# ----------------------------------------------------------------------------------------------
def _pow2_at_most(size, limit):
    k = 0
    while size / 2 ** k > limit:
        k += 1
    return np.float32(1.0 / 2 ** k)


def _box(g: Geom, r, c, x, y, w, h):
    """oracle.decode_ref.build_bbox for one cell, elementwise on f32 arrays (only used to SEARCH for the one-step-below
    pair; tests/test_decode_edges_cpu.py verifies the result with the oracle itself)."""
    f = np.float32
    x, y, w, h = (np.asarray(v, np.float32) for v in (x, y, w, h))
    rx, ry = (x + f(c)) * f(CELL), (y + f(r)) * f(CELL)
    rw, rh = f(g.inW) * w, f(g.inH) * h
    return ry - rh / f(2), rx - rw / f(2), ry + rh / f(2), rx + rw / f(2)


def _iou(a, b):
    """nms_ref's IoU of box b against the kept box a, elementwise in f32."""
    area = lambda q: (q[2] - q[0]) * (q[3] - q[1])
    tl0, tl1 = np.maximum(b[0], a[0]), np.maximum(b[1], a[1])
    br0, br1 = np.minimum(b[2], a[2]), np.minimum(b[3], a[3])
    inter = ((br0 - tl0) * (br1 - tl1) * ((tl0 < br0) & (tl1 < br1))).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter / ((area(b) + area(a)) - inter)).astype(np.float32)


def _steps(v, k):
    """f32 values k ulps away from v (k an integer array)."""
    return (np.asarray(v, np.float32).view(np.int32) + k.astype(np.int32)).view(np.float32)


@functools.lru_cache(maxsize=None)
def _below_pair(name, thr, r, c):
    """(wA, hA, wB, hB): box A in cell (r, c) with x = 1, box B in cell (r, c + 1) with x = 0 (same centre), B inside
    A, whose IoU in the oracle's f32 arithmetic is the float just below `thr`.  With B inside A the IoU is
    area(B) / area(A); the quotient can only round to the float below thr when area(A) lies in the upper two thirds of
    its binade and area(B) is one unit short of thr * area(A), so A's sides are searched among multiples of 1/64 and
    B's among the floats around the sides that give IoU == thr exactly."""
    g = geom(name)
    k = np.arange(-1024, 1025, 4)
    ki, kj = np.meshgrid(k, k, indexing="ij")
    want = np.nextafter(np.float32(thr), np.float32(0))
    for mw in range(2, 17):
        for mh in range(2, 17):
            wA, hA = np.float32(mw / 64.0), np.float32(mh / 64.0)
            if not (16 <= g.inW * wA <= 48 and 8 <= g.inH * hA <= 28):
                continue
            wB = _steps(wA * np.float32(thr), ki)                 # thr of A's width, (nearly) all of its height
            hB = _steps(hA, -np.abs(kj))
            A, B = _box(g, r, c, 1.0, 0.5, wA, hA), _box(g, r, c + 1, 0.0, 0.5, wB, hB)
            inside = (B[0] >= A[0]) & (B[1] >= A[1]) & (B[2] <= A[2]) & (B[3] <= A[3])
            hit = np.argwhere((_iou(A, B) == want) & inside)
            if len(hit):
                i, j = hit[0]
                return float(wA), float(hA), float(wB[i, j]), float(hB[i, j])
    raise AssertionError(f"no one-step-below pair found for {name} at {thr}")


# pair kinds of the iou_edge images, in placement order; `suppress` is what the NMS must do with the second box
PAIR_KINDS = (("equal", True), ("below", False), ("touch", False), ("zero_same", False), ("zero_inside", False),
              ("line_same", False), ("equal2", True), ("below2", False))


def iou_edge_pairs(name, thr):
    """[(kind, suppress, cellA, cellB)] of the image built for threshold `thr`; A has the higher score."""
    g = geom(name)
    out = []
    for p, (kind, sup) in enumerate(PAIR_KINDS):
        r, c = 1 + 2 * (p // 2), 2 + 6 * (p % 2)
        out.append((kind, sup, r * g.W + c, r * g.W + c + 1))
    return out


def _iou_edge_image(g: Geom, thr: float) -> np.ndarray:
    head = _base(g, 2000 + g.ncell)
    resp = np.full(g.ncell, 0.0625, np.float32)      # no candidates but the placed ones
    conf = np.ones(g.ncell, np.float32)
    x, y = np.full(g.ncell, 0.5, np.float32), np.full(g.ncell, 0.5, np.float32)
    w, h = np.zeros(g.ncell, np.float32), np.zeros(g.ncell, np.float32)
    wA, hA = _pow2_at_most(g.inW, 40), _pow2_at_most(g.inH, 24)
    half = np.float32(0.5)
    for p, (kind, _, a, b) in enumerate(iou_edge_pairs(g.name, thr)):
        resp[a], resp[b] = 1.0 - 2 * p / 64.0, 1.0 - (2 * p + 1) / 64.0          # distinct dyadic scores, A first
        x[a], x[b] = 1.0, 0.0                        # same centre: (1 + c) * 16 == (0 + c + 1) * 16
        w[a], h[a] = wA, hA
        if kind.startswith("equal"):                 # B inside A with half (a quarter) of its area: IoU == thr exactly
            w[b], h[b] = wA * half, hA if thr == 0.5 else hA * half
        elif kind.startswith("below"):
            w[a], h[a], w[b], h[b] = _below_pair(g.name, thr, a // g.W, a % g.W)
        elif kind == "touch":                        # equal boxes one width apart: xmax(A) == xmin(B), all dyadic
            x[a], x[b] = 0.0, np.float32(g.W) * wA - np.float32(1.0)
            w[b], h[b] = wA, hA
        elif kind == "zero_same":                    # two points on the same spot: union 0, IoU = 0/0
            w[a] = h[a] = w[b] = h[b] = 0.0
        elif kind == "zero_inside":                  # a point inside a box: intersection 0, IoU = 0
            w[b] = h[b] = 0.0
        elif kind == "line_same":                    # two coincident horizontal segments: areas 0, IoU = 0/0
            h[a] = h[b] = 0.0
            w[b] = wA
    _set_root(head, resp, conf, x, y, w, h)
    return head


# ----------------------------------------------------------------------------------------------
# hops: every cell a root, the limb arg-max of image i at cell c is s = (i + 7 c + 3 e) % S for edge e
# ----------------------------------------------------------------------------------------------
HOP_THR = 0.15
HOP_DST = D.EDGES[0][1]                              # keypoint 15: the target of edge 0


def hops_images(name):
    """Image numbers of the hops batch.  The two smallest geometries take all S (every (cell, s) pair once); the others
    take images 0..6: s = (i + 7 c) % S then runs through every residue, so every window row and column is visited."""
    g = geom(name)
    return list(range(g.S)) if name in FULL_HOPS else list(range(7))


def hop_s(g: Geom, i, e=0):
    return (i + 7 * np.arange(g.ncell) + 3 * e) % g.S


def hop_kind(g: Geom):
    """Per cell: 0 = the hop target's delta is exactly the threshold (passes), 1 = the float below (fails), 2 = 0.8."""
    c = np.arange(g.ncell)
    return (c + c // g.W) % 3


@functools.lru_cache(maxsize=8)
def _hops_base(name):
    g = geom(name)
    head = _base(g, 3000 + g.ncell, quantised=True)
    c = np.arange(g.ncell)
    resp = ((g.ncell + (c * 37 + 11) % g.ncell) / (2.0 * g.ncell)).astype(np.float32)      # distinct, > 0.5
    _set_root(head, resp, 1.0, 0.5, 0.5, np.float32(4.0 / g.inW), np.float32(4.0 / g.inH))     # 4-pixel boxes: disjoint
    thr = np.float32(HOP_THR)
    tgt = np.asarray([thr, np.nextafter(thr, np.float32(0)), np.float32(0.8)], np.float32)[hop_kind(g)]
    head[HOP_DST] = tgt.reshape(g.H, g.W)
    head[K + HOP_DST] = np.float32(1.0)
    head.setflags(write=False)
    return head


def _hops_image(g: Geom, i: int) -> np.ndarray:
    head = _hops_base(g.name).copy()
    ev = head[6 * K:].reshape(E, g.S, g.ncell)
    c = np.arange(g.ncell)
    for e in range(E):
        ev[e, hop_s(g, i, e), c] = np.float32(0.9)   # above every background level (<= 0.375)
    return head


# ----------------------------------------------------------------------------------------------
# counts: the candidate-count ladder, one image per rung
# ----------------------------------------------------------------------------------------------
def ladder(name):
    n = geom(name).ncell
    return sorted({v for v in LADDER + (n - 1, n) if v <= n})


def _counts_image(g: Geom, idx: int, n: int) -> np.ndarray:
    head = _base(g, 4000 + 16 * idx + g.ncell)
    cells = np.argsort(prng.raw_u64(prng.stream_seed(4100 + idx, g.ncell), g.ncell), kind="stable")[:n]
    resp = np.full(g.ncell, 0.05, np.float32)
    resp[cells] = (0.6 + 0.4 * (np.arange(n) + 1.0) / (n + 1.0)).astype(np.float32)          # distinct scores
    head[0] = resp.reshape(g.H, g.W)
    head[K] = np.float32(1.0)
    # every root finds its first keypoint in its own cell (edge 0 points at the window centre, delta = resp >= 0.3), so
    # an image with candidates always has people; the other sixteen edges stay random
    head[6 * K + (g.sH // 2) * g.sW + g.sW // 2] = np.float32(0.95)
    head[K + D.EDGES[0][1]] = np.float32(1.0)
    return head


# ----------------------------------------------------------------------------------------------
def build(name: str, variant: str, thr: float = 0.5) -> np.ndarray:
    """Head batch f32 [B, C, H, W] of a case (shared: do not modify).  `thr` selects the threshold the iou_edge image is built for."""
    return _build(name, variant, float(thr) if variant == "iou_edge" else 0.5)


@functools.lru_cache(maxsize=3)
def _build(name, variant, thr):
    g = geom(name)
    if variant == "ties":
        heads = [_ties_image(g, m) for m in range(3)]
    elif variant == "iou_edge":
        heads = [_iou_edge_image(g, thr)]
    elif variant == "hops":
        heads = [_hops_image(g, i) for i in hops_images(name)]
    elif variant == "counts":
        heads = [_counts_image(g, i, n) for i, n in enumerate(ladder(name))]
    else:
        raise KeyError(variant)
    return np.stack(heads)


def default_nms_thr(variant, thr=0.5):
    return thr if variant == "iou_edge" else 0.3


def expected(name: str, variant: str, thr: float = 0.5, det_thr: float = 0.15, min_kp: int = 1):
    """Per image oracle.decode_ref.decode_ref of build(name, variant, thr) with nms_thr = 0.3 (iou_edge: thr)."""
    return _expected(name, variant, float(thr) if variant == "iou_edge" else 0.5, float(det_thr), int(min_kp))


@functools.lru_cache(maxsize=None)
def _expected(name, variant, thr, det_thr, min_kp):
    g = geom(name)
    return tuple(D.decode_ref(h, det_thr=det_thr, nms_thr=default_nms_thr(variant, thr), min_kp=min_kp, insize=g.insize,
                              local_grid=g.local_grid) for h in build(name, variant, thr))


def root_boxes(name, head, det_thr=0.15):
    """(bbox f32 [m, 4], score f32 [m], cells) of an image's root candidates in row-major order, from the oracle."""
    g = geom(name)
    delta, x, y, w, h, _ = D.split_head(head, g.local_grid)
    bbox = D.build_bbox(x, y, w, h, g.insize)
    ch, cw = np.where(delta[0] > np.float32(det_thr))
    return bbox[0][ch, cw], delta[0][ch, cw], (ch * g.W + cw).astype(np.int32)


def nms_ref_reversed_ties(bbox, thresh, score):
    """nms_ref with the tie rule reversed: equal scores by DESCENDING index (indices into the given arrays)."""
    n = len(bbox)
    sel = D.nms_ref(bbox[::-1], thresh, score[::-1])
    return (n - 1 - sel).astype(np.int32)


def unary_and_keys(heads, n_edges=E):
    """What the fused head conv leaves for Decoder.decode_fused: the 6K unary channels and one u64 key per (image, edge,
    cell) = value bits << 32 | ~(first arg-max index of the sH x sW window).  Any grid and window; `heads` is a NumPy
    array or a tensor [B, 6K + E*S, H, W] and the result lives on the tensor's device (NumPy: the current GPU)."""
    h = torch.from_numpy(np.ascontiguousarray(heads)).cuda() if isinstance(heads, np.ndarray) else heads
    B = h.shape[0]
    e = h[:, 6 * K:].reshape(B, n_edges, -1, h.shape[2], h.shape[3])
    val, _ = e.max(dim=2)
    first = (e == val.unsqueeze(2)).to(torch.uint8).argmax(dim=2)                      # lowest index among ties
    keys = (val.contiguous().view(torch.int32).to(torch.int64) << 32) | (0xFFFFFFFF - first)
    return h[:, :6 * K].contiguous(), keys.contiguous()


# ----------------------------------------------------------------------------------------------
# stand-alone NMS box sets
# ----------------------------------------------------------------------------------------------
def nms_line_boxes(n: int) -> np.ndarray:
    """n boxes of 10 x 10 along a line, 20 apart (disjoint), except: box i with i % 4 == 1 sits one unit beside box
    i - 1 (IoU 9/11: suppressed by a box of its own 64-chunk), and box i >= 64 with i % 8 == 2 sits two units beside the
    place of box i - 64 (suppressed, if at all, by a box kept in an earlier chunk)."""
    i = np.arange(n)
    xpos = 20.0 * i
    xpos = np.where(i % 4 == 1, 20.0 * (i - 1) + 1.0, xpos)
    xpos = np.where((i >= 64) & (i % 8 == 2), 20.0 * (i - 64) + 2.0, xpos)
    bb = np.stack([np.zeros(n), xpos, np.full(n, 10.0), xpos + 10.0], axis=1)
    return bb.astype(np.float32)


NMS_SCORE_SETS = ("none", "distinct", "equal", "two", "zeros")


def nms_scores(kind: str, n: int):
    i = np.arange(n)
    if kind == "none":
        return None
    if kind == "distinct":
        return prng.uniform(prng.stream_seed(5000, n), n, -1.0, 1.0)
    if kind == "equal":
        return np.full(n, 0.5, np.float32)
    if kind == "two":
        return np.asarray([0.25, 0.75], np.float32)[(i * 3 // 2) % 2]
    if kind == "zeros":                              # signed zeros are equal by value: index order decides among them
        return np.asarray([0.0, -0.0, 0.0, -0.0, 0.5, -0.5, -0.0, 0.0, 0.25, -1.0], np.float32)[i % 10]
    raise KeyError(kind)
