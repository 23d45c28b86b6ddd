"""Deterministic edge cases for the loss / target kernels (csrc/loss.hip, csrc/encode.hip, ppn_head_grad) and their f64
references.  Plain helper module (no tests): tests/test_loss_edges_cpu.py checks that the inputs are what they claim,
tests/test_loss_edges_gpu.py runs the kernels on them.

    head, targets, insize, outsize, local_grid = build("g35/fit")

A case name is "<geometry>/<head variant>[/b<batch>]".  insize, outsize and local_grid are written W-first.

References are computed once per (case, coefficients) and shared (first_order / second_order below): callers must not
modify what they get.  Every reference exists twice, evaluated by the same oracle in f64 and in f32; the distance between
the two per channel group, `e32`, is the oracle's own f32 rounding on that case and sets the tolerance of the GPU tests
(`tol`).
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from oracle import loss_ref as Lr, targets_ref as T
from pytorch_pose_proposal_network_amd import prng, synth

K, E = Lr.K, Lr.E

#            insize      outsize   window
GEOMS = {
    "g35": ((112, 80), (7, 5), (5, 5)),          # HW = 35: scalar limb kernels, one partial 64-cell block, C = 533 -> cpad 576
    "g135": ((144, 240), (9, 15), (21, 21)),     # HW = 135: scalar, three blocks (last ragged), the real 7605 channels
    "g60": ((96, 160), (6, 10), (21, 21)),       # HW % 4 == 0 but W % 4 != 0: vector loss kernels on scalar-encoded targets
    "g140": ((160, 224), (10, 14), (9, 9)),      # vector path, ragged third block, the reference's default window
    "g30s": ((160, 96), (5, 6), (9, 9)),         # gridW = 32, gridH = 16: the two cell sizes differ
}
VARIANTS = ("plain", "sat", "fit", "edge_ties", "zero_area")
GROUPS = ("resp", "conf", "x", "y", "w", "h", "limb")

COEFFS = {
    "mix": (0.25, 0.15, 0.3, 0.2, 0.1),
    "e0": (1.0, 0.0, 0.0, 0.0, 0.0),
    "e1": (0.0, 1.0, 0.0, 0.0, 0.0),
    "e2": (0.0, 0.0, 1.0, 0.0, 0.0),
    "e3": (0.0, 0.0, 0.0, 1.0, 0.0),
    "e4": (0.0, 0.0, 0.0, 0.0, 1.0),
    "zn": (0.4, 0.0, -0.3, 0.2, 0.5),            # a zero and a negative entry
    "unary": (0.25, 0.15, 0.3, 0.2, 0.0),        # the four unary losses (PPNLoss.unary_backward, dual(unary_only=True))
    "limb": (0.0, 0.0, 0.0, 0.0, -0.37),         # the limb stream of the second-order pass
}

COEFFS = {k: tuple(float(np.float32(c)) for c in v) for k, v in COEFFS.items()}    # the f32 numbers the kernels receive

# every case the GPU tests run: each geometry x {plain, sat}, the two batch variants, g35 / g60 x the three tie cases
CASES = ([f"{g}/{v}" for g in GEOMS for v in ("plain", "sat")] + ["g35/plain/b1", "g35/plain/b5"] +
         [f"{g}/{v}" for g in ("g35", "g60") for v in ("fit", "edge_ties", "zero_area")])

# edge_ties: image 0 holds six people that are a bounding box only (keypoint 0, every joint invisible), each in a cell of
# its own.  Everything is a multiple of 1/64, so that with cells of 16 px and inW / 64, inH / 64 dyadic every box edge is
# exact in f32 and in f64.  A prediction whose width is 2/64 narrower and whose centre is W/64 further right ends at the
# target's right edge: (W/64) * gridW = inW/64 = (2/64) * inW / 2.  `rel` names the relation in unary_kernel's variables
# (a = pred max edge, b = pred min edge, c / d the target's; 1 = horizontal, 2 = vertical).
#   cell (ix, iy), target (tx, ty, tw, th) in 1/64, prediction minus target (dx, dy, dw, dh) in 1/64 with W, H symbolic
TIE_CELLS = (
    ("a1==c1", (1, 1), (32, 32, 20, 20), ("+W", 1, -2, 6)),      # right edges equal only
    ("b1==d1", (3, 1), (32, 32, 20, 20), ("-W", 1, -2, 6)),      # left edges equal only
    ("b2==d2", (5, 1), (32, 32, 20, 20), (1, "-H", 6, -2)),      # top edges equal only
    ("a2==c2", (1, 3), (32, 32, 20, 20), (1, "+H", 6, -2)),      # bottom edges equal only
    ("wr==0", (3, 3), (8, 32, 4, 20), ("touch", 1, 0, 6)),       # the boxes touch: pred's left edge on the target's right edge
    ("wr<0", (5, 3), (4, 32, 4, 20), (46, 1, 0, 6)),             # disjoint
)


def tt(a):
    """NumPy array (possibly read-only) -> a torch CPU tensor of its own."""
    return torch.from_numpy(np.array(a))


def parse(name):
    parts = name.split("/")
    geom, variant = parts[0], parts[1]
    batch = int(parts[2][1:]) if len(parts) > 2 else 2
    assert geom in GEOMS and variant in VARIANTS, name
    return geom, variant, batch


def channels(local_grid):
    return 6 * K + E * local_grid[0] * local_grid[1]


def group_slices(C):
    """[(group name, channel slice)] of a head-layout tensor with C channels."""
    return [(g, slice(i * K, (i + 1) * K)) for i, g in enumerate(GROUPS[:6])] + [("limb", slice(6 * K, C))]


def _seed(geom, variant, batch):
    return 1000 + 97 * list(GEOMS).index(geom) + 13 * VARIANTS.index(variant) + batch


def _stack(per):
    return {k: np.ascontiguousarray(np.stack([p[k] for p in per])) for k in per[0]}


def tie_people(insize, outsize):
    """The six bounding-box-only people of TIE_CELLS."""
    inW, inH = insize
    gW, gH = inW // outsize[0], inH // outsize[1]
    people = []
    for _, (ix, iy), (tx, ty, tw, th), _ in TIE_CELLS:
        bbox = (np.float32((ix + tx / 64) * gW), np.float32((iy + ty / 64) * gH), np.float32(tw / 64 * inW),
                np.float32(th / 64 * inH))
        people.append(dict(bbox=bbox, points=np.zeros((K - 1, 2), np.float32), visible=np.zeros(K - 1, bool),
                           size=np.float32(8.0)))
    return people


def tie_prediction(i, outsize):
    """(x, y, w, h) of the prediction in TIE_CELLS[i]'s cell, exact multiples of 1/64 as f32."""
    W, H = outsize
    _, _, (tx, ty, tw, th), (dx, dy, dw, dh) = TIE_CELLS[i]
    sym = {"+W": W, "-W": -W, "+H": H, "-H": -H}
    w, h = tw + dw, th + dh
    if dx == "touch":                       # rx - rw/2 == rtx + rtw/2  <=>  x - tx = (W/2) (w + tw), in 1/64: W (w + tw) / 2
        dx = W * (w + tw) // 2
        assert (W * (w + tw)) % 2 == 0
    dx, dy = sym.get(dx, dx), sym.get(dy, dy)
    return tuple(np.float32(v / 64) for v in (tx + dx, ty + dy, w, h))


def people_lists(geom, variant, batch):
    insize, outsize, _ = GEOMS[geom]
    seed = _seed(geom, variant, batch)
    lists = [synth.synthetic_people(seed + i, insize=insize) for i in range(batch)]
    if variant == "edge_ties":
        lists[0] = tie_people(insize, outsize)
    return lists


@functools.lru_cache(maxsize=None)
def build(name):
    """-> (head f32 [B, C, H, W], targets dict of f32 arrays, insize, outsize, local_grid).  Read-only."""
    geom, variant, batch = parse(name)
    insize, outsize, local_grid = GEOMS[geom]
    W, H = outsize
    C = channels(local_grid)
    seed = _seed(geom, variant, batch)
    tg = _stack([T.encode_targets(p, insize, outsize, local_grid) for p in people_lists(geom, variant, batch)])
    on = tg["delta"] > 0
    assert on.any(), name
    n = batch * C * H * W
    if variant == "sat":                    # every element exactly 0.0 or 1.0 (what sigmoid gives for |z| of a few tens)
        head = (prng.uniform01(prng.stream_seed(seed, 7), n) < 0.5).astype(np.float32).reshape(batch, C, H, W)
        return _freeze(head, tg, insize, outsize, local_grid)
    head = prng.uniform(prng.stream_seed(seed, 7), n, 0.02, 0.98).reshape(batch, C, H, W)
    if variant == "zero_area":              # target and predicted boxes of zero area on the on-cells: U = eps
        tg["tw"][on] = 0.0
        tg["th"][on] = 0.0
    if variant == "fit":                    # the prediction IS the target: a four-way tie of the box edges
        pull = ((2, "tx", 1.0, 0.0), (3, "ty", 1.0, 0.0), (4, "tw", 1.0, 0.0), (5, "th", 1.0, 0.0))
    else:                                   # overlapping but different boxes, as tests/test_loss_gpu.py::_case
        pull = ((2, "tx", 0.9, 0.03), (3, "ty", 0.95, 0.02), (4, "tw", 1.2, 0.01), (5, "th", 0.8, 0.01))
    for g, key, a, b in pull:
        head[:, g * K:(g + 1) * K][on] = (tg[key][on] * np.float32(a) + np.float32(b)).astype(np.float32)
    if variant == "zero_area":
        head[:, 4 * K:5 * K][on] = 0.0
        head[:, 5 * K:6 * K][on] = 0.0
    if variant == "edge_ties":
        for i, (_, (ix, iy), _, _) in enumerate(TIE_CELLS):
            assert tg["delta"][0, 0, iy, ix] == 1.0
            for g, v in zip((2, 3, 4, 5), tie_prediction(i, outsize)):
                head[0, g * K, iy, ix] = v
    return _freeze(head, tg, insize, outsize, local_grid)


def _freeze(head, tg, *rest):
    head = np.ascontiguousarray(head, np.float32)
    head.setflags(write=False)
    for v in tg.values():
        v.setflags(write=False)
    return (head, tg) + rest


def tangent(name):
    """Logit tangent of the second-order passes: f32 like head, uniform in (-1, 1)."""
    head = build(name)[0]
    geom, variant, batch = parse(name)
    return prng.uniform(prng.stream_seed(_seed(geom, variant, batch), 8), head.size, -1.0, 1.0).reshape(head.shape)


def iou_edges(name, dtype):
    """unary_kernel's a1, c1, b1, d1, a2, c2, b2, d2 and wr, hr (oracle/loss_ref.py::_iou's formulas) for every
    (image, keypoint, cell), as torch tensors of `dtype`."""
    head, tg, insize, outsize, _ = build(name)
    (inW, inH), (W, H) = insize, outsize
    gW, gH = int(inW / W), int(inH / H)
    fm = tt(head).to(dtype)
    t = {k: tt(v).to(dtype) for k, v in tg.items()}
    x, y, w, h = (fm[:, i * K:(i + 1) * K] for i in (2, 3, 4, 5))
    X, Y = torch.meshgrid(torch.arange(W, dtype=dtype), torch.arange(H, dtype=dtype), indexing="xy")
    rx, ry, rw, rh = (x + X) * gW, (y + Y) * gH, inW * w, inH * h
    rtx, rty, rtw, rth = (t["tx"] + X) * gW, (t["ty"] + Y) * gH, inW * t["tw"], inH * t["th"]
    e = dict(a1=rx + rw / 2, c1=rtx + rtw / 2, b1=rx - rw / 2, d1=rtx - rtw / 2,
             a2=ry + rh / 2, c2=rty + rth / 2, b2=ry - rh / 2, d2=rty - rth / 2)
    e["wr"] = torch.min(e["a1"], e["c1"]) - torch.max(e["b1"], e["d1"])
    e["hr"] = torch.min(e["a2"], e["c2"]) - torch.max(e["b2"], e["d2"])
    return e


# ---- references -----------------------------------------------------------------------------------------------------------
def _oracle_first(name, coeff, dtype):
    head, tg, insize, _, local_grid = build(name)
    fm = tt(head).to(dtype).requires_grad_(True)
    t = {k: tt(v).to(dtype) for k, v in tg.items()}
    losses = Lr.ppn_loss_ref(fm, t, insize=insize, local_grid=local_grid)
    total = sum(float(c) * l for c, l in zip(coeff, losses))
    total.backward()
    return np.array([float(l.detach()) for l in losses], np.float64), fm.grad.numpy()


def group_e32(a32, a64, C):
    """{group: max|a32 - a64|} of two [B, C', ...] arrays (C' = C, or 6K for a compact tensor: no limb group)."""
    return {g: float(np.abs(a32[:, sl].astype(np.float64) - a64[:, sl]).max()) for g, sl in group_slices(C)
            if a64[:, sl].size}


@functools.lru_cache(maxsize=None)
def first_order(name, ckey):
    """Losses and d(sum_i coeff_i L_i)/d(head) of the oracle in f64 and f32, and what follows from them for the fused
    kernels: dz = grad * s (1 - s) and its per-channel sums.  dict:
      l64, l32 [5]; e32_loss [5]; g64 [B, C, H, W]; finite32 (is the f32 gradient finite); e32 {group: max|g32 - g64|};
      e32_dz {group} (of dz64(r) below); db64 [C], e32_db {group}."""
    coeff = COEFFS[ckey]
    head = build(name)[0]
    C = head.shape[1]
    l64, g64 = _oracle_first(name, coeff, torch.float64)
    l32, g32 = _oracle_first(name, coeff, torch.float32)
    s64 = head.astype(np.float64)
    dz64 = g64 * (s64 * (1.0 - s64))
    dz32 = g32 * (head * (np.float32(1.0) - head))
    db64, db32 = dz64.sum((0, 2, 3)), dz32.sum((0, 2, 3), dtype=np.float32)
    r = dict(l64=l64, l32=l32, e32_loss=np.abs(l32 - l64), g64=g64, finite32=bool(np.isfinite(g32).all()),
             e32=group_e32(g32, g64, C), e32_dz=group_e32(dz32, dz64, C), db64=db64,
             e32_db=group_e32(db32[None, :, None, None], db64[None, :, None, None], C))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def dz64(name, ckey):
    """grad * s (1 - s) in f64, head layout: what ppn_head_grad / forward_backward_dz write (as NHWC)."""
    s = build(name)[0].astype(np.float64)
    return first_order(name, ckey)["g64"] * (s * (1.0 - s))


def _oracle_second(name, coeff, dtype):
    """(zbar, tzbar) = d/d(z, tz) of F = <d(sum c_i L_i)/ds, sig'(z) tz>, as tests/test_second_order_gpu.py builds it, but
    with the head s itself as the leaf (ds/dz = s (1 - s) applied by hand) so that the kernel and the reference see the
    same s bit for bit -- a saturated head has no finite logit."""
    head, tg, insize, _, local_grid = build(name)
    s = tt(head).to(dtype).requires_grad_(True)
    tz = tt(tangent(name)).to(dtype)
    t = {k: tt(v).to(dtype) for k, v in tg.items()}
    losses = Lr.ppn_loss_ref(s, t, insize=insize, local_grid=local_grid)
    total = sum(float(c) * l for c, l in zip(coeff, losses))
    gs, = torch.autograd.grad(total, s, create_graph=True)
    s1 = s * (1 - s)
    Fv = (gs * (s1 * tz)).sum()
    dF_ds, = torch.autograd.grad(Fv, s)
    return (dF_ds * s1).detach().numpy(), (gs * s1).detach().numpy()


@functools.lru_cache(maxsize=None)
def second_order(name, ckey):
    """dict: zbar64, tzbar64 [B, C, H, W] (f64 double backward), e32_zbar, e32_tzbar {group}; zsum64 [C] (per-channel
    sums of zbar64), e32_zsum {group}."""
    coeff = COEFFS[ckey]
    C = build(name)[0].shape[1]
    z64, t64 = _oracle_second(name, coeff, torch.float64)
    z32, t32 = _oracle_second(name, coeff, torch.float32)
    zs64, zs32 = z64.sum((0, 2, 3)), z32.sum((0, 2, 3), dtype=np.float32)
    r = dict(zbar64=z64, tzbar64=t64, e32_zbar=group_e32(z32, z64, C), e32_tzbar=group_e32(t32, t64, C), zsum64=zs64,
             e32_zsum=group_e32(zs32[None, :, None, None], zs64[None, :, None, None], C))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


# ---- the one tolerance rule -----------------------------------------------------------------------------------------------
def tol(scale, e32):
    """err <= max(2e-5 * scale, 4 * e32): 2e-5 is tests/test_loss_gpu.py's figure, e32 the reference's own f32 rounding on
    the case, 4 covers the kernel's other operation order and FMA contraction."""
    return max(2e-5 * scale, 4.0 * e32)


def check_groups(tag, got, ref64, e32, lines=None):
    """Per channel group: max|got - ref64| <= tol(max|ref64|, e32[group]).  got, ref64: [B, C, ...] arrays in the head
    layout.  Prints err / e32 per group; returns the list of failures (empty: pass)."""
    C = ref64.shape[1]
    bad, parts = [], []
    for g, sl in group_slices(C):
        r = ref64[:, sl]
        if r.size == 0:                     # a compact [B, 6K, ...] tensor has no limb channels
            continue
        d = got[:, sl].astype(np.float64) - r
        if not np.isfinite(d).all():
            bad.append(f"{tag} {g}: non-finite")
            continue
        err, scale = float(np.abs(d).max()), float(np.abs(r).max())
        ratio = err / e32[g] if e32[g] > 0 else (0.0 if err == 0 else float("inf"))
        parts.append(f"{g} {ratio:.2f}")
        if err > tol(scale, e32[g]):
            bad.append(f"{tag} {g}: err {err:.3e} > max(2e-5 * {scale:.3e}, 4 * {e32[g]:.3e}); err/e32 {ratio:.2f}")
    line = f"LOSS_EDGE {tag}: err/e32 " + ", ".join(parts)
    print(line)
    if lines is not None:
        lines.append(line)
    return bad
