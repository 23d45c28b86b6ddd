"""Edge cases for the two arg-max code paths every fused-decode plan ends in -- the edge-aligned limb kernel of csrc/conv_head.hip
(ppn_conv_desc.limb_edge_pad) and the atomic-key epilogue of csrc/conv_big.hip (ppn_conv_desc.argmax_keys alone) -- their f64
reference and a checker for a key that does NOT rest on the other kernel.  Plain helper module (no tests):
tests/test_head_edges_cpu.py checks that the cases are what they claim and that the checker sees planted faults,
tests/test_head_edges_gpu.py runs the kernels on them.

A case is a Head (below): a 1x1 convolution x [B, K, H, W] -> uch + E * win channels, bias, sigmoid; the limb channels form E
windows of win values per pixel.  A key is (f32 value bits << 32) | ~k with k the FIRST index of the window that attains the
largest sigmoid VALUE (np.argmax of the materialised head).

Reference (reference()): operands ALREADY ROUNDED to the storage type; logits t = x . w + b in f64; S = |x| . |w|;
    A = (K + 4) u (S + |b|),   u = 2^-24
is the A term of tests/forward_cases.py (f32 products and accumulation in any order, the shift) and bounds |t^ - t| for the f32
logit t^ a kernel holds.

sigmoid_fast (csrc/conv_common.h:37-39) is  rcp(1.0f + __expf(-v)),  __expf(y) = v_exp_f32(y * log2(e)).  Its relative error at
the f32 logit v, term by term:
    (a) the product y * log2(e) is rounded and so is the constant (conv_common.h:39, __expf): the exponent is off by 2 u |v| log2(e)
        at most, which is a relative error 2 u |v| of e^-v;
    (b) v_exp_f32, 1 ulp (conv_common.h:37): 2 u;
    (c) 1.0f + e is rounded once (conv_common.h:39): u; the error of e enters the sum with the weight e / (1 + e) = 1 - sigmoid(v);
    (d) v_rcp_f32, 1 ulp (conv_common.h:37): 2 u.
    E_rel(v) = u (3 + (1 - sigmoid(v)) (2 |v| + 2))
(1 - sigmoid(v)) (2 |v| + 2) is below 1.14 for v >= 0, below 4 on [-1, 0) and below 2 |v| + 2 for v < 0.  Two logits v' < v whose
computed sigmoids tie or swap are less than 1 apart (sigmoid(v - 1) <= 0.74 sigmoid(v) for v <= 0, and v' > -1 for v >= 0), hence
    e_rel(m) = u (7 + 2 max(0, -m)) (1 + 2^-10)      covers E_rel at every logit that can compete with a maximum m, and the
                                                     second-order products of (a)-(d)
    E_sig(t) = sigmoid(t) e_rel(t)                   the evaluation term of a VALUE
    D(m)     = 2 e_rel(m) (1 + e^(m + A[s*]))        the width of the logit interval below a maximum m whose sigmoids can round
                                                     to the same or a swapped f32: computed sigmoids s(1 + eps), |eps| <= e_rel,
                                                     tie or swap only when ln sigmoid(v) - ln sigmoid(v') <= 2 e_rel, and
                                                     d/dv ln sigmoid(v) = 1 - sigmoid(v) >= 1 / (1 + e^(m + A[s*])) below m^
A bound is widened only by a named term for a rounding step the source shows, with the line cited; never to fit what a kernel
returned (the rule of tests/forward_cases.py).

Checker (check()) for the key (value, k) of one window, s* the first f64 maximum:
    index range       0 <= k < win, always
    near-maximal      t[k] >= t[s*] - A[k] - A[s*] - D(t[s*])
    decided windows   where t[s*] - t[s] > A[s*] + A[s] + D(t[s*]) for every other s:  k == s*.  At most UNDECIDED_CAP of the windows
                      of a random case may be left undecided -- a condition on the case, asserted, not a measurement
    value             |value - sigmoid64(t[k])| <= sigmoid'(t[k]) A[k] (1 + A[k]) + E_sig(t[k]) + tiny      (1 + A[k]: the Taylor
                      remainder, |sigmoid''| <= sigmoid'); the worst err / bound is the ratio of a case, <= 1

Exact cases (kind "ties", "saturated"): x in {-2 .. 2}, weights small integers, biases multiples of 1/4 and S + |b| <= 2^21, so
every partial sum in any order is a multiple of 1/4 below 2^22 and exact in f32 (exact_condition()); the f64 logits ARE the
kernels' logits.  Channel 0 of x is a flag, 1 everywhere but at the `ambiguous` pixels (and 0, like every input, in the rows a
pixel tile has past M):
    ties       three rows of every window share their weights but for the flag's: where the flag is 1 the MIDDLE one leads by 1,
               where it is 0 the three logits are equal and the lowest index must win; every other logit lies >= 2 below, and all lie
               below 14
    saturated  three rows have logits >= 20 (1 + exp(-20) rounds to 1.0f: value bits 0x3F800000, whatever their order as logits),
               the first of them only where the flag is 0; the rest are <= 10.  The lowest saturated index must win.
No logit lies in the band 14 .. 19, where the outcome would depend on the device's sigmoid.  expected_exact() gives the index,
and for `saturated` the value bits: there the key equals the reference bit for bit.  For `ties` the value is sigmoid_fast of an
unsaturated logit, which the source specifies to its accuracy only: index bit for bit, value within E_sig.
"""
from __future__ import annotations

import collections
import functools

import numpy as np
import torch

from forward_cases import DTYPE_NAMES, TINY, U, q  # noqa: F401  (DTYPE_NAMES: re-exported to the tests)

# pad: what the rows of an edge's 448-row tile past the window hold (edge path only): "hostile" bias 1000 (a pad row that competed
# would win every window), "zero" weights and bias 0 as model.py:260-266 packs them.  kind: "random", "negative" (random with the
# biases lowered by NEGATIVE_SHIFT: every limb score below 0.5, so that a zero pad row that competed would win), "ties",
# "saturated".  ksteps: the GEMM depth in K steps (32 values in f32, 64 in the 16-bit types) or 0: K = `K` in every type.
Head = collections.namedtuple("Head", "B H W K ksteps E win uch kind pad bias ranges paths")
Head.__new__.__defaults__ = (True, None, ("edge",))

BP, EDGE_PAD = 128, 448                       # kEdgeTileBP / kEdgeTileBC of csrc/conv_args.h
UNDECIDED_CAP = 0.01
NEGATIVE_SHIFT = 8.0
SAT_BITS = 0x3F800000
GARBAGE = 0x7EADBEEF7EADBEEF
EDGE_WINDOWS = (385, 420, 431, 432, 433, 441, 447, 448)
SMALL_WINDOWS = (1, 25, 81)


def _h(B, H, W, E=2, win=441, K=128, ksteps=0, uch=0, kind="random", pad="hostile", **kw):
    return Head(B, H, W, K, ksteps, E, win, uch, kind, pad, **kw)


CASES = {}
# every window of 385 .. 448 the issue lists, and three small ones, through the edge-aligned tile in both paddings (M = 135: two
# pixel tiles, 7 rows in the second); the atomic path takes the same operands
for _w in EDGE_WINDOWS + SMALL_WINDOWS:
    CASES["win%d/hostile" % _w] = _h(1, 9, 15, win=_w, E=3, paths=("edge", "atomic"))
    CASES["win%d/production" % _w] = _h(1, 9, 15, win=_w, E=3, kind="negative", pad="zero", paths=("edge", "atomic"))
CASES.update({
    # XCD-slot splits of the pixel tiles: n_ptiles = 8 pq + pr
    "slots/9_exact": _h(2, 24, 24),                                   # M = 1152: pq 1, pr 1, no tail
    "slots/9_tail": _h(3, 19, 19),                                    # M = 1083: pq 1, pr 1, 59 rows in the last tile
    "slots/23": _h(5, 24, 24),                                        # M = 2880: pq 2, pr 7
    "slots/7": _h(2, 21, 21),                                         # M = 882: pq 0, one empty slot
    "slots/1_partial": _h(1, 7, 9),                                   # M = 63
    # >= 3 tiles per workgroup across edge changes (the bias row alternates by tile parity in LDS)
    "walk17": _h(9, 24, 24, E=17),                                    # M = 5184: 41 pixel tiles x 17 edges
    # pixel ranges: cuts off every multiple of 128; multiples of 4 where HoWo % 4 == 0 (the route demands it of NCHW launches)
    "ranges/2": _h(3, 19, 19, ranges=((0, 500), (500, 583))),
    "ranges/3": _h(3, 19, 19, ranges=((0, 333), (333, 444), (777, 306))),
    "ranges/3_of4": _h(2, 24, 24, ranges=((0, 388), (388, 512), (900, 252))),
    # GEMM depth: two K steps (the last-step prefetch of the next tile is also the first loop step), four, and 512
    "depth/2steps": _h(3, 19, 19, ksteps=2),
    "depth/4steps": _h(3, 19, 19, ksteps=4),
    "depth/512": _h(3, 19, 19, K=512),
    # images smaller than a pixel tile
    "howo6": _h(40, 2, 3),                                            # a 128-pixel tile spans 21 images
    "howo1": _h(150, 1, 1),
    "null_bias": _h(3, 19, 19, bias=False, paths=("edge", "atomic")),
    # exact cases: tile 0 has exactly ONE ambiguous pixel, the ambiguous pixels of tile 1 are its last valid rows (M = 135), and
    # the 121 zero rows past them tie among themselves
    "ties": _h(1, 9, 15, kind="ties", paths=("edge", "atomic")),
    "saturated": _h(1, 9, 15, kind="saturated", paths=("edge", "atomic")),
    "ties/production": _h(1, 9, 15, kind="ties", pad="zero"),
    # the atomic-key epilogue of conv_big.hip alone
    "atomic/win81": _h(3, 15, 13, E=3, win=81, uch=108, paths=("atomic",)),
    "atomic/win441": _h(3, 15, 13, E=3, win=441, uch=108, paths=("atomic", "edge")),
    "atomic/win529": _h(2, 12, 16, E=2, win=529, uch=64, paths=("atomic",)),           # wider than a 448-row tile; HoWo % 4 == 0
    "atomic/win20": _h(3, 15, 13, E=9, win=20, uch=0, paths=("atomic",)),              # a 32-channel run crosses two edge boundaries
    "atomic/win20_u108": _h(3, 15, 13, E=9, win=20, uch=108, paths=("atomic",)),
    "atomic/win420_negative": _h(2, 12, 16, E=3, win=420, uch=108, kind="negative", paths=("atomic",)),
    "atomic/ties": _h(3, 15, 13, E=3, win=441, uch=108, kind="ties", paths=("atomic",)),
    "atomic/saturated": _h(3, 15, 13, E=3, win=81, uch=64, kind="saturated", paths=("atomic",)),
})
AMBIGUOUS = {"ties": (77, 133, 134), "saturated": (77, 133, 134), "ties/production": (77, 133, 134),
             "atomic/ties": (5, 300, 584), "atomic/saturated": (5, 300, 584)}
# forced tiles of the atomic path (test_conv_tiles_gpu.force_tile); None: the automatic choice
ATOMIC_TILES = (None, (192, 128), (256, 256))
ODD_DEPTH_STEPS = 3                          # refused: the edge kernel needs an even number of K steps


def k_step(dtype):
    return 32 if dtype == "f32" else 64


def depth(c, dtype):
    return c.ksteps * k_step(dtype) if c.ksteps else c.K


def pixels(c):
    return c.B * c.H * c.W


def schedule(m_count, n_edges, n_cu):
    """The persistent tile walk of head_limb_argmax_kernel for a launch over m_count pixels on n_cu compute units, restated:
    n_ptiles = 8 pq + pr; workgroup b has XCD slot b & 7 and index b >> 3 in it; slot x owns pq + (x < pr) pixel tiles for all
    edges and its workgroups take local tiles index, index + per, ...; edge = local tile // pixel tiles of the slot."""
    n_ptiles = -(-m_count // BP)
    pq, pr = divmod(n_ptiles, 8)
    grid = min(max(n_cu, 8) // 8 * 8, 8 * (pq + (1 if pr else 0)) * n_edges)
    per = grid // 8
    walks = []
    for b in range(grid):
        x, idx = b & 7, b >> 3
        psize = pq + (1 if x < pr else 0)
        walks.append([li // psize for li in range(idx, psize * n_edges, per)])
    return {"n_ptiles": n_ptiles, "pq": pq, "pr": pr, "grid": grid, "tail": m_count % BP,
            "max_tiles": max(len(w_) for w_ in walks), "empty": sum(1 for w_ in walks if not w_),
            "edge_changes": max((sum(1 for a, b_ in zip(w_, w_[1:]) if a != b_) for w_ in walks), default=0)}


def _seed(name):
    return 4000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100000


def _random_operands(c, dtype, K, g):
    scale = (1.8432 / K) ** 0.5                  # 0.06 / 0.12 / 0.17 at K = 512 / 128 / 64: logit standard deviation 1.36
    C = c.uch + c.E * c.win
    x = q(torch.randn(c.B, K, c.H, c.W, generator=g), dtype)
    w = q(torch.randn(C, K, generator=g) * scale, dtype)
    b = torch.randn(C, generator=g) * 0.1
    if c.kind == "negative":
        b[c.uch:] -= NEGATIVE_SHIFT
    return x, w, (b if c.bias else None)


def tie_rows(c):
    """The three window indices the exact cases arrange: first, middle, last."""
    return (min(3, c.win - 3), c.win // 2, c.win - 1)


def _exact_operands(c, name, K, g):
    C, M = c.uch + c.E * c.win, pixels(c)
    x = torch.randint(-2, 3, (M, K), generator=g).float()
    x[:, 0] = 1.0
    x[list(AMBIGUOUS[name]), 0] = 0.0
    w = torch.zeros(C, K)
    cols = torch.stack([torch.randperm(K - 1, generator=g)[:4] + 1 for _ in range(C)])
    w.scatter_(1, cols, torch.randint(0, 2, (C, 4), generator=g).float() * 2 - 1)          # four +-1 per row: |x . w| <= 8
    quarters = torch.randint(0, 9, (C,), generator=g).float() / 4
    i1, i2, i3 = tie_rows(c)
    if c.kind == "ties":
        b = -18.0 - quarters                                                                # others: logits in [-28, -10]
        b[:c.uch] = -quarters[:c.uch]
        for e in range(c.E):
            r = c.uch + e * c.win
            w[r + i2], w[r + i3] = w[r + i1], w[r + i1]
            w[r + i1, 0], w[r + i2, 0], w[r + i3, 0] = -2.0, 0.0, -1.0                      # the three: logits in [-10, 8]
            b[r + i1] = b[r + i2] = b[r + i3] = 0.0
    else:
        b = -quarters                                                                       # others: logits in [-10, 8]
        for e in range(c.E):
            r = c.uch + e * c.win
            b[r + i1], b[r + i2], b[r + i3] = 31.0, 30.25, 30.0                             # logits in [22, 39]
            w[r + i1, 0] = -40.0                                                            # ... in [-17, -1] where the flag is 1
    x = x.view(c.B, c.H, c.W, K).permute(0, 3, 1, 2).contiguous()
    return x, w, b


@functools.lru_cache(maxsize=None)
def operands(name, dtype):
    """(x [B, K, H, W], w [uch + E * win, K], bias [uch + E * win] or None): f32 tensors holding values of the storage type (the
    bias is f32 in every type).  Fixed seed per case."""
    c = CASES[name]
    g = torch.Generator().manual_seed(_seed(name))
    K = depth(c, dtype)
    if c.kind in ("ties", "saturated"):
        x, w, b = _exact_operands(c, name, K, g)
        assert torch.equal(q(x, dtype), x) and torch.equal(q(w, dtype), w)
        return x, w, b
    return _random_operands(c, dtype, K, g)


def exact_condition(x, w, b):
    """Every partial sum of every logit, in any order, is exact in f32: all terms are multiples of 1/4 and S + |b| <= 2^21."""
    M = x.shape[0] * x.shape[2] * x.shape[3]
    X = x.permute(0, 2, 3, 1).reshape(M, -1).double()
    S = X.abs() @ w.double().abs().t() + b.double().abs()
    whole = all(bool((t * 4 == (t * 4).round()).all()) for t in (x, w, b))
    return whole and float(S.max()) <= 2.0 ** 21


Ref = collections.namedtuple("Ref", "t A tu Au first tmax decided")


def sigmoid64(t):
    return torch.sigmoid(t.double())


def e_rel(m):
    return U * (7.0 + 2.0 * (-m).clamp(min=0.0)) * (1.0 + 2.0 ** -10)


def e_sig(t):
    return sigmoid64(t) * e_rel(t)


def d_width(m, a_star):
    return 2.0 * e_rel(m) * (1.0 + torch.exp(m + a_star))


def value_bound(t, A):
    s = sigmoid64(t)
    return s * (1.0 - s) * A * (1.0 + A) + e_sig(t) + TINY


def first_max(t):
    """(maximum, lowest index attaining it) along the last axis."""
    m = t.max(dim=-1).values
    return m, (t == m.unsqueeze(-1)).to(torch.uint8).argmax(dim=-1)


def reference_of(c, x, w, b):
    """Ref of a case's operands: t, A f64 [M, E, win] of the limb windows; tu, Au [M, uch] of the unary channels; per window the
    first f64 maximum, its logit, and whether the window is decided."""
    M, K = pixels(c), x.shape[1]
    X = x.permute(0, 2, 3, 1).reshape(M, K).double()
    W = w.double()
    bias = b.double() if b is not None else torch.zeros(W.shape[0], dtype=torch.float64)
    t = X @ W.t() + bias
    A = X.abs() @ W.abs().t()
    A.add_(bias.abs()).mul_((K + 4) * U)
    tu, Au = t[:, :c.uch], A[:, :c.uch]
    t, A = t[:, c.uch:].reshape(M, c.E, c.win), A[:, c.uch:].reshape(M, c.E, c.win)
    tmax, first = first_max(t)
    a_star = A.gather(2, first.unsqueeze(-1)).squeeze(-1)
    rival = (t + A).scatter(2, first.unsqueeze(-1), float("-inf")).max(dim=2).values       # -inf when win == 1
    decided = tmax - rival > a_star + d_width(tmax, a_star)
    return Ref(t, A, tu, Au, first, tmax, decided)


@functools.lru_cache(maxsize=2)
def reference(name, dtype):
    """Computed once per (case, dtype) and shared by consecutive users: callers must not modify what they get."""
    return reference_of(CASES[name], *operands(name, dtype))


def split_keys(keys):
    """keys i64 [B, E, H, W] -> (value f32 [M, E], index i64 [M, E]) in the reference's pixel order."""
    k = keys.permute(0, 2, 3, 1).reshape(-1, keys.shape[1])
    bits = ((k >> 32) & 0xFFFFFFFF).numpy().astype(np.uint32)
    return torch.from_numpy(bits.view(np.float32).copy()), 0xFFFFFFFF - (k & 0xFFFFFFFF)


def make_keys(val, idx, c):
    """The inverse of split_keys: (value f32 [M, E], index [M, E]) -> keys i64 [B, E, H, W]."""
    bits = val.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    k = (bits << 32) | (0xFFFFFFFF - idx.to(torch.int64))
    return k.view(c.B, c.H, c.W, c.E).permute(0, 3, 1, 2).contiguous()


Verdict = collections.namedtuple("Verdict", "ok ratio undecided bad_index not_near wrong_decided where")


def check(c, ref, keys, rows=None):
    """Judge keys i64 [B, E, H, W] against ref.  rows: a bool [M] mask of the pixels to judge (a launch over a pixel range) or
    None.  ok needs: every index in range, every key near-maximal, every decided window exact, value ratio <= 1."""
    val, idx = split_keys(keys)
    if rows is None:
        rows = torch.ones(idx.shape[0], dtype=torch.bool)
    live = rows.unsqueeze(1).expand_as(idx)
    in_range = (idx >= 0) & (idx < c.win)
    k = idx.clamp(0, c.win - 1).unsqueeze(-1)
    tk, Ak = ref.t.gather(2, k).squeeze(-1), ref.A.gather(2, k).squeeze(-1)
    a_star = ref.A.gather(2, ref.first.unsqueeze(-1)).squeeze(-1)
    near = tk >= ref.tmax - Ak - a_star - d_width(ref.tmax, a_star)
    right = (idx == ref.first) | ~ref.decided
    r = (val.double() - sigmoid64(tk)).abs() / value_bound(tk, Ak)
    r = torch.nan_to_num(r, nan=float("inf"))
    bad = live & ~(in_range & near & right & (r <= 1.0))
    where = None
    if bool(bad.any()):
        m, e = (int(v) for v in bad.nonzero()[0])
        where = "pixel %d edge %d: key (%.9g, %d), f64 first maximum %d (logit %.6f, key's logit %.6f), %s" % (
            m, e, float(val[m, e]), int(idx[m, e]), int(ref.first[m, e]), float(ref.tmax[m, e]), float(tk[m, e]),
            "decided" if bool(ref.decided[m, e]) else "undecided")
    n = max(1, int(live.sum()))
    return Verdict(where is None, float(r[live].max()) if bool(live.any()) else 0.0, float((live & ~ref.decided).sum()) / n,
                   int((live & ~in_range).sum()), int((live & in_range & ~near).sum()), int((live & in_range & ~right).sum()), where)


def expected_exact(c, ref):
    """(index i64 [M, E], value bits i64 [M, E] or None) an exact case must give: the lowest index with a logit >= 20 where there
    is one (`saturated`: value 1.0f), else the first maximum of the logits."""
    sat = ref.t >= 20.0
    if c.kind == "saturated":
        assert bool(sat.any(dim=2).all())
        return sat.to(torch.uint8).argmax(dim=2), torch.full(ref.first.shape, SAT_BITS, dtype=torch.int64)
    assert c.kind == "ties" and not bool(sat.any())
    return ref.first, None


def check_exact(c, ref, keys):
    """Why the keys of an exact case are wrong (a string), or None."""
    val, idx = split_keys(keys)
    want_idx, want_bits = expected_exact(c, ref)
    bad = idx != want_idx
    if want_bits is not None:
        bad |= (val.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF) != want_bits
    if not bool(bad.any()):
        return None
    m, e = (int(v) for v in bad.nonzero()[0])
    return "pixel %d edge %d: key (%.9g, %d), wanted index %d%s" % (
        m, e, float(val[m, e]), int(idx[m, e]), int(want_idx[m, e]), "" if want_bits is None else " with value 1.0f")


def head_ratio(c, ref, head):
    """max err / bound of a materialised NCHW sigmoid head f32 [B, uch + E * win, H, W] against sigmoid64(t), every element."""
    M = pixels(c)
    got = head.permute(0, 2, 3, 1).reshape(M, -1).double()
    t = torch.cat([ref.tu, ref.t.reshape(M, -1)], dim=1)
    A = torch.cat([ref.Au, ref.A.reshape(M, -1)], dim=1)
    r = (got - sigmoid64(t)).abs() / value_bound(t, A)
    return float("inf") if bool(torch.isnan(r).any()) else float(r.max())


def emulate(c, x, w, b, win_rows=None):
    """What a correct kernel may return, as keys i64 [B, E, H, W]: f32 logits (torch's order), f32 sigmoid, first maximum of the
    VALUES.  win_rows: the value matrix [M, E, rows] is handed to this callable before the arg-max (where planted faults go in)."""
    M, K = pixels(c), x.shape[1]
    X = x.permute(0, 2, 3, 1).reshape(M, K)
    t = X @ w[c.uch:].t()
    if b is not None:
        t = t + b[c.uch:]
    v = torch.sigmoid(t.float()).view(M, c.E, c.win)
    if win_rows is not None:
        v = win_rows(v)
    val, idx = first_max(v)
    return make_keys(val, idx, c)
