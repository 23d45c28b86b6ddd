"""Cases, operands, f64 references and DERIVED per-element error bounds for the two MFMA stages of csrc/stgcn16.hip
(ppn_stgcn16_gcn, ppn_stgcn16_tcn) and the inputs of the float16 whole-network tests.  Plain helper module (no tests):
tests/test_actions16_cpu.py shows that an emulation in f32 arithmetic stays inside the bounds and that planted faults leave
them; tests/test_actions16_gpu.py runs the kernels.  The shapes are tests/stgcn_cases.py's, by import.

Operands.  x and u are stgcn_cases' operands rounded to half FIRST, so they are exact inputs; weights and adjacency are the
f64 folded values rounded once to half (tests/stgcn16_ref.py's own fold).  The reference is f64 on these rounded operands,
without the rounding of y and of the output: those are terms of the bound.  h = 2^-11 (half), u = 2^-24 (f32); S is the
reference's expression on absolute values, in f64; 2^-25 is half the smallest subnormal half.

GCN stage  (out = half(relu(z s0 + t0)), z = sum_{p,ci} W half(y), y = sum_v x A):
    bound = 1.01 h |ref| + 2^-25                                   the output's rounding, with its subnormal floor
          + |s0| (1.01 h S + 2^-25 sum_{p,ci} |W|)                 the ONE rounding of y, passed through |W| and the scale
          + 1.01 (K + P cin + 6) u (S |s0| + |t0|)                 the two f32 chains, the scale and shift roundings (stgcn_cases)
TCN stage  (out = half(relu(z s3 + t3 (+ x)))):
    bound = 1.01 h |ref| + 2^-25 + (depth + 4) u (S + |t3|) (+ 2 u |x| for identity),  depth = 9 cout (+ cin for proj)
    with S = |s3| (conv(|u|, |Wt|) + conv1x1(|x|, |Wr'|)).
The bounds may be widened only by a named term for a rounding step the kernel's source shows, never to fit what a kernel
returned.

Wall cases: the two outer clips are 6.0e4 everywhere (finite in half).  Their own outputs may overflow to inf, which the contract
allows; finiteness and the bound are asserted on the MIDDLE clip only.

Exact cases: small-integer operands, an adjacency of 0 / 0.5 / 1, scale 1, shift 0, chosen so that every intermediate and
output of the reference is an integer of magnitude <= 2048 (the caller asserts it): a kernel must match on every byte.
"""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import stgcn16_ref as R16
import stgcn_cases as SC

H = 2.0 ** -11
U = 2.0 ** -24
FLOOR = 2.0 ** -25
WALL16 = 6.0e4


def _block(c):
    A = c["sd"]["A"].double().numpy()
    return R16.fold_block(c["sd"], 0, c["spec"].P, A, c["spec"].blocks[0])


def _ch(a):
    return torch.from_numpy(np.ascontiguousarray(a)).view(1, -1, 1, 1)


def gcn_bound(b, x, ref):
    """x f64 [n, cin, t, v] (half values), ref f64 [n, cout, t, v]."""
    P, cout, cin = b["wg"].shape
    K = b["adj"].shape[1]
    adj, wg = torch.from_numpy(np.abs(R16.rh(b["adj"]))), torch.from_numpy(np.abs(R16.rh(b["wg"])))
    S = torch.einsum("npitw,pci->nctw", torch.einsum("nitv,pvw->npitw", x.abs(), adj), wg)
    s0, t0 = _ch(np.abs(b["s0"])), torch.from_numpy(np.abs(b["t0"])).t().unsqueeze(0).unsqueeze(2)
    sum_w = _ch(wg.sum(dim=(0, 2)).numpy())
    return (1.01 * H * ref.abs() + FLOOR + s0 * (1.01 * H * S + FLOOR * sum_w) + 1.01 * (K + P * cin + 6) * U * (S * s0 + t0))


def tcn_bound(b, u, x, ref):
    cout, cin, s = b["cout"], b["cin"], b["stride"]
    S = F.conv2d(u.abs(), torch.from_numpy(np.abs(R16.rh(b["wt"]))).unsqueeze(-1), None, (s, 1), (4, 0))
    depth = 9 * cout
    if b["residual"] == "proj":
        S = S + F.conv2d(x.abs(), torch.from_numpy(np.abs(R16.rh(b["wr"]))).view(cout, cin, 1, 1), None, (s, 1))
        depth += cin
    bound = 1.01 * H * ref.abs() + FLOOR + (depth + 4) * U * (S * _ch(np.abs(b["s3"])) + _ch(np.abs(b["t3"])))
    if b["residual"] == "identity":
        bound = bound + 2 * U * x.abs()
    return bound


@functools.lru_cache(maxsize=None)
def gcn_case(name):
    """{case, spec, sd, b (folded, f64), x f64 [n, cin, T, K] (half values), ref f64, bound}; callers must not modify it."""
    c = SC.gcn_case(name)
    b, x = _block(c), R16.rh(c["x"].double())
    ref = R16.gcn16(b, x, torch.float64, exact=True)
    return dict(case=c["case"], spec=c["spec"], sd=c["sd"], b=b, x=x, ref=ref, bound=gcn_bound(b, x, ref))


@functools.lru_cache(maxsize=None)
def tcn_case(name):
    """{case, spec, sd, b, u, x f64 (half values), ref f64, bound}; wall cases: 6.0e4 in the two outer clips."""
    c = SC.tcn_case(name)
    b = _block(c)
    u, x = c["u"].double().clone(), c["x"].double().clone()
    if name in SC.WALL_CASES:
        u[0], u[2], x[0], x[2] = WALL16, WALL16, WALL16, WALL16
    u, x = R16.rh(u), R16.rh(x)
    ref = R16.tcn16(b, u, x, torch.float64, exact=True)
    return dict(case=c["case"], spec=c["spec"], sd=c["sd"], b=b, u=u, x=x, ref=ref, bound=tcn_bound(b, u, x, ref))


def mid(name):
    """The clips a case is judged on: the middle one between two walls, else all."""
    return slice(1, 2) if name in SC.WALL_CASES else slice(None)


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
EXACT_GCN, EXACT_TCN = "16_32_t7", "16_32_s2_proj_t7"


def _ints(rng, shape, lo, hi, density=1.0):
    v = rng.integers(lo, hi + 1, shape).astype(np.float64)
    return v * (rng.random(shape) < density)


@functools.lru_cache(maxsize=None)
def exact_gcn():
    """{case, b, x, y, ref}: even integers x in -4..4, an asymmetric adjacency of 0 / 0.5 / 1, W in {-1, 0, 1}."""
    k = SC.GCN_CASES[EXACT_GCN]
    rng = np.random.default_rng(161)
    adj = rng.choice([0.0, 0.5, 1.0], (3, k.K, k.K), p=[0.75, 0.125, 0.125])
    b = dict(cin=k.cin, cout=k.cout, stride=1, residual="none", adj=adj, wg=_ints(rng, (3, k.cout, k.cin), -1, 1, 0.5),
             s0=np.ones(k.cout), t0=np.zeros((k.K, k.cout)), wt=np.zeros((k.cout, k.cout, 9)), wr=None, s3=np.ones(k.cout),
             t3=np.zeros(k.cout))
    x = torch.from_numpy(2.0 * _ints(rng, (k.n, k.cin, k.T, k.K), -2, 2))
    y = torch.einsum("nitv,pvw->npitw", x, torch.from_numpy(adj))
    return dict(case=k, b=b, x=x, y=y, ref=R16.gcn16(b, x, torch.float64, exact=True))


@functools.lru_cache(maxsize=None)
def exact_tcn():
    """{case, b, u, x, ref}: integers u in 0..3, x in -2..2, Wt and Wr' in {-1, 0, 1}."""
    k = SC.TCN_CASES[EXACT_TCN]
    rng = np.random.default_rng(162)
    b = dict(cin=k.cin, cout=k.cout, stride=k.stride, residual=k.residual, adj=np.zeros((3, k.K, k.K)),
             wg=np.zeros((3, k.cout, k.cin)), s0=np.ones(k.cout), t0=np.zeros((k.K, k.cout)),
             wt=_ints(rng, (k.cout, k.cout, 9), -1, 1, 0.5), wr=_ints(rng, (k.cout, k.cin), -1, 1), s3=np.ones(k.cout),
             t3=np.zeros(k.cout))
    u = torch.from_numpy(_ints(rng, (k.n, k.cout, k.T, k.K), 0, 3))
    x = torch.from_numpy(_ints(rng, (k.n, k.cin, k.T, k.K), -2, 2))
    return dict(case=k, b=b, u=u, x=x, ref=R16.tcn16(b, u, x, torch.float64, exact=True))


def small_integers(*tensors):
    """Every value an integer of magnitude <= 2048: exactly representable in half, sums of them exact in f32."""
    return all(bool((t == t.round()).all()) and float(t.abs().max()) <= 2048 for t in tensors)


# ---- the whole network ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def network(name):
    """stgcn_cases.network(name) plus {emu64, emu32, E16}: the float16 mode emulated in f64 and in f32 arithmetic, E16 = max
    |emu32 - emu64|."""
    net = dict(SC.network(name))
    net["emu64"] = R16.forward16(net["spec"], net["sd"], net["A"], net["clips"], torch.float64)
    net["emu32"] = R16.forward16(net["spec"], net["sd"], net["A"], net["clips"], torch.float32)
    net["E16"] = float((net["emu32"].double() - net["emu64"]).abs().max())
    return net


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def refusals(lib):
    """[(what, return code, expected)] of ppn_stgcn16_* calls that must be refused before anything is launched (no GPU is
    touched): stgcn_cases.refusals' list with PPN_F16 as the good dtype, PPN_F32 and PPN_BF16 unsupported."""
    import ctypes as C
    l = lib.load()
    p = 4096                                                    # a non-NULL, 16-byte aligned address nothing dereferences
    ok = dict(dtype=lib.PPN_F16, K=18, P=3, T=8, cin=16, cout=16, stride=1, residual=lib.PPN_STGCN_RES_NONE)
    out = []

    def gcn(**kw):
        d = lib.StgcnDesc(**dict(ok, **{k: v for k, v in kw.items() if k in ok}))
        return l.ppn_stgcn16_gcn(C.byref(d), kw.get("x", p), kw.get("w", p), p, p, p, p, kw.get("capacity", 64), kw.get("out", p), None)

    def tcn(**kw):
        d = lib.StgcnDesc(**dict(ok, **{k: v for k, v in kw.items() if k in ok}))
        return l.ppn_stgcn16_tcn(C.byref(d), kw.get("u", p), kw.get("x", p), kw.get("w", p), p, p, p, kw.get("capacity", 64),
                                 kw.get("out", p), None)

    inv, uns = -1, -3                                           # PPN_E_INVALID, PPN_E_UNSUPPORTED
    for fn, f in (("gcn", gcn), ("tcn", tcn)):
        out += [(f"{fn} bf16", f(dtype=lib.PPN_BF16), uns), (f"{fn} f32", f(dtype=lib.PPN_F32), uns),
                (f"{fn} f16x3", f(dtype=lib.PPN_F16X3), uns),
                (f"{fn} K 0", f(K=0), inv), (f"{fn} K 33", f(K=33), inv), (f"{fn} T 0", f(T=0), inv),
                (f"{fn} P 4", f(P=4), inv), (f"{fn} cout 24", f(cout=24), inv), (f"{fn} cout 272", f(cout=272), inv),
                (f"{fn} cin 8", f(cin=8), inv), (f"{fn} stride 3", f(stride=3), inv), (f"{fn} residual 3", f(residual=3), inv),
                (f"{fn} identity cin != cout", f(residual=lib.PPN_STGCN_RES_IDENTITY, cout=32), inv),
                (f"{fn} identity stride 2", f(residual=lib.PPN_STGCN_RES_IDENTITY, stride=2), inv),
                (f"{fn} capacity 0", f(capacity=0), inv), (f"{fn} capacity 65", f(capacity=65), inv),
                (f"{fn} misaligned w", f(w=p + 8), inv), (f"{fn} misaligned out", f(out=p + 8), inv)]
    out += [("gcn NULL w", gcn(w=None), inv), ("gcn misaligned x", gcn(x=p + 8), inv), ("tcn misaligned u", tcn(u=p + 8), inv),
            ("tcn NULL x with a shortcut", tcn(x=None, residual=lib.PPN_STGCN_RES_PROJ, cout=32), inv),
            ("tcn misaligned x with a shortcut", tcn(x=p + 8, residual=lib.PPN_STGCN_RES_PROJ, cout=32), inv),
            ("gcn NULL desc", l.ppn_stgcn16_gcn(None, p, p, p, p, p, p, 64, p, None), inv)]
    d = lib.StgcnDesc(**ok)
    d32 = lib.StgcnDesc(**dict(ok, dtype=lib.PPN_F32))
    dbf = lib.StgcnDesc(**dict(ok, dtype=lib.PPN_BF16))
    out += [("input f32", l.ppn_stgcn16_input(C.byref(d32), p, p, p, 1, 1, p, p, p, p, p, p, None), uns),
            ("input bf16", l.ppn_stgcn16_input(C.byref(dbf), p, p, p, 1, 1, p, p, p, p, p, p, None), uns),
            ("input 0 streams", l.ppn_stgcn16_input(C.byref(d), p, p, p, 0, 1, p, p, p, p, p, p, None), inv),
            ("input NULL ids", l.ppn_stgcn16_input(C.byref(d), p, None, p, 1, 1, p, p, p, p, p, p, None), inv),
            ("input misaligned x0", l.ppn_stgcn16_input(C.byref(d), p, p, p, 1, 1, p, p, p, p, p, p + 8, None), inv),
            ("head f32", l.ppn_stgcn16_head(C.byref(d32), 4, p, p, p, p, 1, p, p, None), uns),
            ("head bf16", l.ppn_stgcn16_head(C.byref(dbf), 4, p, p, p, p, 1, p, p, None), uns),
            ("head 0 classes", l.ppn_stgcn16_head(C.byref(d), 0, p, p, p, p, 1, p, p, None), inv),
            ("head 1025 classes", l.ppn_stgcn16_head(C.byref(d), 1025, p, p, p, p, 1, p, p, None), inv),
            ("head NULL rank", l.ppn_stgcn16_head(C.byref(d), 4, p, p, p, None, 1, p, p, None), inv)]
    return out
