"""Cases, operands, f64 references and DERIVED per-element error bounds for the two MFMA stages of csrc/stgcn.hip
(ppn_stgcn_gcn, ppn_stgcn_tcn) and the inputs of the whole-network tests, in the manner of tests/forward_cases.py.  Plain
helper module (no tests): tests/test_actions_cpu.py shows that an f32 evaluation stays inside the bounds and that planted
faults leave them; tests/test_actions_gpu.py runs the kernels.

References come from tests/stgcn_ref.py (the UNFOLDED state dict, f64); scales and shifts for the bounds are worked out here
from the same dict, not taken from actions.py.  u = 2^-24; S is the reference's expression on absolute values, in f64.

GCN stage  (out = relu(z s0 + t0), z = sum_p sum_v (sum_ci W x) A):
    bound = u_out |ref| + 1.01 (K + P cin + 6) u (S |s0| + |t0|) + tiny
    two chained f32 sums of lengths K and P cin, in either order (n u sum |terms| bounds an f32 sum of n products in any
    order); the remaining 6: the roundings of the folded adjacency (A x importance), s0 and t0 to f32, the scale, the shift,
    and one to spare; 1.01 covers the second-order terms of the chain.  t0 is the folded shift with the gcn bias passed through
    the adjacency.
TCN stage  (out = relu(z s3 + t3 (+ x)), z = the 9 x 1 convolution (+ the projection shortcut as further depth)):
    A     = (depth + 4) u (S |s3| + |t3|),   depth = 9 cout (+ cin for proj)        forward_cases' bound
    bound = u_out |ref| + A (+ 2 u |x| for identity) + tiny
    with S |s3| = |s3| conv(|u|, |Wt|) + |sr| conv1x1(|x|, |Wr|): the shortcut's weights reach the kernel scaled by sr / s3 and
    leave it scaled by s3 (one more rounding per product, inside the 4).
u_out = 2^-23 (f32 stores), tiny = 2^-126.  ReLU is 1-Lipschitz.  The bounds may be widened only by a named term for a rounding
step the kernel's source shows, never to fit what a kernel returned.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools

import numpy as np
import torch
import torch.nn.functional as F

import stgcn_ref as R
from pytorch_pose_proposal_network_amd import actions as AC
from pytorch_pose_proposal_network_amd import prng

U = 2.0 ** -24
U_OUT = 2.0 ** -23
TINY = 2.0 ** -126
EPS = 1e-5

Gcn = collections.namedtuple("Gcn", "cin cout T K n")
Tcn = collections.namedtuple("Tcn", "cin cout stride residual T K n")

HAND_EDGES = [(0, 1), (1, 2), (1, 3), (3, 4)]          # the K = 5 graph: a star at joint 1 with one arm of two

GCN_CASES = {
    "3_16_t8": Gcn(3, 16, 8, 18, 2),                   # cin padded inside the kernel, one full tile of 144 rows
    "16_32_t7": Gcn(16, 32, 7, 18, 2),                 # a partial time tile: 126 rows, the last row tile partial
    "32_32_t1": Gcn(32, 32, 1, 18, 1),                 # 18 rows: one full and one partial row tile, two depth chunks
    "256_256_t8": Gcn(256, 256, 8, 18, 1),             # four channel groups, sixteen depth chunks
    "16_16_k5": Gcn(16, 16, 9, 5, 2),                  # a hand-made graph; 40 rows per tile, a second tile of 5
    "16_16_n1": Gcn(16, 16, 9, 18, 1),
    "16_16_n2": Gcn(16, 16, 9, 18, 2),
    "16_16_n5": Gcn(16, 16, 9, 18, 5),
}

TCN_CASES = {}
for _T in (1, 7, 8, 9, 32):
    TCN_CASES[f"16_16_s1_identity_t{_T}"] = Tcn(16, 16, 1, "identity", _T, 18, 2)
    TCN_CASES[f"16_32_s2_proj_t{_T}"] = Tcn(16, 32, 2, "proj", _T, 18, 2)
TCN_CASES.update({
    "16_16_s1_none_t9": Tcn(16, 16, 1, "none", 9, 18, 2),
    "16_16_s2_none_t9": Tcn(16, 16, 2, "none", 9, 18, 2),
    "16_32_s1_proj_t9": Tcn(16, 32, 1, "proj", 9, 18, 2),
    "3_16_s2_proj_t7": Tcn(3, 16, 2, "proj", 7, 18, 1),           # a shortcut from 3 channels: its depth chunk is padded
    "256_256_s1_identity_t8": Tcn(256, 256, 1, "identity", 8, 18, 1),
    "256_256_s2_proj_t9": Tcn(256, 256, 2, "proj", 9, 18, 1),
    "16_16_k5_identity_t9": Tcn(16, 16, 1, "identity", 9, 5, 3),
})
# three adjacent clips, the outer two 1e30 everywhere: a read across a clip boundary breaks the bound by thirty orders
WALL_CASES = {
    "wall_s1": Tcn(16, 16, 1, "identity", 8, 18, 3),
    "wall_s2": Tcn(16, 32, 2, "proj", 9, 18, 3),
    "wall_t1": Tcn(16, 16, 1, "none", 1, 18, 3),
}
WALL = 1e30
ALL_TCN = dict(TCN_CASES, **WALL_CASES)


def _seed(name):
    return 7000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100000


def graph_of(K):
    """f32 tensor [3, K, K]: the project's skeleton for K = 18, the hand-made graph for K = 5."""
    if K == 18:
        return torch.from_numpy(AC.skeleton_graph())
    assert K == 5
    return torch.from_numpy(AC.skeleton_graph(HAND_EDGES, 5, 1))


def block_setup(c, seed):
    """(spec of the one block, state dict with its own "A", graph) of a stage case."""
    res = getattr(c, "residual", "none")
    spec = AC.STGCNSpec(((c.cin, c.cout, getattr(c, "stride", 1), res),), 4, c.K)
    sd = AC.random_state_dict(spec, seed)
    sd["A"] = graph_of(c.K)
    return spec, sd, sd["A"]


def _randn(seed, shape):
    return torch.from_numpy(prng.normalish(seed, int(np.prod(shape))).reshape(shape).copy())


def _bn(sd, prefix):
    s = sd[prefix + ".weight"].double() / torch.sqrt(sd[prefix + ".running_var"].double() + EPS)
    return s, sd[prefix + ".bias"].double() - sd[prefix + ".running_mean"].double() * s


def ch(t):
    return t.view(1, -1, 1, 1)


@functools.lru_cache(maxsize=None)
def gcn_case(name):
    """{spec, sd, x f32 [n, cin, T, K], ref f64 [n, cout, T, K], bound}; callers must not modify what they get."""
    c = GCN_CASES[name]
    spec, sd, A = block_setup(c, _seed(name))
    x = _randn(_seed(name) + 1, (c.n, c.cin, c.T, c.K))
    ref, bound = gcn_reference(spec, sd, A, x)
    return dict(case=c, spec=spec, sd=sd, x=x, ref=ref, bound=bound)


def gcn_reference(spec, sd, A, x):
    cin, cout = spec.blocks[0][:2]
    P, K = spec.P, spec.K
    b = "st_gcn_networks.0"
    ref = R.gcn(sd, 0, P, A, x.double())
    adj = (A.double() * sd["edge_importance.0"].double())
    g = F.conv2d(x.double().abs(), sd[b + ".gcn.conv.weight"].double().abs()).view(x.shape[0], P, cout, x.shape[2], K)
    S = torch.einsum("nkctv,kvw->nctw", g, adj.abs())
    s0, h0 = _bn(sd, b + ".tcn.0")
    t0 = s0.view(-1, 1) * torch.einsum("pc,pw->cw", sd[b + ".gcn.conv.bias"].double().view(P, cout), adj.sum(1)) + h0.view(-1, 1)
    bound = U_OUT * ref.abs() + 1.01 * (K + P * cin + 6) * U * (S * ch(s0.abs()) + t0.abs().view(1, cout, 1, K)) + TINY
    return ref, bound


@functools.lru_cache(maxsize=None)
def tcn_case(name):
    """{spec, sd, u f32 [n, cout, T, K] (non-negative, as a ReLU leaves it), x f32 [n, cin, T, K], ref, bound}."""
    c = ALL_TCN[name]
    spec, sd, _ = block_setup(c, _seed(name))
    u = _randn(_seed(name) + 1, (c.n, c.cout, c.T, c.K)).clamp_(min=0)
    x = _randn(_seed(name) + 2, (c.n, c.cin, c.T, c.K))
    if name in WALL_CASES:
        u[0], u[2] = WALL, WALL
        x[0], x[2] = WALL, WALL
    ref, bound = tcn_reference(spec, sd, u, x)
    return dict(case=c, spec=spec, sd=sd, u=u, x=x, ref=ref, bound=bound)


def tcn_reference(spec, sd, u, x):
    cin, cout, stride, residual = spec.blocks[0]
    b = "st_gcn_networks.0"
    ref = R.tcn(sd, 0, stride, residual, u.double(), x.double())
    s3, h3 = _bn(sd, b + ".tcn.3")
    S = ch(s3.abs()) * F.conv2d(u.double().abs(), sd[b + ".tcn.2.weight"].double().abs(), None, (stride, 1), (4, 0))
    t3 = s3 * sd[b + ".tcn.2.bias"].double() + h3
    depth = 9 * cout
    if residual == "proj":
        sr, hr = _bn(sd, b + ".residual.1")
        S = S + ch(sr.abs()) * F.conv2d(x.double().abs(), sd[b + ".residual.0.weight"].double().abs(), None, (stride, 1))
        t3 = t3 + sr * sd[b + ".residual.0.bias"].double() + hr
        depth += cin
    bound = U_OUT * ref.abs() + (depth + 4) * U * (S + ch(t3.abs())) + TINY
    if residual == "identity":
        bound = bound + 2 * U * x.double().abs()
    return ref, bound


def ratio(got, ref, bound):
    """max(err / bound) over the tensor [n, c, t, v]; a case passes at ratio <= 1.  A NaN or inf in `got` gives inf."""
    r = (got.double() - ref).abs() / bound
    return float("inf") if not torch.isfinite(r).all() else float(r.max())


def to_nctv(t):
    """The kernels' [n, t, v, c] -> the reference's [n, c, t, v]."""
    return t.permute(0, 3, 1, 2)


def to_ntvc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- the whole network --------------------------------------------------------------------------------------------------------
NETWORKS = {"tiny": ("tiny", 16, 10, 11), "paper": ("paper", 32, 60, 12)}      # preset, T, num_class, seed
N_CLIPS = 3


def clips_like_root_norm(seed, n, T, K):
    """f32 [n, 3, T, K] in the range PoseClips' norm="root" produces: x and y within about +-0.6 of the root box's centre (a
    pose that drifts along the clip), scores in [0, 1]."""
    pose = prng.uniform(seed, n * 2 * K, -0.45, 0.45).reshape(n, 2, 1, K)
    drift = np.cumsum(prng.uniform(seed + 1, n * 2 * T * K, -0.02, 0.02).reshape(n, 2, T, K), axis=2)
    xy = np.clip(pose + drift, -0.6, 0.6)
    score = prng.uniform(seed + 2, n * T * K, 0.0, 1.0).reshape(n, 1, T, K)
    return torch.from_numpy(np.concatenate([xy, score], axis=1).astype(np.float32))


@functools.lru_cache(maxsize=None)
def network(name):
    """{spec, sd, A, T, clips f32 [3, 3, T, K], ref64, ref32, E}: E = max |stgcn_ref in f32 - stgcn_ref in f64|."""
    preset, T, nc, seed = NETWORKS[name]
    spec = AC.stgcn_spec(preset, nc)
    sd = AC.random_state_dict(spec, seed)
    A = torch.from_numpy(AC.skeleton_graph())
    clips = clips_like_root_norm(seed + 100, N_CLIPS, T, spec.K)
    ref64 = R.forward(spec, sd, A, clips, torch.float64)
    ref32 = R.forward(spec, sd, A, clips, torch.float32)
    return dict(spec=spec, sd=sd, A=A, T=T, clips=clips, ref64=ref64, ref32=ref32,
                E=float((ref32.double() - ref64).abs().max()))


def margins(logits):
    """Top-1 minus top-2 per clip, f64."""
    top = torch.topk(logits.double(), 2, dim=1).values
    return top[:, 0] - top[:, 1]


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def refusals(lib):
    """[(what, return code, expected)] of calls that must be refused before anything is launched (no GPU is touched)."""
    l = lib.load()
    p = 4096                                                    # a non-NULL, 16-byte aligned address nothing dereferences
    ok = dict(dtype=lib.PPN_F32, K=18, P=3, T=8, cin=16, cout=16, stride=1, residual=lib.PPN_STGCN_RES_NONE)
    out = []

    def gcn(**kw):
        d = lib.StgcnDesc(**dict(ok, **{k: v for k, v in kw.items() if k in ok}))
        return l.ppn_stgcn_gcn(C.byref(d), p, kw.get("w", p), p, p, p, p, kw.get("capacity", 64), p, None)

    def tcn(**kw):
        d = lib.StgcnDesc(**dict(ok, **{k: v for k, v in kw.items() if k in ok}))
        return l.ppn_stgcn_tcn(C.byref(d), p, kw.get("x", p), p, p, p, p, kw.get("capacity", 64), p, None)

    inv, uns = -1, -3                                           # PPN_E_INVALID, PPN_E_UNSUPPORTED
    for fn, f in (("gcn", gcn), ("tcn", tcn)):
        out += [(f"{fn} bf16", f(dtype=lib.PPN_BF16), uns), (f"{fn} f16", f(dtype=lib.PPN_F16), uns),
                (f"{fn} K 0", f(K=0), inv), (f"{fn} K 33", f(K=33), inv), (f"{fn} T 0", f(T=0), inv),
                (f"{fn} P 4", f(P=4), inv), (f"{fn} cout 24", f(cout=24), inv), (f"{fn} cout 272", f(cout=272), inv),
                (f"{fn} cin 8", f(cin=8), inv), (f"{fn} stride 3", f(stride=3), inv), (f"{fn} residual 3", f(residual=3), inv),
                (f"{fn} identity cin != cout", f(residual=lib.PPN_STGCN_RES_IDENTITY, cout=32), inv),
                (f"{fn} identity stride 2", f(residual=lib.PPN_STGCN_RES_IDENTITY, stride=2), inv),
                (f"{fn} capacity 0", f(capacity=0), inv), (f"{fn} capacity 65", f(capacity=65), inv)]
    out += [("gcn NULL w", gcn(w=None), inv), ("gcn misaligned w", gcn(w=p + 4), inv),
            ("tcn NULL x with a shortcut", tcn(x=None, residual=lib.PPN_STGCN_RES_PROJ, cout=32), inv),
            ("gcn NULL desc", l.ppn_stgcn_gcn(None, p, p, p, p, p, p, 64, p, None), inv)]
    d = lib.StgcnDesc(**ok)
    d16 = lib.StgcnDesc(**dict(ok, dtype=lib.PPN_F16))
    out += [("input f16", l.ppn_stgcn_input(C.byref(d16), p, p, p, 1, 1, p, p, p, p, p, p, None), uns),
            ("input 0 streams", l.ppn_stgcn_input(C.byref(d), p, p, p, 0, 1, p, p, p, p, p, p, None), inv),
            ("input NULL ids", l.ppn_stgcn_input(C.byref(d), p, None, p, 1, 1, p, p, p, p, p, p, None), inv),
            ("head f16", l.ppn_stgcn_head(C.byref(d16), 4, p, p, p, p, 1, p, p, None), uns),
            ("head 0 classes", l.ppn_stgcn_head(C.byref(d), 0, p, p, p, p, 1, p, p, None), inv),
            ("head 1025 classes", l.ppn_stgcn_head(C.byref(d), 1025, p, p, p, p, 1, p, p, None), inv),
            ("head NULL rank", l.ppn_stgcn_head(C.byref(d), 4, p, p, p, None, 1, p, p, None), inv)]
    return out
