"""Actions from skeleton clips on the device (no counterpart in the reference) over csrc/stgcn.hip: the forward pass of ST-GCN
(Yan, Xiong, Lin 2018: "Spatial Temporal Graph Convolutional Networks for Skeleton-Based Action Recognition"), one person per
clip, eval mode, on the ``ClipBatch`` that ``PoseClips.gather()`` wrote: exact f32, or opt-in ``compute_dtype="float16"`` over
csrc/stgcn16.hip -- IEEE half storage of activations, weights and adjacency, v_mfma_f32_16x16x32_f16 with f32 accumulation,
scales, shifts, classifier and logits in f32 (rules: ppn_stgcn16_* in include/ppn.h; restatement: tests/stgcn16_ref.py).
Conversions do not clamp: ``ActionModel.half_range_report(batch)`` tells whether a checkpoint's activations fit into half.

* ``skeleton_graph(edges, K, center)``        -- the "spatial" partition of the skeleton at hop 1, f32 [3, K, K] (NumPy).
* ``STGCNSpec`` / ``stgcn_spec(name, n)``     -- the network as data: blocks (cin, cout, stride, residual); "paper", "tiny".
* ``random_state_dict(spec, seed)``           -- weights under the key names of the public ST-GCN implementation, for tests.
* ``fold(spec, state_dict)``                  -- every BatchNorm and bias folded into scale and shift, in f64.
* ``pack_gcn16`` / ``pack_tcn16``                -- the half packed orders of ppn_stgcn16_gcn / ppn_stgcn16_tcn.
* ``ActionModel(spec, state_dict, streams, length)`` -- owns the folded, packed weights and every intermediate buffer for
                                                 streams * 64 clips; ``model(batch)`` is 2 + 2 x blocks launches on the
                                                 current stream -> ``ActionResult``; no allocation, no synchronisation,
                                                 no read-back, and it replays from a captured graph on any population.

The rules are include/ppn.h's (ppn_stgcn_*); tests/stgcn_ref.py restates the function from the unfolded state dict.  NO
trained checkpoint ships and NO CLAIM is made about recognition accuracy: the tests hold the arithmetic to the restatement
on random weights, nothing more.  Not built: bf16, two people per clip, training, softmax, MultiLaneInference
integration.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import config as cfg
from . import lib as L
from . import prng

RESIDUALS = {"none": L.PPN_STGCN_RES_NONE, "identity": L.PPN_STGCN_RES_IDENTITY, "proj": L.PPN_STGCN_RES_PROJ}
EPS = 1e-5
SLOTS = L.PPN_CLIP_SLOTS


# ---- the graph ----------------------------------------------------------------------------------------------------------------
def hop_to(edges, K: int, center: int) -> np.ndarray:
    """Hop distance of every joint to `center` over the undirected `edges` (unreachable: K)."""
    nb = [[] for _ in range(K)]
    for a, b in edges:
        nb[a].append(b)
        nb[b].append(a)
    hop = np.full(K, K, np.int64)
    hop[center], todo = 0, [center]
    while todo:
        v = todo.pop(0)
        for w in nb[v]:
            if hop[w] == K:
                hop[w] = hop[v] + 1
                todo.append(w)
    return hop


def skeleton_graph(edges=cfg.EDGES, K: int = cfg.K, center: int = cfg.KEYPOINT_NAMES.index("thorax")) -> np.ndarray:
    """f32 [3, K, K], indexed [part][v][w] for z[w] = sum_v x[v] A[v][w]: the adjacency with self-loops, column-normalised
    (A D^-1), split by the hop distance to `center`: part 0 the neighbours v as far from it as w (the self-loops are here),
    part 1 the neighbours closer to it than w, part 2 those farther."""
    adj = np.eye(K)
    for a, b in edges:
        if not (0 <= a < K and 0 <= b < K):
            raise ValueError(f"edge {(a, b)} outside 0..{K - 1}")
        adj[a, b] = adj[b, a] = 1.0
    norm = adj / adj.sum(axis=0, keepdims=True)
    hop = hop_to(edges, K, center)
    hv, hw = hop[:, None], hop[None, :]
    return np.stack([norm * (hv == hw), norm * (hv < hw), norm * (hv > hw)]).astype(np.float32)


# ---- the network as data ------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class STGCNSpec:
    blocks: Tuple[Tuple[int, int, int, str], ...]
    num_class: int
    K: int = cfg.K
    P: int = 3
    kt: int = 9

    def __post_init__(self):
        object.__setattr__(self, "blocks", tuple((int(a), int(b), int(s), str(r)) for a, b, s, r in self.blocks))
        if not self.blocks:
            raise ValueError("an STGCNSpec needs at least one block")
        if not 1 <= self.K <= L.PPN_MAX_KP:
            raise ValueError(f"K {self.K} outside 1..{L.PPN_MAX_KP}")
        if not 1 <= self.P <= L.PPN_STGCN_MAX_P or self.kt != 9:
            raise ValueError(f"P {self.P} outside 1..{L.PPN_STGCN_MAX_P} or kt {self.kt} != 9")
        if not 1 <= self.num_class <= L.PPN_STGCN_MAX_CLASS:
            raise ValueError(f"num_class {self.num_class} outside 1..{L.PPN_STGCN_MAX_CLASS}")
        prev = None
        for i, (cin, cout, stride, res) in enumerate(self.blocks):
            if cout % 16 or not 16 <= cout <= L.PPN_STGCN_MAX_C:
                raise ValueError(f"block {i}: cout {cout} must be a multiple of 16 up to {L.PPN_STGCN_MAX_C}")
            if cin != 3 and (cin % 16 or not 16 <= cin <= L.PPN_STGCN_MAX_C):
                raise ValueError(f"block {i}: cin {cin} must be 3 or a multiple of 16 up to {L.PPN_STGCN_MAX_C}")
            if prev is not None and cin != prev:
                raise ValueError(f"block {i}: cin {cin} does not follow {prev} channels")
            if stride not in (1, 2) or res not in RESIDUALS:
                raise ValueError(f"block {i}: stride {stride} must be 1 or 2, residual {res!r} one of {sorted(RESIDUALS)}")
            if res == "identity" and (cin != cout or stride != 1):
                raise ValueError(f"block {i}: an identity shortcut needs cin == cout and stride 1")
            prev = cout

    def lengths(self, T: int) -> List[int]:
        """Time steps at the input of every block and after the last."""
        out = [int(T)]
        for _, _, s, _ in self.blocks:
            out.append((out[-1] - 1) // s + 1)
        return out

    def flops(self, T: int) -> int:
        """Multiply-adds x 2 of one clip (graph aggregation, both convolutions, shortcuts, classifier)."""
        n, K, P = 0, self.K, self.P
        for (cin, cout, s, res), t in zip(self.blocks, self.lengths(T)):
            to = (t - 1) // s + 1
            n += 2 * t * K * (P * cin * K + P * cin * cout) + 2 * to * K * (9 * cout * cout + (cin * cout if res == "proj" else 0))
        return n + 2 * self.blocks[-1][1] * self.num_class


def stgcn_spec(name: str, num_class: int, K: int = cfg.K) -> STGCNSpec:
    if name == "paper":
        blocks = ([(3, 64, 1, "none")] + [(64, 64, 1, "identity")] * 3 + [(64, 128, 2, "proj")] + [(128, 128, 1, "identity")] * 2 +
                  [(128, 256, 2, "proj")] + [(256, 256, 1, "identity")] * 2)
    elif name == "tiny":
        blocks = [(3, 16, 1, "none"), (16, 16, 1, "identity"), (16, 32, 2, "proj"), (32, 32, 1, "identity")]
    else:
        raise ValueError(f"unknown preset {name!r}: 'paper' or 'tiny'")
    return STGCNSpec(tuple(blocks), num_class, K)


def _bn_keys(prefix: str, n: int):
    return [(f"{prefix}.{k}", (n,)) for k in ("weight", "bias", "running_mean", "running_var")]


def state_dict_keys(spec: STGCNSpec, with_A: bool = False) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of every tensor ``ActionModel`` reads, under the names of the public ST-GCN implementation."""
    K, P = spec.K, spec.P
    out = ([("A", (P, K, K))] if with_A else []) + _bn_keys("data_bn", K * 3)
    for i, (cin, cout, _, res) in enumerate(spec.blocks):
        b = f"st_gcn_networks.{i}"
        out += [(f"{b}.gcn.conv.weight", (P * cout, cin, 1, 1)), (f"{b}.gcn.conv.bias", (P * cout,))]
        out += _bn_keys(f"{b}.tcn.0", cout)
        out += [(f"{b}.tcn.2.weight", (cout, cout, 9, 1)), (f"{b}.tcn.2.bias", (cout,))]
        out += _bn_keys(f"{b}.tcn.3", cout)
        if res == "proj":
            out += [(f"{b}.residual.0.weight", (cout, cin, 1, 1)), (f"{b}.residual.0.bias", (cout,))]
            out += _bn_keys(f"{b}.residual.1", cout)
    out += [(f"edge_importance.{i}", (P, K, K)) for i in range(len(spec.blocks))]
    return out + [("fcn.weight", (spec.num_class, spec.blocks[-1][1], 1, 1)), ("fcn.bias", (spec.num_class,))]


def random_state_dict(spec: STGCNSpec, seed: int) -> Dict[str, "torch.Tensor"]:
    """A state dict of torch f32 tensors from prng: He-scaled convolutions, BatchNorm statistics away from the identity
    (running_var in [0.5, 2], means, biases and shifts non-zero), edge importances in [0.5, 1.5]."""
    import torch
    out = {}
    for i, (name, shape) in enumerate(state_dict_keys(spec)):
        n, s = int(np.prod(shape)), prng.stream_seed(seed, i)
        leaf = name.rsplit(".", 1)[1]
        if name.startswith("edge_importance"):
            v = prng.uniform(s, n, 0.5, 1.5)
        elif leaf == "running_var":
            v = prng.uniform(s, n, 0.5, 2.0)
        elif leaf == "running_mean" or leaf == "bias":
            v = prng.uniform(s, n, 0.1, 0.4) * np.where(prng.uniform01(s + 1, n) < 0.5, -1.0, 1.0).astype(np.float32)
        elif len(shape) == 1:                                         # a BatchNorm weight
            v = prng.uniform(s, n, 0.6, 1.4)
        else:
            fan = int(np.prod(shape[1:])) * (spec.P if ".gcn." in name else 1)
            v = prng.normalish(s, n) * np.float32((2.0 / fan) ** 0.5)
        out[name] = torch.from_numpy(np.ascontiguousarray(v, np.float32).reshape(shape))
    return out


# ---- folding (f64) ------------------------------------------------------------------------------------------------------------
def _f64(sd, name):
    t = sd[name]
    return (t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)).astype(np.float64)


def _bn(sd, prefix):
    """(scale, shift) of an eval-mode BatchNorm."""
    s = _f64(sd, prefix + ".weight") / np.sqrt(_f64(sd, prefix + ".running_var") + EPS)
    return s, _f64(sd, prefix + ".bias") - _f64(sd, prefix + ".running_mean") * s


def fold(spec: STGCNSpec, sd) -> dict:
    """Every BatchNorm and bias folded, f64: {"in": (scale, shift) [K*3], "blocks": [{adj [P,K,K], wg [P,cout,cin], s0 [cout],
    t0 [K,cout], wt [cout,cout,9], wr [cout,cin] or None (already times sr / s3), s3, t3 [cout]}], "wf" [c,num_class],
    "bf"}.  The gcn bias passes through the adjacency: t0[w][c] = s0[c] * sum_p b[p][c] * colsum_p[w] + shift0[c]."""
    K, P = spec.K, spec.P
    missing = [n for n, _ in state_dict_keys(spec) if n not in sd]
    if missing:
        raise KeyError(f"state dict lacks {missing[:4]}{' ...' if len(missing) > 4 else ''}")
    for n, shape in state_dict_keys(spec, "A" in sd):
        if tuple(sd[n].shape) != shape:
            raise ValueError(f"{n}: shape {tuple(sd[n].shape)}, expected {shape}")
    A = _f64(sd, "A") if "A" in sd else skeleton_graph(K=K).astype(np.float64) if K == cfg.K else None
    if A is None:
        raise ValueError(f"K = {K} is not the project's skeleton: the state dict must bring its own 'A' [{P}, {K}, {K}]")
    if A.shape[0] != P:
        raise ValueError(f"the graph has {A.shape[0]} parts, the spec {P}")
    blocks = []
    for i, (cin, cout, stride, res) in enumerate(spec.blocks):
        b = f"st_gcn_networks.{i}"
        adj = A * _f64(sd, f"edge_importance.{i}")
        wg = _f64(sd, b + ".gcn.conv.weight").reshape(P, cout, cin)
        bg = _f64(sd, b + ".gcn.conv.bias").reshape(P, cout)
        s0, h0 = _bn(sd, b + ".tcn.0")
        t0 = s0[None, :] * np.einsum("pc,pw->wc", bg, adj.sum(axis=1)) + h0[None, :]
        s3, h3 = _bn(sd, b + ".tcn.3")
        t3 = s3 * _f64(sd, b + ".tcn.2.bias") + h3
        wr = None
        if res == "proj":
            if (s3 == 0).any():
                raise ValueError(f"block {i}: a tcn.3 weight of exactly 0 cannot carry the projection shortcut")
            sr, hr = _bn(sd, b + ".residual.1")
            wr = _f64(sd, b + ".residual.0.weight").reshape(cout, cin) * (sr / s3)[:, None]
            t3 = t3 + sr * _f64(sd, b + ".residual.0.bias") + hr
        blocks.append(dict(cin=cin, cout=cout, stride=stride, residual=res, adj=adj, wg=wg, s0=s0, t0=t0,
                           wt=_f64(sd, b + ".tcn.2.weight").reshape(cout, cout, 9), wr=wr, s3=s3, t3=t3))
    c_last = spec.blocks[-1][1]
    return {"in": _bn(sd, "data_bn"), "blocks": blocks, "wf": _f64(sd, "fcn.weight").reshape(spec.num_class, c_last).T.copy(),
            "bf": _f64(sd, "fcn.bias")}


def gcn_folded(b: dict, x: np.ndarray) -> np.ndarray:
    """The graph convolution of a folded block as ppn_stgcn_gcn states it, in x's precision: x [n, t, v, cin]."""
    y = np.einsum("ntvi,pvw->ntwpi", x, b["adj"].astype(x.dtype))
    z = np.einsum("ntwpi,pci->ntwc", y, b["wg"].astype(x.dtype))
    return np.maximum(z * b["s0"].astype(x.dtype) + b["t0"].astype(x.dtype)[None, None], 0)


def tcn_folded(b: dict, u: np.ndarray, x: Optional[np.ndarray]) -> np.ndarray:
    """The temporal convolution of a folded block as ppn_stgcn_tcn states it: u [n, t, v, cout], x the block's input."""
    s, T = b["stride"], u.shape[1]
    To = (T - 1) // s + 1
    up = np.pad(u, ((0, 0), (4, 4), (0, 0), (0, 0)))
    wt = b["wt"].astype(u.dtype)
    z = sum(np.einsum("ntvi,ci->ntvc", up[:, k:k + (To - 1) * s + 1:s], wt[:, :, k]) for k in range(9))
    if b["residual"] == "proj":
        z = z + np.einsum("ntvi,ci->ntvc", x[:, ::s][:, :To], b["wr"].astype(u.dtype))
    z = z * b["s3"].astype(u.dtype) + b["t3"].astype(u.dtype)
    return np.maximum(z + x if b["residual"] == "identity" else z, 0)


def forward_folded(folded: dict, clips: np.ndarray) -> np.ndarray:
    """Logits [n, num_class] of clips [n, 3, T, K] from the folded parameters, in the clips' precision (f64 in the tests)."""
    dt = clips.dtype
    n, _, T, K = clips.shape
    sc, sh = (v.astype(dt).reshape(K, 3) for v in folded["in"])
    x = clips.transpose(0, 2, 3, 1) * sc[None, None] + sh[None, None]
    for b in folded["blocks"]:
        x = tcn_folded(b, gcn_folded(b, x), x)
    return x.mean(axis=(1, 2)) @ folded["wf"].astype(dt) + folded["bf"].astype(dt)


# ---- packing ------------------------------------------------------------------------------------------------------------------
def _pad_to(a: np.ndarray, axis: int, mult: int) -> np.ndarray:
    pad = [(0, 0)] * a.ndim
    pad[axis] = (0, -a.shape[axis] % mult)
    return np.pad(a, pad)


def pack_gcn(wg: np.ndarray) -> np.ndarray:
    """wg [P, cout, cin] -> f32 in the fragment order of ppn_stgcn_gcn: [ct][cc][p][g][col][j]."""
    w = _pad_to(wg, 2, 16)
    P, cout, cp = w.shape
    w = w.reshape(P, cout // 16, 16, cp // 16, 4, 4).transpose(1, 3, 0, 4, 2, 5)
    return np.ascontiguousarray(w, np.float32).reshape(-1)


def pack_tcn(wt: np.ndarray, wr: Optional[np.ndarray]) -> np.ndarray:
    """wt [cout, cout, 9] (and wr [cout, cin]) -> f32 in the fragment order of ppn_stgcn_tcn: [ct][cc][k][g][col][j], then
    [ct][rc][g][col][j]."""
    cout = wt.shape[0]
    w = wt.reshape(cout // 16, 16, cout // 16, 4, 4, 9).transpose(0, 2, 5, 3, 1, 4)
    parts = [np.ascontiguousarray(w, np.float32).reshape(-1)]
    if wr is not None:
        r = _pad_to(wr, 1, 16)
        r = r.reshape(cout // 16, 16, r.shape[1] // 16, 4, 4).transpose(0, 2, 3, 1, 4)
        parts.append(np.ascontiguousarray(r, np.float32).reshape(-1))
    return np.concatenate(parts)


def pack_gcn16(wg: np.ndarray) -> np.ndarray:
    """wg [P, cout, cin] f64 -> half in the fragment order of ppn_stgcn16_gcn: [ct][cc][p][g][col][j], 8 halves j per lane,
    the input channel cc * 32 + 8 g + j, zero past cin; every value rounded once from f64."""
    w = _pad_to(wg, 2, 32)
    P, cout, cp = w.shape
    w = w.reshape(P, cout // 16, 16, cp // 32, 4, 8).transpose(1, 3, 0, 4, 2, 5)
    return np.ascontiguousarray(w).astype(np.float16).reshape(-1)


def pack_tcn16(wt: np.ndarray, wr: Optional[np.ndarray]) -> np.ndarray:
    """wt [cout, cout, 9] (and wr [cout, cin]) f64 -> half in the fragment order of ppn_stgcn16_tcn: [ct][cc][k][g][col][j],
    then [ct][rc][g][col][j]; input channels in chunks of 32, zero past cout / cin."""
    cout = wt.shape[0]
    w = _pad_to(wt, 1, 32)
    w = w.reshape(cout // 16, 16, w.shape[1] // 32, 4, 8, 9).transpose(0, 2, 5, 3, 1, 4)
    parts = [np.ascontiguousarray(w).astype(np.float16).reshape(-1)]
    if wr is not None:
        r = _pad_to(wr, 1, 32)
        r = r.reshape(cout // 16, 16, r.shape[1] // 32, 4, 8).transpose(0, 2, 3, 1, 4)
        parts.append(np.ascontiguousarray(r).astype(np.float16).reshape(-1))
    return np.concatenate(parts)


DTYPES = {"float32": L.PPN_F32, "float16": L.PPN_F16}


def desc(K: int, P: int, T: int, cin: int, cout: int, stride: int, residual: str, dtype: int = L.PPN_F32) -> "L.StgcnDesc":
    return L.StgcnDesc(dtype, K, P, T, cin, cout, stride, RESIDUALS[residual])


class BlockWeights:
    """The device tensors of one folded block, in the layout the kernels read."""

    def __init__(self, b: dict, device, dtype: str = "float32"):
        import torch
        if dtype not in DTYPES:
            raise ValueError(f"dtype {dtype!r}: one of {sorted(DTYPES)}")
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)                 # noqa: E731
        self.dtype = dtype
        self.cin, self.cout, self.stride, self.residual = b["cin"], b["cout"], b["stride"], b["residual"]
        self.s0, self.t0, self.s3, self.t3 = dev(b["s0"]), dev(b["t0"]), dev(b["s3"]), dev(b["t3"])
        if dtype == "float16":                                        # one rounding from the f64 folded value to half
            h = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)                           # noqa: E731
            self.adj, self.wg = h(b["adj"].astype(np.float16)), h(pack_gcn16(b["wg"]))
            self.wt = h(pack_tcn16(b["wt"], b["wr"]))
        else:
            self.adj, self.wg, self.wt = dev(b["adj"]), dev(pack_gcn(b["wg"])), dev(pack_tcn(b["wt"], b["wr"]))


def _entry(d, w: BlockWeights, stage: str) -> str:
    """The entry point of `stage` for the descriptor's dtype; weights packed for the other mode are refused here."""
    if d.dtype != DTYPES[w.dtype]:
        raise ValueError(f"a descriptor of dtype {d.dtype} with weights packed for {w.dtype}")
    return ("ppn_stgcn16_" if d.dtype == L.PPN_F16 else "ppn_stgcn_") + stage


def launch_gcn(d, w: BlockWeights, x, n_active, capacity: int, out):
    name = _entry(d, w, "gcn")
    L.check(getattr(L.load(), name)(C.byref(d), x.data_ptr(), w.wg.data_ptr(), w.adj.data_ptr(), w.s0.data_ptr(),
                                    w.t0.data_ptr(), n_active.data_ptr(), capacity, out.data_ptr(), L.current_stream_ptr()),
            name)


def launch_tcn(d, w: BlockWeights, u, x, n_active, capacity: int, out):
    name = _entry(d, w, "tcn")
    L.check(getattr(L.load(), name)(C.byref(d), u.data_ptr(), x.data_ptr() if w.residual != "none" else None, w.wt.data_ptr(),
                                    w.s3.data_ptr(), w.t3.data_ptr(), n_active.data_ptr(), capacity, out.data_ptr(),
                                    L.current_stream_ptr()), name)


# ---- the public interface -----------------------------------------------------------------------------------------------------
@dataclass
class ActionResult:
    """Views of the ActionModel's buffers, all on the device; the next call overwrites them."""
    logits: "object"                 # f32 [S, 64, num_class]  class scores per slot, zeros for an inactive slot
    label: "object"                  # i32 [S, 64]             arg-max (lowest index on ties), -1 for an inactive slot
    active: "object"                 # i32 [S * 64]            the active slots s * 64 + i, ascending, then -1
    n_active: "object"               # i32 [1]
    ids: "object" = field(default=None, repr=False)   # i32 [S, 64]  the ClipBatch's track ids (for to_host)

    def to_host(self) -> List[Dict[int, Tuple[int, np.ndarray]]]:
        """The one read-back: per stream {track id: (label, logits [num_class])} of the active slots."""
        label, logits, ids = self.label.cpu().numpy(), self.logits.cpu().numpy(), self.ids.cpu().numpy()
        return [{int(ids[s, i]): (int(label[s, i]), logits[s, i].copy()) for i in range(label.shape[1]) if label[s, i] >= 0}
                for s in range(label.shape[0])]


class ActionModel:
    """ST-GCN over the clips of `streams` streams.

        clips = PoseClips(streams=1, frames=1, length=32, max_gap=tracker.cfg.max_age)
        actions = ActionModel(stgcn_spec("paper", 60), state_dict, streams=1, length=32)
        for frame in camera:
            res, tracks, rows, batch, act = rt.inference_batch_actions(frame, model, tracker, clips, actions, decoder)
            # act.label[0, i] is the class of track batch.ids[0, i], -1 while its clip is shorter than min_len

    `length` is the clips' T; a slot takes part iff it is live and holds at least `min_len` frames (default: a full clip)."""

    def __init__(self, spec: STGCNSpec, state_dict, streams: int, length: int, min_len: Optional[int] = None, device="cuda",
                 compute_dtype: str = "float32"):
        import torch
        if compute_dtype not in DTYPES:
            raise ValueError(f"compute_dtype {compute_dtype!r}: one of {sorted(DTYPES)}")
        self.compute_dtype = compute_dtype
        dt, half = DTYPES[compute_dtype], compute_dtype == "float16"
        if not 1 <= streams <= L.PPN_STGCN_MAX_STREAMS or not 1 <= length <= L.PPN_CLIP_MAX_LEN:
            raise ValueError(f"{streams} streams of clips of {length}: 1..{L.PPN_STGCN_MAX_STREAMS} and 1..{L.PPN_CLIP_MAX_LEN}")
        if spec.blocks[0][0] != 3:
            raise ValueError(f"the first block takes the clips' 3 planes, not {spec.blocks[0][0]} channels")
        self.spec, self.streams, self.length = spec, int(streams), int(length)
        self.min_len = self.length if min_len is None else int(min_len)
        self.capacity = cap = self.streams * SLOTS
        folded = fold(spec, state_dict)
        dev = torch.device(device)
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        K, T = spec.K, self.length
        self.scale, self.shift = (torch.from_numpy(v.astype(np.float32)).to(dev) for v in folded["in"])
        self.blocks = [BlockWeights(b, dev, compute_dtype) for b in folded["blocks"]]
        self.wf = torch.from_numpy(np.ascontiguousarray(folded["wf"], np.float32)).to(dev)
        self.bf = torch.from_numpy(folded["bf"].astype(np.float32)).to(dev)
        self.lengths = spec.lengths(T)
        self.descs = [desc(K, spec.P, t, cin, cout, s, res, dt) for (cin, cout, s, res), t in zip(spec.blocks, self.lengths)]
        self.d_in = desc(K, spec.P, T, 3, 16, 1, "none", dt)
        self.d_head = desc(K, spec.P, self.lengths[-1], spec.blocks[-1][1], spec.blocks[-1][1], 1, "none", dt)
        big = max(max(t * cout, to * cout) for (_, cout, _, _), t, to in zip(spec.blocks, self.lengths, self.lengths[1:]))
        act = dict(dtype=torch.float16 if half else torch.float32, device=dev)
        self.x0 = torch.zeros(cap * T * K * (4 if half else 3), **act)       # half rows carry a zero pad channel: 8 bytes
        self.u = torch.zeros(cap * big * K, **act)
        self.y = [torch.zeros(cap * big * K, **act) for _ in range(2 if len(spec.blocks) > 1 else 1)]
        self.active = torch.full((cap,), -1, **i32)
        self.rank = torch.full((cap,), -1, **i32)
        self.n_active = torch.zeros(1, **i32)
        self.logits = torch.zeros(self.streams, SLOTS, spec.num_class, **f32)
        self.label = torch.full((self.streams, SLOTS), -1, **i32)
        self.device = self.x0.device

    def __call__(self, batch) -> ActionResult:
        """ppn_stgcn_input, per block ppn_stgcn_gcn and ppn_stgcn_tcn, ppn_stgcn_head on the current stream."""
        import torch
        from .validate import _dense
        dev, S, T, K = self.device, self.streams, self.length, self.spec.K
        if dev.type != "cuda":
            raise ValueError("ActionModel runs on the device: its buffers live on " + str(dev))
        _dense("batch.x", batch.x, (S, SLOTS, 3, T, K), torch.float32, dev)
        _dense("batch.ids", batch.ids, (S, SLOTS), torch.int32, dev)
        _dense("batch.length", batch.length, (S, SLOTS), torch.int32, dev)
        lib, st = L.load(), L.current_stream_ptr()
        pre = "ppn_stgcn16_" if self.compute_dtype == "float16" else "ppn_stgcn_"
        L.check(getattr(lib, pre + "input")(C.byref(self.d_in), batch.x.data_ptr(), batch.ids.data_ptr(), batch.length.data_ptr(),
                                            S, self.min_len, self.scale.data_ptr(), self.shift.data_ptr(),
                                            self.active.data_ptr(), self.n_active.data_ptr(), self.rank.data_ptr(),
                                            self.x0.data_ptr(), st), pre + "input")
        cur = self.x0
        for i, (d, w) in enumerate(zip(self.descs, self.blocks)):
            out = self.y[i % len(self.y)]
            launch_gcn(d, w, cur, self.n_active, self.capacity, self.u)
            launch_tcn(d, w, self.u, cur, self.n_active, self.capacity, out)
            cur = out
        L.check(getattr(lib, pre + "head")(C.byref(self.d_head), self.spec.num_class, cur.data_ptr(), self.wf.data_ptr(),
                                           self.bf.data_ptr(), self.rank.data_ptr(), S, self.logits.data_ptr(),
                                           self.label.data_ptr(), st), pre + "head")
        return ActionResult(self.logits, self.label, self.active, self.n_active, batch.ids)

    def half_range_report(self, batch) -> dict:
        """A debugging aid that SYNCHRONISES: runs the call stage by stage and returns {"tensors": {name: largest |value|
        over the active clips} for "x0" and every block's "block<i>.u" and "block<i>.out", "finite": whether all of them are
        finite, "limit": 65504.0}.  How a user with a real checkpoint learns that half does not fit: a stored value beyond
        65504 is inf (the conversions do not clamp).  It reads the buffers the call itself uses; the result of the call is
        left in place as after ``model(batch)``."""
        import torch
        self(batch)                                                  # validates the batch, writes x0 and n_active
        torch.cuda.synchronize(self.device)
        n, K = int(self.n_active.item()), self.spec.K
        peak = lambda t, m: float(t[:m].float().abs().max()) if m else 0.0                               # noqa: E731
        out = {"x0": peak(self.x0, n * self.length * K * (4 if self.compute_dtype == "float16" else 3))}
        cur = self.x0
        for i, (d, w) in enumerate(zip(self.descs, self.blocks)):   # the buffers alternate: each stage is read before reuse
            dst = self.y[i % len(self.y)]
            launch_gcn(d, w, cur, self.n_active, self.capacity, self.u)
            out[f"block{i}.u"] = peak(self.u, n * self.lengths[i] * K * w.cout)
            launch_tcn(d, w, self.u, cur, self.n_active, self.capacity, dst)
            out[f"block{i}.out"] = peak(dst, n * self.lengths[i + 1] * K * w.cout)
            cur = dst
        torch.cuda.synchronize(self.device)
        finite = all(np.isfinite(v) for v in out.values())
        return {"tensors": out, "finite": bool(finite), "limit": 65504.0}
