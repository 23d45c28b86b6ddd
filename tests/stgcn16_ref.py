"""The float16 mode of the action model (ppn_stgcn16_* in include/ppn.h) restated on its own, on the CPU: its own fold of the
UNFOLDED state dict in f64 (nothing is taken from actions.py), operands rounded ONCE to IEEE half at exactly the points the
header lists, and the evaluation in f64 or, for comparison, in f32 arithmetic.  Tensors are [n, c, t, v] like tests/stgcn_ref.py.

Rounded to half (`rh`, NumPy's direct round-to-nearest-even conversion; torch's f64 -> f16 goes through f32):
    the adjacency x edge importance, W, Wt, Wr' = Wr sr / s3          from their f64 folded values
    x0 = fma(x, scale, shift); y = sum_v x A; the gcn's output; the tcn's output
Not rounded: the scale and shift tables (f32 on the device), the classifier, the logits.  `exact=True` leaves out the roundings
of y and of the outputs: that is the stage REFERENCE of tests/stgcn16_cases.py, whose bounds carry those roundings as terms.

A folded block is a dict with the keys of actions.fold's blocks (cin, cout, stride, residual, adj, wg, s0, t0 [K, cout], wt, wr,
s3, t3; f64 NumPy, NOT yet rounded), so that a hand-made block can go to the kernels and to this file alike.

`fault` plants the mistakes of tests/stgcn_ref.py ("tap", "neighbour", "transpose", "importance", "bias", "residual", "stride").
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5


def rh(t):
    """One rounding to IEEE half (nearest even, no clamp: beyond 65504 -> inf), returned in t's own type."""
    if isinstance(t, np.ndarray):
        with np.errstate(over="ignore"):
            return t.astype(np.float16).astype(t.dtype)
    with np.errstate(over="ignore"):
        return torch.from_numpy(t.detach().numpy().astype(np.float16)).to(t.dtype)


def _np(sd, name):
    return sd[name].detach().double().numpy()


def _bn(sd, prefix):
    s = _np(sd, prefix + ".weight") / np.sqrt(_np(sd, prefix + ".running_var") + EPS)
    return s, _np(sd, prefix + ".bias") - _np(sd, prefix + ".running_mean") * s


def fold_block(sd, i, P, A, block, fault=None):
    """Block i = (cin, cout, stride, residual) folded in f64.  A: f64 NumPy [P, K, K]."""
    cin, cout, stride, residual = block
    b = f"st_gcn_networks.{i}"
    adj = A.copy() if fault == "importance" else A * _np(sd, f"edge_importance.{i}")
    if fault == "transpose":
        adj = adj.transpose(0, 2, 1).copy()
    wg = _np(sd, b + ".gcn.conv.weight").reshape(P, cout, cin)
    bg = _np(sd, b + ".gcn.conv.bias").reshape(P, cout)
    s0, h0 = _bn(sd, b + ".tcn.0")
    through = np.ones((P, adj.shape[2])) if fault == "bias" else adj.sum(axis=1)        # [p][w]
    t0 = s0[None, :] * np.einsum("pc,pw->wc", bg, through) + h0[None, :]
    wt = _np(sd, b + ".tcn.2.weight").reshape(cout, cout, 9).copy()
    if fault == "tap":
        wt[:, :, 2] = 0
    s3, h3 = _bn(sd, b + ".tcn.3")
    t3 = s3 * _np(sd, b + ".tcn.2.bias") + h3
    wr = None
    if fault == "residual":
        residual = "none"
    if residual == "proj":
        sr, hr = _bn(sd, b + ".residual.1")
        wr = _np(sd, b + ".residual.0.weight").reshape(cout, cin) * (sr / s3)[:, None]
        t3 = t3 + sr * _np(sd, b + ".residual.0.bias") + hr
    return dict(cin=cin, cout=cout, stride=stride, residual=residual, adj=adj, wg=wg, s0=s0, t0=t0, wt=wt, wr=wr, s3=s3, t3=t3)


def _t(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def gcn16(b, x, dt=torch.float64, exact=False):
    """x [n, cin, t, v] (values a half holds) -> [n, cout, t, v] in dt."""
    adj, wg = _t(rh(b["adj"]), dt), _t(rh(b["wg"]), dt)
    y = torch.einsum("nitv,pvw->npitw", x.to(dt), adj)
    if not exact:
        y = rh(y)
    z = torch.einsum("npitw,pci->nctw", y, wg)
    o = F.relu(z * _t(b["s0"], dt).view(1, -1, 1, 1) + _t(b["t0"], dt).t().unsqueeze(0).unsqueeze(2))
    return o if exact else rh(o)


def tcn16(b, u, x, dt=torch.float64, exact=False, fault=None):
    """u [n, cout, t, v], x [n, cin, t, v] (values a half holds) -> [n, cout, t', v] in dt."""
    s = b["stride"]
    w = _t(rh(b["wt"]), dt).unsqueeze(-1)                      # [cout, cout, 9, 1]
    u = u.to(dt)
    if fault == "neighbour":                                   # the clips back to back along t, as they lie in memory
        n, c, t, v = u.shape
        flat = u.permute(1, 0, 2, 3).reshape(1, c, n * t, v)
        z = F.conv2d(flat, w, None, (1, 1), (4, 0)).reshape(-1, n, t, v).permute(1, 0, 2, 3)[:, :, ::s]
    else:
        z = F.conv2d(u, w, None, (s, 1), (4, 0))
    if fault == "stride" and s == 2 and z.shape[2] > 1:
        z = torch.cat([z[:, :, :-1], z[:, :, -2:-1]], 2)
    if b["residual"] == "proj":
        z = z + F.conv2d(x.to(dt), _t(rh(b["wr"]), dt).view(b["cout"], b["cin"], 1, 1), None, (s, 1))
    o = z * _t(b["s3"], dt).view(1, -1, 1, 1) + _t(b["t3"], dt).view(1, -1, 1, 1)
    if b["residual"] == "identity":
        o = o + x.to(dt)
    o = F.relu(o)
    return o if exact else rh(o)


def forward16(spec, sd, A, clips, dt=torch.float64, fault=None, fault_block=None):
    """Logits [n, num_class] in dt of clips [n, 3, T, K] in the float16 mode."""
    A = (sd["A"] if "A" in sd else A).detach().double().numpy()
    n, _, T, K = clips.shape
    sc, sh = (_t(v.reshape(K, 3).T.copy(), dt).view(1, 3, 1, K) for v in _bn(sd, "data_bn"))       # channel v * 3 + c
    x = rh(clips.to(dt) * sc + sh)
    for i, block in enumerate(spec.blocks):
        f = fault if fault_block in (None, i) else None
        b = fold_block(sd, i, spec.P, A, block, f)
        x = tcn16(b, gcn16(b, x, dt), x, dt, fault=f)
    pooled = x.mean(dim=(2, 3))
    wf = sd["fcn.weight"].detach().to(dt).view(spec.num_class, -1)
    return pooled @ wf.t() + sd["fcn.bias"].detach().to(dt)
