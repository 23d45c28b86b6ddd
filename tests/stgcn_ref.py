"""ST-GCN's forward pass restated from the UNFOLDED state dict with F.batch_norm, F.conv2d and torch.einsum on the CPU, in f64
or f32, as the public implementation writes it (one person per clip, eval mode).  Shares no code with actions.py's folding;
tests/test_actions_cpu.py holds the two against each other.  Tensors here are [n, c, t, v] like the original.

`fault` plants one deliberate mistake, for the tests that show the bounds see it:
    "tap"        the temporal tap k = 2 is dropped           "neighbour"  taps outside a clip read the neighbouring clip
    "transpose"  the adjacency is transposed                 "importance" the edge importance is ignored
    "bias"       the gcn bias is added after the adjacency   "residual"   the shortcut is dropped
    "stride"     t' is one too few under stride 2 (the last output step repeats the one before)
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

EPS = 1e-5


def _p(sd, name, dt):
    return sd[name].to(dt)


def _bn(sd, prefix, x):
    dt = x.dtype
    return F.batch_norm(x, _p(sd, prefix + ".running_mean", dt), _p(sd, prefix + ".running_var", dt),
                        _p(sd, prefix + ".weight", dt), _p(sd, prefix + ".bias", dt), False, 0.0, EPS)


def data_bn(sd, clips):
    """clips [n, 3, t, v] -> x0 [n, 3, t, v]: BatchNorm1d over the channels v * 3 + c."""
    n, c, t, v = clips.shape
    x = clips.permute(0, 3, 1, 2).reshape(n, v * c, t)
    return _bn(sd, "data_bn", x).reshape(n, v, c, t).permute(0, 2, 3, 1)


def gcn(sd, i, P, A, x, fault=None):
    """relu(bn0(graph convolution)) of block i: x [n, cin, t, v] -> [n, cout, t, v]."""
    dt = x.dtype
    b = f"st_gcn_networks.{i}"
    adj = A.to(dt) * (1.0 if fault == "importance" else _p(sd, f"edge_importance.{i}", dt))
    if fault == "transpose":
        adj = adj.transpose(1, 2)
    w, bias = _p(sd, b + ".gcn.conv.weight", dt), _p(sd, b + ".gcn.conv.bias", dt)
    g = F.conv2d(x, w, None if fault == "bias" else bias)
    n, kc, t, v = g.shape
    g = g.view(n, P, kc // P, t, v)
    z = torch.einsum("nkctv,kvw->nctw", g, adj)
    if fault == "bias":
        z = z + bias.view(P, kc // P).sum(0).view(1, -1, 1, 1)
    return F.relu(_bn(sd, b + ".tcn.0", z))


def tcn(sd, i, stride, residual, u, x, fault=None):
    """relu(bn3(conv9x1(u)) + res(x)) of block i: u [n, cout, t, v], x [n, cin, t, v] -> [n, cout, t', v]."""
    dt = u.dtype
    b = f"st_gcn_networks.{i}"
    w, bias = _p(sd, b + ".tcn.2.weight", dt), _p(sd, b + ".tcn.2.bias", dt)
    if fault == "tap":
        w = w.clone()
        w[:, :, 2] = 0
    if fault == "neighbour":                                 # the clips back to back along t, as they lie in memory
        n, c, t, v = u.shape
        flat = u.permute(1, 0, 2, 3).reshape(1, c, n * t, v)
        y = F.conv2d(flat, w, bias, (1, 1), (4, 0)).reshape(c, n, t, v).permute(1, 0, 2, 3)[:, :, ::stride]
    else:
        y = F.conv2d(u, w, bias, (stride, 1), (4, 0))
    if fault == "stride" and stride == 2 and y.shape[2] > 1:
        y = torch.cat([y[:, :, :-1], y[:, :, -2:-1]], 2)
    y = _bn(sd, b + ".tcn.3", y)
    if fault != "residual":
        if residual == "identity":
            y = y + x
        elif residual == "proj":
            r = F.conv2d(x, _p(sd, b + ".residual.0.weight", dt), _p(sd, b + ".residual.0.bias", dt), (stride, 1))
            y = y + _bn(sd, b + ".residual.1", r)
    return F.relu(y)


def forward(spec, sd, A, clips, dtype=torch.float64, fault=None, fault_block=None):
    """Logits [n, num_class] of clips [n, 3, T, K] (any float tensor).  `A` [P, K, K]: the graph (sd["A"] if the dict has one).
    `fault` is planted in block `fault_block` (None: every block)."""
    A = sd["A"] if "A" in sd else A
    x = data_bn(sd, clips.to(dtype))
    for i, (cin, cout, stride, residual) in enumerate(spec.blocks):
        f = fault if fault_block in (None, i) else None
        x = tcn(sd, i, stride, residual, gcn(sd, i, spec.P, A, x, f), x, f)
    pooled = x.mean(dim=(2, 3), keepdim=True)
    return F.conv2d(pooled, _p(sd, "fcn.weight", dtype), _p(sd, "fcn.bias", dtype)).flatten(1)
