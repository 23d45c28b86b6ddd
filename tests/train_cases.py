"""Edge cases for the streaming training kernels of csrc/train.hip (train-mode BatchNorm forward / backward, its forward-mode
tangent and the dual backward, Adam, GradNorm's five weights, the pointwise tails), their closed-form f64 references and the
error bounds the GPU results are held to.  Plain helper module (no tests, no GPU, no import of the library):
tests/test_train_edges_cpu.py checks that the references are right, that every case reaches the path it is for and that the
bounds notice defects; tests/test_train_edges_gpu.py runs the kernels.

Layout: a BatchNorm operand is [P, C] (pixels x channels, channels last) -- what the kernels see of any NHWC tensor.
References take the ALREADY ROUNDED f32 / bf16 operands (eps and momentum as the f32 values the kernels receive, leaky-ReLU's
slope as float(0.1f)) and do everything else in f64, in closed form (no autograd: the block-cap cases have 16.8 M elements).
References and operands are computed once per case and shared: callers must not modify what they get.

Bounds are functions of the f64 intermediates, in units of u = 2^-24 (one f32 rounding is at most u relative), with a small
integer K per output that counts the f32 roundings on the kernel's path (the count stands next to each constant).  They are
first-order worst cases: no constant was fitted to what a kernel returns.  A 16-bit output adds 2^-8 |ref| per rounding to
bf16 (a bf16 value just above a power of two is up to 2^-8 of itself away from the f32 value it rounds: the project's
per-element rule, profiles/backward_edge_errors.txt), so a bf16 ratio close to 1 is that one rounding.
"""
from __future__ import annotations

import functools
import types

import numpy as np
import torch

U = 2.0 ** -24
BF = 2.0 ** -8
LRELU = float(np.float32(0.1))                       # act_fwd / act_slope multiply by 0.1f
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
ACTS = ("none", "relu", "lrelu")
K_THREADS, K_MAX_BLOCKS = 256, 1024


# ---- make_slab restated (train.hip): how the pixel rows are dealt to work-groups ------------------------------------------------

def make_slab(C, P):
    """cc chunk columns of 8 channels, rpi pixel rows per iteration of one work-group, nb_want work-groups for 8 rows per
    thread, nb after the cap, slab rows per work-group (a multiple of rpi), nblocks recounted from the rounded slab."""
    assert 8 <= C <= 2048 and C & (C - 1) == 0 and P > 0
    cc = C // 8
    rpi = K_THREADS // cc
    nb_want = (P + rpi * 8 - 1) // (rpi * 8)
    nb = max(1, min(nb_want, K_MAX_BLOCKS))
    slab = (P + nb - 1) // nb
    slab = (slab + rpi - 1) // rpi * rpi
    return types.SimpleNamespace(cc=cc, rpi=rpi, nb_want=nb_want, nb=nb, slab=slab, nblocks=(P + slab - 1) // slab)


# ---- activation -----------------------------------------------------------------------------------------------------------------

def _slope(pos, act):
    if act == "none":
        return None
    return torch.where(pos, 1.0, 0.0 if act == "relu" else LRELU).double()


def _dslope(act):
    """|slope(z > 0) - slope(z <= 0)|: what one element on the wrong side of the kink changes."""
    return {"none": 0.0, "relu": 1.0, "lrelu": 1.0 - LRELU}[act]


def _mul(a, s):
    return a if s is None else a * s


# ---- BatchNorm: reference ---------------------------------------------------------------------------------------------------

def bn_ref(x, gamma, beta, rm=None, rv=None, eps=1e-5, momentum=0.1, act="none", dy=None, add=None, branch=None):
    """y = act(batch_norm(x)) with batch statistics, the running statistics, and (with dy) dgamma, dbeta, dx [+ add].
    nn.BatchNorm2d semantics; a single pixel (n == 1) takes the kernel's documented guard, an unbiased factor of 1 --
    nn.BatchNorm2d refuses that case in train mode ("Expected more than 1 value per channel"), so there is nothing to copy.
    branch: bool [P, C], the side of the kink every element is on (default z > 0, the kernels' rule: the kink itself has the
    slope of the negative side)."""
    r = types.SimpleNamespace(act=act)
    r.x = x64 = x.double()
    n = r.n = x64.shape[0]
    r.gamma, r.beta = gamma.double(), beta.double()
    r.eps, r.mom = float(np.float32(eps)), float(np.float32(momentum))
    r.mean = x64.mean(0)
    r.xc = x64 - r.mean
    r.var = (r.xc * r.xc).mean(0)
    r.rstd = 1.0 / torch.sqrt(r.var + r.eps)
    r.sc = r.gamma * r.rstd
    r.xhat = r.xc * r.rstd
    r.z = r.xc * r.sc + r.beta
    r.pos = (r.z > 0) if branch is None else branch
    r.slope = _slope(r.pos, act)
    r.y = _mul(r.z, r.slope)
    if rm is not None:
        unbiased = r.var * (n / (n - 1.0) if n > 1 else 1.0)
        r.rm_old, r.rm_new = (1.0 - r.mom) * rm.double(), r.mom * r.mean
        r.rv_old, r.rv_new = (1.0 - r.mom) * rv.double(), r.mom * unbiased
        r.rm, r.rv = r.rm_old + r.rm_new, r.rv_old + r.rv_new
    if dy is not None:
        r.dy = dy.double()
        r.g = _mul(r.dy, r.slope)
        _backward(r, r, r.g)
        r.add = None if add is None else add.double()
        r.dx_add = None if add is None else r.dx + r.add
    return r


def _backward(r, o, g):
    """The BatchNorm backward of the adjoint g (already through the activation) into o: dbeta, dgamma, dx, and the three
    coefficients of the kernels' form dx = ca*g + cb*x + cc, cc in its two parts (bn_bwd_finalize_kernel)."""
    n = r.n
    o.dbeta = g.sum(0)
    o.dgamma = (g * r.xhat).sum(0)
    o.dx = r.sc * (g - o.dbeta / n - r.xhat * (o.dgamma / n))
    o.cb = -r.gamma * r.rstd ** 2 * o.dgamma / n
    o.cc1 = r.gamma * r.rstd ** 2 * r.mean * o.dgamma / n
    o.cc2 = -r.sc * o.dbeta / n


# ---- BatchNorm: bounds ------------------------------------------------------------------------------------------------------
# Roundings of the per-channel constants, shared by every count below:
#   rstd = 1/sqrtf((float)var + eps): the cast and the sum each move var by u (u/2 each in rstd), sqrtf and the division are
#   correctly rounded (u each): 3u.   mean -> f32: u.
KF = 4     # forward, set by the issue: on |mean*sc| the roundings of mean, mean*sc, shift = beta - mean*sc and of x*sc (or of
           # the fused x*sc + shift) are 4; an error of sc itself (rstd 3 + the product gamma*rstd 1 = 4) multiplies (x - mean)*sc
           # only.  All of them at their maximum with one sign, plus the last rounding, would be 5 on a centred channel; an f32
           # emulation stays below 0.36 of this bound from mean/sigma = 0 to 1000, and an FMA only removes a rounding.
K_MEAN = 2      # f64 sums, one rounding to f32; the issue's allowance is 2
K_RSTD = 4      # 3 as counted above; the issue's allowance is 4
K_RUN = 4       # (1 - momentum) in f32, its product, the sum: 3 on the old term; mean (or var) -> f32, its product, the sum:
                # 3 on the new one; the issue's allowance is 4
K_DBETA = 2     # the f32 product dy * 0.1f, the final rounding of the f64 sum
K_XHAT = 6      # xhat = (x - (float)mean) * rstd per element, in units of u (|x| + |mean|) rstd: mean 1, the subtraction 1,
                # rstd 3, the product 1
K_DGAMMA = K_XHAT + 2   # ... + the f32 product dy * 0.1f + the final rounding of the f64 sum = 8
K_DX = 11       # dx = ca*g + cb*x + cc (+ add), all f32.  cb*x, the largest count: cb = -gamma rstd^2 dgamma / n has rstd twice
                # (6) and its own rounding (1), then the product (1) and three additions (3) = 11.  ca*g: 4 + 1 (g) + 1 + 3 = 9;
                # cc's mean part: 6 + 1 (mean) + 1 + 2 = 10, its dbeta part 3 + 1 + 2 = 6; add: 1.  One K for all five.
K_DUAL = 13     # dx += k0*xhat + k1*q + k2*xdot + k3: a coefficient 6 (rstd twice) + 1, q = dyt * 0.1f 1, the product 1, four
                # additions 4 = 13; xhat's own error is carried separately (K_XHAT)


def _cached(r, name, fn):
    """Per-element helpers shared by several bounds (|x|, |xhat|, ...), computed once per reference."""
    if not hasattr(r, name):
        setattr(r, name, fn())
    return getattr(r, name)


def _ax(r):
    return _cached(r, "_ax", lambda: r.x.abs())


def _axh(r):
    return _cached(r, "_axh", lambda: r.xhat.abs())


def _bz(r):
    """The forward bound on z: Kf u (|x*sc| + |mean*sc| + |beta|)."""
    return _cached(r, "_bz", lambda: (_ax(r) * (KF * U * r.sc.abs())).add_(KF * U * ((r.mean * r.sc).abs() + r.beta.abs())))


def ambiguous(r):
    """bool [P, C] or None: |z_ref| is below the forward bound on z, so the kernels may sit on either side of the kink.
    Channels with gamma == 0 and beta == 0 have z == 0 exactly, in the reference and in every kernel: never ambiguous."""
    if r.act == "none":
        return None
    amb = r.z.abs() < _bz(r)
    amb[:, (r.gamma == 0) & (r.beta == 0)] = False
    return amb


def _lo(b, ref, lo, times=1):
    """+ 2^-8 |ref| per rounding to bf16."""
    return b.add(ref.abs(), alpha=times * BF) if lo else b


def forward_bounds(r, lo):
    b = {}
    b["mean"] = K_MEAN * U * r.mean.abs()
    b["rstd"] = K_RSTD * U * r.rstd
    b["y"] = _lo(_bz(r), r.y, lo)
    if hasattr(r, "rm"):
        b["rm"] = K_RUN * U * (r.rm_old.abs() + r.rm_new.abs())
        b["rv"] = K_RUN * U * (r.rv_old.abs() + r.rv_new.abs())
    return b


def _amb_sum(amb, *factors):
    """sum over the ambiguous elements of |product of the factors|, per channel (there are few of them: gathered)."""
    rows, cols = amb.nonzero(as_tuple=True)
    v = torch.ones(rows.numel(), dtype=torch.float64)
    for f in factors:
        v = v * f[rows, cols].abs()
    return torch.zeros(amb.shape[1], dtype=torch.float64).index_add_(0, cols, v)


def _sum_bounds(r, g, amb, adj, lrelu=None):
    """Bounds on sum g and sum g*xhat as the kernels form them (f32 terms, f64 sums), without the final rounding to f32;
    also returns sum |g| and sum |g| (|x| + |mean|) rstd.  amb / adj: the ambiguous elements and the adjoint before the
    activation there (their slope may be the other one).  lrelu: whether g carries the f32 product with 0.1f."""
    lre = U if (r.act == "lrelu" if lrelu is None else lrelu) else 0.0
    ga = g.abs()
    s_g = ga.sum(0)
    s_gx = ((ga * _ax(r)).sum(0) + s_g * r.mean.abs()) * r.rstd
    e_s = lre * s_g
    e_sx = (K_XHAT * U + lre) * s_gx                     # |g xhat| <= |g| (|x| + |mean|) rstd
    if amb is not None:
        e_s = e_s + _dslope(r.act) * _amb_sum(amb, adj)
        e_sx = e_sx + _dslope(r.act) * _amb_sum(amb, adj, r.xhat)
    return e_s, e_sx, s_g, s_gx, ga


def _backward_bounds(r, o, g, amb, adj, lrelu=None):
    """(dbeta, dgamma, dx without add / 16-bit terms) for the backward o of the adjoint g.  dbeta and dgamma carry K_DBETA /
    K_DGAMMA in total; dx adds the image of their errors through cb and cc.  Per element the dx bound is
    A_c |g| + B_c |x| + D_c with per-channel A, B, D."""
    e_s, e_sx, s_g, s_gx, ga = _sum_bounds(r, g, amb, adj, lrelu)
    lre = 1 if (r.act == "lrelu" if lrelu is None else lrelu) else 0
    b_db = e_s + U * s_g * (K_DBETA - lre)
    b_dg = e_sx + U * s_gx * (K_DGAMMA - K_XHAT - lre)
    k = r.gamma.abs() * r.rstd / r.n
    img = k * r.rstd * e_sx                              # dgamma's error through cb (times |x|) and cc (times |mean|)
    b_dx = ga.mul_(K_DX * U * r.sc.abs()).addcmul_(_ax(r), K_DX * U * o.cb.abs() + img)
    b_dx.add_(K_DX * U * (o.cc1.abs() + o.cc2.abs()) + img * r.mean.abs() + k * e_s)
    return b_db, b_dg, b_dx


def backward_bounds(r, lo, amb=None):
    b = {}
    b["dbeta"], b["dgamma"], core = _backward_bounds(r, r, r.g, amb, r.dy)
    b["dx"] = _lo(core, r.dx, lo)
    if r.add is not None:
        b["dx_add"] = _lo(core.add(r.add.abs(), alpha=K_DX * U), r.dx_add, lo)
    return b


# ---- tangent and dual backward ----------------------------------------------------------------------------------------------

def bn_dual_ref(r, xdot, dyt=None):
    """r: bn_ref(..., dy=dy) of the same x.  The forward-mode tangent of y = act(bn(x)) for the input tangent xdot,
        ydot = act'(z) * gamma*rstd * (xdot - mean(xdot) - xhat*mean(xdot*xhat)),
    and (with dyt) the adjoint of the pair (y, ydot) for the adjoints (dy, dyt): dx, dxdot, dgamma, dbeta, by the formulas in
    the comments of bn_dual_finalize_kernel:
        q = dyt*act'(z);  Sq, Sqx = sum q*xhat, Sx = sum xdot, Sxx = sum xdot*xhat, Sqd = sum q*xdot;  m1, m2, qb = Sx, Sxx, Sq / n
        A = Sqd - Sq*Sx/n - Sqx*Sxx/n;  k0 = -gamma*rstd^2
        dx += k0*[A*xhat/n + m2*(q - qb - xhat*Sqx/n) + (Sqx/n)*(xdot - m1 - xhat*m2)],  dgamma += A*rstd."""
    d = types.SimpleNamespace()
    n = r.n
    d.xdot = xdot.double()
    d.jvp = types.SimpleNamespace()
    _backward(r, d.jvp, d.xdot)                       # the tangent of BN IS its backward formula (train.bn_tangent)
    d.tan = _mul(d.jvp.dx, r.slope)
    if dyt is None:
        return d
    d.dyt = dyt.double()
    d.q = _mul(d.dyt, r.slope)
    d.bdot = types.SimpleNamespace()
    _backward(r, d.bdot, d.q)
    d.dxdot = d.bdot.dx
    d.Sq, d.Sqx = d.q.sum(0), (d.q * r.xhat).sum(0)
    d.Sx, d.Sxx, d.Sqd = d.xdot.sum(0), (d.xdot * r.xhat).sum(0), (d.q * d.xdot).sum(0)
    m1, m2, qb = d.Sx / n, d.Sxx / n, d.Sq / n
    d.A = d.Sqd - d.Sq * d.Sx / n - d.Sqx * d.Sxx / n
    d.k0 = -r.gamma * r.rstd ** 2
    d.c0 = d.k0 * (d.A / n - 2.0 * m2 * d.Sqx / n)
    d.c1, d.c2 = d.k0 * m2, d.k0 * d.Sqx / n
    d.c3 = d.k0 * (-m2 * qb - d.Sqx / n * m1)
    d.dual = d.c0 * r.xhat + d.c1 * d.q + d.c2 * d.xdot + d.c3
    d.dx = r.dx + d.dual
    d.dg_tan = d.A * r.rstd
    d.dgamma, d.dbeta = r.dgamma + d.dg_tan, r.dbeta
    return d


def tangent_bounds(r, d, lo):
    """train.bn_tangent: the backward kernels on xdot without activation (stored once in the tensor's type), then
    ppn_bn_act_mask (the f32 product with 0.1f, stored again)."""
    _, _, core = _backward_bounds(r, d.jvp, d.xdot, None, None, lrelu=False)
    b = _mul(_lo(core, d.jvp.dx, lo), r.slope)
    if r.act == "lrelu":
        b = b.add(d.tan.abs(), alpha=U)
    return {"tan": _lo(b, d.tan, lo)}


def dual_bounds(r, d, lo, amb=None, streams=1):
    """train.bn_dual_backward: dx = [backward of dy, stored] + the dual term, stored again; dxdot = the backward of dyt;
    dgamma = dgamma(dy) + A*rstd, both f32, added in f32.  streams: bn_dual_backward_summed adds that many equal dual terms."""
    n = r.n
    b = {}
    db0, dg0, dx0 = _backward_bounds(r, r, r.g, amb, r.dy)
    _, _, dxd = _backward_bounds(r, d.bdot, d.q, amb, d.dyt)
    b["dxdot"] = _lo(dxd, d.dxdot, lo)
    b["dbeta"] = db0
    # the five sums: Sx is exact (f32 terms in f64), the others carry the f32 roundings of q and xhat
    e_sq, e_sqx, _, _, qa = _sum_bounds(r, d.q, amb, d.dyt)
    _, e_sxx, _, _, xda = _sum_bounds(r, d.xdot, None, None, lrelu=False)
    e_sqd = (U if r.act == "lrelu" else 0.0) * (qa * xda).sum(0)
    if amb is not None:
        e_sqd = e_sqd + _dslope(r.act) * _amb_sum(amb, d.dyt, d.xdot)
    e_a = e_sqd + e_sq * d.Sx.abs() / n + (e_sqx * d.Sxx.abs() + d.Sqx.abs() * e_sxx) / n
    a_abs = d.Sqd.abs() + (d.Sq * d.Sx).abs() / n + (d.Sqx * d.Sxx).abs() / n            # A without its cancellations
    k0 = d.k0.abs()
    c0_abs = k0 / n * (a_abs + 2.0 * (d.Sxx * d.Sqx).abs() / n)
    c3_abs = k0 / n * ((d.Sxx * d.Sq).abs() / n + (d.Sqx * d.Sx).abs() / n)
    e_c0 = k0 / n * (e_a + 2.0 * (e_sxx * d.Sqx.abs() + d.Sxx.abs() * e_sqx) / n)
    e_c1, e_c2 = k0 * e_sxx / n, k0 * e_sqx / n
    e_c3 = k0 / n * ((e_sxx * d.Sq.abs() + d.Sxx.abs() * e_sq) / n + (e_sqx * d.Sx.abs()) / n)
    # per element: K_DUAL u (|c0|~ |xhat| + |c1 q| + |c2 xdot| + |c3|~) + |c0|~ K_XHAT u (|x| + |mean|) rstd + the coefficients' errors
    xh_err = c0_abs * (K_XHAT * U) * r.rstd
    dual = _axh(r) * (K_DUAL * U * c0_abs + e_c0)
    dual.addcmul_(qa, K_DUAL * U * d.c1.abs() + e_c1).addcmul_(xda, K_DUAL * U * d.c2.abs() + e_c2)
    dual.addcmul_(_ax(r), xh_err).add_(K_DUAL * U * c3_abs + e_c3 + xh_err * r.mean.abs())
    # every accumulating launch stores dx again: one rounding at the magnitude of ITS partial sum dx(dy) + k dual (the sum can
    # cancel, so the last magnitude alone does not cover the earlier stores)
    total = _lo(dx0, r.dx, lo).add_(dual, alpha=streams)
    for k in range(1, streams + 1):
        total.add_((r.dx + k * d.dual).abs_(), alpha=BF if lo else U)
    b["dx"] = total
    # dgamma: dgamma(dy) in f32 + (float)(A*rstd) with rstd's 3 roundings and its own, then one f32 addition per stream
    dg_tan = r.rstd * e_a + (K_RSTD * U) * r.rstd * a_abs
    b["dgamma"] = dg0 + streams * dg_tan + streams * U * (r.dgamma.abs() + streams * d.dg_tan.abs())
    return b


def bn_references(r, d=None):
    """name -> reference tensor of every output the GPU test compares (those that were computed)."""
    o = dict(mean=r.mean, rstd=r.rstd, y=r.y)
    if hasattr(r, "rm"):
        o.update(rm=r.rm, rv=r.rv)
    if hasattr(r, "dy"):
        o.update(dbeta=r.dbeta, dgamma=r.dgamma, dx=r.dx)
        if r.add is not None:
            o["dx_add"] = r.dx_add
    if d is not None:
        o["tan"] = d.tan
        if hasattr(d, "dyt"):
            o.update(dual_dx=d.dx, dual_dxdot=d.dxdot, dual_dgamma=d.dgamma, dual_dbeta=d.dbeta)
    return o


def bn_bounds(r, d, lo, amb=None):
    """name -> bound, same names as bn_references."""
    b = forward_bounds(r, lo)
    if hasattr(r, "dy"):
        b.update(backward_bounds(r, lo, amb))
    if d is not None:
        b.update(tangent_bounds(r, d, lo))
        if hasattr(d, "dyt"):
            b.update({"dual_" + k: v for k, v in dual_bounds(r, d, lo, amb).items()})
    return b


PER_ELEMENT = ("dx", "dx_add", "tan", "dual_dx", "dual_dxdot")      # ambiguous elements are left out of these


def bn_ratios(got, refs, bounds, amb=None):
    """name -> worst err / bound for every output in `got`."""
    return {k: worst_ratio(v, refs[k], bounds[k], amb if k in PER_ELEMENT else None) for k, v in got.items()}


def worst_ratio(got, ref, bound, skip=None):
    """max err / bound over the tensor (0 / 0 counts as 0, err > 0 over a zero bound as inf, anything not finite in `got`
    as inf); `skip` elements are left out."""
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got.double() - ref).abs_()
    zero = err == 0
    err.div_(bound).masked_fill_(zero, 0.0)
    if skip is not None:
        err.masked_fill_(skip, 0.0)
    return float(err.max())


# ---- BatchNorm: cases ---------------------------------------------------------------------------------------------------------
# name -> C, P, activations, dtypes, seed, why.  Seeds are chosen so that no element outside the two block-cap cases is
# mask-ambiguous (tests/test_train_edges_cpu.py asserts it).
BN_SHAPES = {
    "c8": dict(C=8, P=70, acts=ACTS, dtypes=("f32", "bf16"), seed=11,
               why="one chunk column; fewer pixels than the 256 rows of one iteration"),
    "c256": dict(C=256, P=45, acts=("lrelu",), dtypes=("f32", "bf16"), seed=12, why="a width no other test runs"),
    "c1024": dict(C=1024, P=30, acts=("relu",), dtypes=("f32", "bf16"), seed=13, why="a width no other test runs, rpi = 2"),
    "p1": dict(C=64, P=1, acts=("relu", "none"), dtypes=("f32", "bf16"), seed=14,
               why="a single pixel: variance 0, xhat 0, the unbiased factor's guard"),
    "p2": dict(C=16, P=2, acts=("lrelu",), dtypes=("f32", "bf16"), seed=15, why="two pixels"),
    "ragged": dict(C=32, P=513, acts=ACTS, dtypes=("f32", "bf16"), seed=16,
                   why="one pixel more than rpi * 8: a second work-group, a short slab, a partial last iteration"),
    "cap16": dict(C=16, P=1048576 + 389, acts=("relu",), dtypes=("f32", "bf16"), seed=11,
                  why="the block cap at layer0's width: 1024 work-groups, slab rounding, the finalize over 1024 partials"),
    "cap2048": dict(C=2048, P=8192 + 37, acts=("lrelu",), dtypes=("f32",), seed=17, why="the block cap with rpi = 1"),
}
CAP_CASES = ("cap16", "cap2048")
STREAM_CASES = ("c8", "ragged", "cap16")             # bn_dual_backward_summed and the multi-stream forms run on these only
AMBIGUOUS_SHARE_MAX = 1e-5

# The value case: C = 16, P = 1152, one purpose per channel.  `ratio` is mean / sigma of x = sigma * (randn + ratio).
VALUE_C, VALUE_P = 16, 1152
VALUE_CHANNELS = {
    0: dict(kind="offset", ratio=0.0, why="mean/sigma 0"),
    1: dict(kind="offset", ratio=100.0, why="mean/sigma +100: x*sc + sh and cb*x + cc cancel 2 digits"),
    2: dict(kind="offset", ratio=-100.0, why="mean/sigma -100"),
    3: dict(kind="offset", ratio=1000.0, why="mean/sigma +1000: 3 digits"),
    4: dict(kind="offset", ratio=-1000.0, why="mean/sigma -1000"),
    5: dict(kind="const", value=3.25, why="constant channel: variance exactly 0, rstd = 1/sqrt(eps)"),
    6: dict(kind="const", value=0.0, why="all-zero channel: y == act(beta) bitwise"),
    7: dict(kind="tiny", sigma=1e-4, why="variance 1e-8, far below eps"),
    8: dict(kind="plain", gamma=-0.8, why="negative gamma"),
    9: dict(kind="plain", gamma=0.0, beta=0.0, why="z == 0 exactly at every element: the kink itself"),
    10: dict(kind="plain", gamma=0.0, beta=-1.0, why="fully masked channel, every coefficient 0: dx == dx_add bitwise"),
}
BN_VALUES = {
    "values": dict(acts=ACTS, dtypes=("f32", "bf16"), seed=26, eps=1e-5, momentum=0.1, why="one purpose per channel"),
    "values_eps": dict(acts=("lrelu",), dtypes=("f32", "bf16"), seed=26, eps=1e-3, momentum=0.3,
                       why="eps and momentum other than the defaults"),
}


def bn_runs():
    """[(case, act, dtype name)] of every BatchNorm run of the GPU test."""
    out = []
    for table in (BN_SHAPES, BN_VALUES):
        for name, c in table.items():
            out += [(name, a, d) for a in c["acts"] for d in c["dtypes"]]
    return out


def case_eps_momentum(name):
    c = BN_VALUES.get(name)
    return (c["eps"], c["momentum"]) if c else (1e-5, 0.1)


@functools.lru_cache(maxsize=4)
def bn_operands(name, dtype):
    """dict of CPU tensors: x, dy, add, xdot, dyt [P, C] in the kernel's dtype; gamma, beta, rm, rv f32 [C]."""
    t = DTYPES[dtype]
    if name in BN_SHAPES:
        c = BN_SHAPES[name]
        C, P = c["C"], c["P"]
        g = torch.Generator().manual_seed(c["seed"])
        x = torch.randn(P, C, generator=g) * 1.7 + 0.6
        gamma = torch.rand(C, generator=g) + 0.5
        beta = torch.randn(C, generator=g) * 0.3
    else:
        c = BN_VALUES[name]
        C, P = VALUE_C, VALUE_P
        g = torch.Generator().manual_seed(c["seed"])
        x = torch.randn(P, C, generator=g) * 1.7 + 0.6
        z = torch.randn(P, C, generator=g)
        gamma = torch.rand(C, generator=g) + 0.5
        beta = torch.randn(C, generator=g).sign() * (torch.rand(C, generator=g) * 0.4 + 0.1)
        for ch, v in VALUE_CHANNELS.items():
            if v["kind"] == "offset":
                x[:, ch] = z[:, ch] + v["ratio"]
            elif v["kind"] == "const":
                x[:, ch] = v["value"]
            elif v["kind"] == "tiny":
                x[:, ch] = z[:, ch] * v["sigma"]
            if "gamma" in v:
                gamma[ch] = v["gamma"]
            if "beta" in v:
                beta[ch] = v["beta"]
    o = dict(x=x.to(t), gamma=gamma, beta=beta)
    o["rm"], o["rv"] = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    for k in ("dy", "add", "xdot", "dyt"):
        o[k] = torch.randn(P, C, generator=g).to(t)
    return o


def kink_operands(act, seed=31, C=16, P=4096):
    """An f32 case with thousands of elements whose |z| is within a few ulps of 0: half of every channel's pixels sit on a grid
    of single-ulp steps around x0, and beta is set AFTER the statistics are known so that z(x0) = 0:  beta = -(x0 - mean)*sc.
    (The kernels' z = x*sc + (beta - mean*sc) carries roundings of about u*|x0*sc| ~ ulp(x0)*sc: the grid step.)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(P, C, generator=g) * 1.7 + 0.6
    x0 = 0.5625 + torch.arange(C, dtype=torch.float32) / 64
    k = (torch.arange(P // 2) % 33 - 16).float()       # every grid point many times: P / 2 elements within 16 steps of x0
    x[::2] = x0 + k[:, None] * (2.0 ** -24)            # ulp(x0) = 2^-24 in [0.5, 1): every grid point is an f32 value
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[::4] *= -1
    x64 = x.double()
    mean = x64.mean(0)
    rstd = 1.0 / torch.sqrt(x64.var(0, unbiased=False) + float(np.float32(1e-5)))
    beta = (-(x0.double() - mean) * gamma.double() * rstd).float()
    o = dict(x=x, gamma=gamma, beta=beta)
    for name in ("dy", "add", "xdot", "dyt"):
        o[name] = torch.randn(P, C, generator=g)
    return o


# ---- pointwise tails, in f32 arithmetic ------------------------------------------------------------------------------------------

def add_relu_ref(z, r):
    """relu(z + r): the sum in f32, v > 0 ? v : +0, one rounding to the tensor's type."""
    v = z.float() + r.float()
    return torch.where(v > 0, v, torch.zeros_like(v)).to(z.dtype)


def relu_mask_ref(out, dout, add=None):
    """dout where out > 0, else +0; + add in f32; one rounding."""
    g = torch.where(out.float() > 0, dout.float(), torch.zeros_like(dout, dtype=torch.float32))
    if add is not None:
        g = g + add.float()
    return g.to(out.dtype)


def pointwise_values(dtype):
    """(z, r) of 8 * k elements holding the value cases: exact cancellations z = -r, +-0 on both sides, sums that tie between
    two bf16 values (1 + 2^-8 and its neighbours, both signs), tiny and huge magnitudes."""
    t = DTYPES[dtype]
    z = [1.5, -1.5, 0.0, -0.0, 0.0, -0.0, 1.0, 1.0, 1.0078125, -1.0, 3.0, 2.0 ** -126, -2.0 ** -126, 1e30, -1e30, 0.25,
         1.0, 1.0078125, 2.0 ** -133, 65280.0, 0.5, -0.5, 7.0, -7.0]
    r = [-1.5, 1.5, 0.0, 0.0, -0.0, -0.0, 2.0 ** -8, 3 * 2.0 ** -8, 2.0 ** -8, -2.0 ** -8, -3.0, -2.0 ** -126, 2.0 ** -126, 1e30,
         1e30, -0.25, -2.0 ** -8, -2.0 ** -8, 2.0 ** -133, 128.0, -0.5, 0.5, -7.5, 7.5]
    assert len(z) == len(r) and len(z) % 8 == 0
    return torch.tensor(z).to(t), torch.tensor(r).to(t)


# ---- Adam, sum of squares, column sums ------------------------------------------------------------------------------------------

def adam_ref(p, grads, lr, betas, eps, weight_decay, first_step=1, grad_scale=1.0, m=None, v=None):
    """torch.optim.Adam (L2 weight decay folded into the gradient) in plain f64 over a list of gradients; returns p, m, v."""
    p = p.double().clone()
    m = torch.zeros_like(p) if m is None else m.double().clone()
    v = torch.zeros_like(p) if v is None else v.double().clone()
    b1, b2 = betas
    for i, g in enumerate(grads):
        t = first_step + i
        g = g.double() * grad_scale + weight_decay * p
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr / (1 - b1 ** t) * m / (v.sqrt() / (1 - b2 ** t) ** 0.5 + eps)
    return p, m, v


K_SUMSQ = 2     # f32 -> f64 products and sums (2^-53 each, nothing next to u), one rounding to f32; the issue's allowance is 2
K_COLSUM = 2


def sumsq_bound(ref):
    return K_SUMSQ * U * ref


def colsum_bound(x64):
    """2u |ref| + 2^-45 sum |x|: one rounding to f32 (allowance 2) and the f64 summation (at most 2^-53 per addition)."""
    return K_COLSUM * U * x64.sum(0).abs() + 2.0 ** -45 * x64.abs().sum(0)


# ---- GradNorm on 5 scalars --------------------------------------------------------------------------------------------------

def gradnorm_step_ref(w, losses, gn, base, alpha, m, v, lr, betas, eps, step):
    """ppn_gradnorm_weight_step in f64 (main.py:668-768): G_i = |w_i| gn_i, C_i = mean(G) (lhat_i / mean(lhat))^alpha with
    lhat_i = w_i L_i / base_i, Lgrad = sum |G_i - C_i| with C detached, dLgrad/dw_i = sign(G_i - C_i) sign(w_i) gn_i (sign(0) =
    0 for both), then Adam on w.  Returns (w, m, v, G, C, dw, Lgrad)."""
    w, losses, gn, base, m, v = (np.asarray(t, np.float64).copy() for t in (w, losses, gn, base, m, v))
    G = np.abs(w) * gn
    lhat = w * losses / base
    Cc = G.mean() * (lhat / lhat.mean()) ** alpha
    d = G - Cc
    dw = np.sign(d) * np.sign(w) * gn
    b1, b2 = betas
    m = b1 * m + (1 - b1) * dw
    v = b2 * v + (1 - b2) * dw * dw
    w = w - lr / (1 - b1 ** step) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps)
    return w, m, v, G, Cc, dw, np.abs(d).sum()


def gradnorm_renorm_ref(w, world):
    """main.py:769-777 after the SUM all-reduce: w / world, clamp at 0, divide by the mean."""
    t = np.maximum(np.asarray(w, np.float64) / world, 0.0)
    return t / t.mean()
