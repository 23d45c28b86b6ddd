"""Edge cases for the backward convolutions (csrc/wgrad.hip, csrc/stem_wgrad.hip, train.conv_dgrad with ppn_pack_weight_dgrad,
ppn_upsample_zero and the parity interleavers) and their f64 reference.  Plain helper module (no tests):
tests/test_backward_edges_cpu.py checks that the cases are what they claim and that the reference is right,
tests/test_backward_edges_gpu.py runs the kernels on them.

Every case is off-square.  A convolution case is Conv(B, ci, co, H, W, k, s, dil, pad): x is NHWC [B, H, W, ci], dy is NHWC
[B, Ho, Wo, co], the weight [co, ci, k, k].

Reference: F.conv2d in f64 on the already-rounded operands, then .backward (grads_ref); conv_grads_by_taps restates the same
two sums as an explicit loop over the filter taps for the CPU test.  References are computed once per (case, dtype) and shared:
callers must not modify what they get.

What the library is asked, never restated here: the number of pixel splits of the generic weight-gradient kernels and the grid
of the stem kernels, both through ppn_conv_wgrad_workspace_bytes (a host function: it runs without a GPU).  What IS restated
are the documented tile sizes (wgrad.hip: 128 x 128 tile, 256 x 256 once cin and cout are both >= 256; 64 pixels per depth
step for the 4-wave bf16 kernel and 32 for the other three; stem_wgrad.hip: tiles of 8 x 64 output pixels, 4 x 64 for the
stride-2 layer, at most 512 workgroups for the 7x7 kernel on 8 channels and 1024 for the other three).
"""
from __future__ import annotations

import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

Conv = collections.namedtuple("Conv", "B ci co H W k s dil pad")

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def eff(c):
    return c.dil * (c.k - 1) + 1


def out_hw(c):
    return (c.H + 2 * c.pad - eff(c)) // c.s + 1, (c.W + 2 * c.pad - eff(c)) // c.s + 1


def pixels(c):
    Ho, Wo = out_hw(c)
    return c.B * Ho * Wo


def wgrad_tol(c):
    """The project's bound on dW (tests/test_train_gpu.py): the operands are already rounded, the products are exact in f32 for
    bf16 operands, only the f32 accumulation order over the B * Ho * Wo pixels differs."""
    return 3e-5 * pixels(c) ** 0.5


# ---- A: generic weight gradient ------------------------------------------------------------------------------------------
# name -> (case, {dtype: what the case is for with that dtype}).  The purposes are checked against the library's split count
# by check_wgrad_purpose(); a dtype that is absent is not run (the case has no purpose there).
#   split23   nsplit in {2, 3}: the smallest multi-split
#   tail      nsplit >= 5, nsplit % 4 != 0 (the fold kernel's tail loop), depth steps not a multiple of nsplit (ragged last split)
#   any       no condition on the split
#   ldscap    more splits than the work-group budget alone gives: the LDS offset table (63 steps of 64 pixels) bounds a split
WGRAD_CASES = {
    # 1: 128-tile, smallest multi-split (f32 steps are 32 pixels, so each dtype has its own ~18-step shape)
    "split2/bf16": (Conv(1, 64, 64, 31, 37, 3, 1, 1, 1), {"bf16": "split23"}),
    "split2/f32": (Conv(1, 64, 64, 17, 33, 3, 1, 1, 1), {"f32": "split23"}),
    # 2: fold tail and a ragged last split
    "tail/bf16": (Conv(3, 64, 64, 31, 41, 3, 1, 1, 1), {"bf16": "tail", "f32": "any"}),
    "tail/f32": (Conv(3, 64, 64, 31, 21, 3, 1, 1, 1), {"f32": "tail", "bf16": "any"}),
    # 3: the 256-tile, once as a 1x1 and once dilated with ragged channel tiles
    "big1x1": (Conv(3, 256, 256, 23, 19, 1, 1, 1, 0), {"f32": "tail", "bf16": "tail"}),
    "big3x3d2": (Conv(3, 264, 320, 23, 19, 3, 1, 2, 2), {"f32": "tail", "bf16": "tail"}),
    # 4: stride 2, (H + 2 pad - k) % 2 == 1 on one axis only
    "s2/3x3": (Conv(2, 64, 128, 18, 13, 3, 2, 1, 1), {"f32": "any", "bf16": "any"}),
    "s2/1x1": (Conv(2, 64, 128, 13, 18, 1, 2, 1, 0), {"f32": "any", "bf16": "any"}),
    "s2/3x3/ci32": (Conv(3, 32, 64, 26, 21, 3, 2, 1, 1), {"f32": "any", "bf16": "any"}),
    # 5: the divisor-1 paths of the index decomposition
    "wo1": (Conv(2, 64, 64, 37, 1, 3, 1, 1, 1), {"f32": "any", "bf16": "any"}),
    "ho1": (Conv(2, 64, 64, 1, 37, 3, 1, 1, 1), {"f32": "any", "bf16": "any"}),
    # optional: 49 taps of an 8 -> 8 layer leave 10 splits of 67 steps; the offset table allows 63, so there are 11
    "ldscap": (Conv(2, 8, 8, 141, 151, 7, 1, 1, 3), {"bf16": "ldscap"}),
}
# 6: work items (taps x tiles x splits) that are not a multiple of 8 -- idle work-groups behind the XCD remap
WGRAD_IDLE = ("split2/bf16", "split2/f32", "tail/bf16", "tail/f32", "big1x1")


def wgrad_runs():
    """[(name, dtype name)] of every (case, dtype) the GPU test runs."""
    return [(n, d) for n, (_, why) in WGRAD_CASES.items() for d in ("f32", "bf16") if d in why]


def wgrad_tile(c):
    return 256 if c.ci >= 256 and c.co >= 256 else 128


def wgrad_steps(c, dtype):
    """Depth steps of the whole reduction: 64 pixels in the 4-wave bf16 kernel, 32 in the f32 kernels and the 8-wave bf16 one."""
    bkp = 64 if dtype == "bf16" and wgrad_tile(c) == 128 else 32
    return -(-pixels(c) // bkp)


def wgrad_items(c, nsplit):
    t = wgrad_tile(c)
    return c.k * c.k * -(-c.co // t) * -(-c.ci // t) * nsplit


def _desc(c, dtype):
    from pytorch_pose_proposal_network_amd import lib as L
    d = L.WgradDesc()
    d.dtype = L.PPN_F32 if dtype == "f32" else L.PPN_BF16
    d.batch, d.in_h, d.in_w, d.cin = c.B, c.H, c.W, c.ci
    d.out_h, d.out_w = out_hw(c)
    d.cout, d.ksize, d.stride, d.dilation, d.pad = c.co, c.k, c.s, c.dil, c.pad
    return d


def partials(c, dtype):
    """Partial results the library folds for this launch: the pixel splits of the generic kernels, the grid (work-groups) of
    the stem kernels.  From the library's workspace size; host code only."""
    import ctypes as C
    from pytorch_pose_proposal_network_amd import lib as L
    need = L.load().ppn_conv_wgrad_workspace_bytes(C.byref(_desc(c, dtype)))
    per = c.k * c.k * c.co * c.ci * 4
    assert need > 0 and need % per == 0, (c, dtype, need)
    return need // per


def check_wgrad_purpose(name, dtype, nsplit):
    """Why the (case, dtype) does not serve its purpose with `nsplit` splits, or None."""
    c, why = WGRAD_CASES[name]
    steps = wgrad_steps(c, dtype)
    kind = why[dtype]
    if kind == "split23" and nsplit not in (2, 3):
        return f"{name} {dtype}: {nsplit} splits, wanted 2 or 3"
    if kind == "tail" and not (nsplit >= 5 and nsplit % 4 and steps % nsplit):
        return f"{name} {dtype}: {nsplit} splits of {steps} steps, wanted >= 5, not a multiple of 4, and a ragged last one"
    if kind == "ldscap":
        budget = 512 // wgrad_items(c, 1)        # splits that fill 512 work-groups: more than that only when the table binds
        if not (dtype == "bf16" and wgrad_tile(c) == 128 and nsplit > budget and
                -(-steps // nsplit) <= 63 < -(-steps // budget)):
            return f"{name} {dtype}: {nsplit} splits of {steps} steps, budget {budget}: the LDS table does not bind"
    if name in WGRAD_IDLE and kind != "any" and wgrad_items(c, nsplit) % 8 == 0:
        return f"{name} {dtype}: {wgrad_items(c, nsplit)} work items, a multiple of 8"
    return None


# ---- B: stem weight gradient (bf16 only) --------------------------------------------------------------------------------------
# persistent: cap < tiles < 2 cap (some work-groups take two tiles, some one); small: tiles < cap, taller than wide
STEM_CASES = {
    "l0c8/persistent": Conv(3, 8, 16, 100, 850, 7, 1, 1, 3),
    "l0c4/persistent": Conv(3, 4, 16, 150, 1190, 7, 1, 1, 3),
    "l1/persistent": Conv(3, 16, 16, 150, 1190, 3, 1, 1, 1),
    "l2/persistent": Conv(3, 16, 32, 150, 2300, 3, 2, 1, 1),
    "l0c8/small": Conv(2, 8, 16, 75, 45, 7, 1, 1, 3),
    "l0c4/small": Conv(2, 4, 16, 75, 45, 7, 1, 1, 3),
    "l1/small": Conv(2, 16, 16, 75, 45, 3, 1, 1, 1),
    "l2/small": Conv(2, 16, 32, 149, 90, 3, 2, 1, 1),
}


def stem_rows(c):
    return 4 if c.s == 2 else 8


def stem_cap(c):
    return 512 if (c.k == 7 and c.ci == 8) else 1024


def stem_tiles(c):
    Ho, Wo = out_hw(c)
    return c.B * -(-Ho // stem_rows(c)) * -(-Wo // 64)


# ---- C: input gradient ----------------------------------------------------------------------------------------------------
# name -> (case, the path of train.conv_dgrad it is for, per (dtype, with add))
DGRAD_CASES = {
    "ragged/d4": Conv(1, 160, 72, 7, 9, 3, 1, 4, 4),           # channel counts that are no tile multiple, dilation > image / 2
    "big/d2/256to512": Conv(1, 256, 512, 10, 7, 3, 1, 2, 2),   # the >= 256-wide tile with dilation
    "big/d2/512to256": Conv(1, 512, 256, 10, 7, 3, 1, 2, 2),
    "w1": Conv(2, 64, 64, 9, 1, 3, 1, 1, 1),                   # a one-column image
    # stride 2, (H + 2 pad - k) % 2 == 1 on exactly one axis
    "s2/3x3/ci16": Conv(2, 16, 32, 12, 9, 3, 2, 1, 1),         # cin <= 16: stacked parity (f32, or no add), zero-upsampled (bf16 + add)
    "s2/3x3/ci16/t": Conv(2, 16, 32, 9, 12, 3, 2, 1, 1),
    "s2/3x3/ci64": Conv(1, 64, 128, 9, 12, 3, 2, 1, 1),        # cin > 16: zero-upsampled
    "s2/1x1/ci64": Conv(2, 64, 128, 9, 12, 1, 2, 1, 0),        # half-resolution 1x1 + ppn_upsample_zero (f32, or no add)
    "s2/1x1/ci8": Conv(2, 8, 16, 12, 9, 1, 2, 1, 0),
    "s2/3x3/pad0": Conv(2, 32, 64, 12, 9, 3, 2, 1, 0),         # pad 0: the last row receives no gradient at all
}
DGRAD_S2 = tuple(n for n, c in DGRAD_CASES.items() if c.s == 2)


def touched(c):
    """bool [H, W]: the input pixels that at least one output pixel reads through at least one tap."""
    def axis(n, no):
        t = np.zeros(n, bool)
        for o in range(no):
            for u in range(c.k):
                i = o * c.s - c.pad + u * c.dil
                if 0 <= i < n:
                    t[i] = True
        return t
    Ho, Wo = out_hw(c)
    return np.outer(axis(c.H, Ho), axis(c.W, Wo))


def dgrad_tols(dtype):
    """(max-norm factor, per-element relative term, per-element absolute factor); the absolute terms scale with
    max(1, max |ref|).  bf16: 2^-8 |ref| is twice the half-ulp of the one final rounding, 3e-5 the f32 accumulation allowance."""
    return (2e-2, 2.0 ** -8, 3e-5) if dtype == "bf16" else (3e-5, 0.0, 3e-5)


# ---- operands and references ----------------------------------------------------------------------------------------------

def _seed(name):
    return 1000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100000


@functools.lru_cache(maxsize=None)
def wgrad_operands(table, name, dtype):
    """(x NHWC, dy NHWC) in the kernel's dtype, CPU."""
    c = WGRAD_CASES[name][0] if table == "wgrad" else STEM_CASES[name]
    g = torch.Generator().manual_seed(_seed(name))
    Ho, Wo = out_hw(c)
    x = torch.randn(c.B, c.H, c.W, c.ci, generator=g).to(DTYPES[dtype])
    dy = torch.randn(c.B, Ho, Wo, c.co, generator=g).to(DTYPES[dtype])
    return x, dy


@functools.lru_cache(maxsize=None)
def wgrad_ref(table, name, dtype):
    """dW f64 [co, ci, k, k] by autograd."""
    c = WGRAD_CASES[name][0] if table == "wgrad" else STEM_CASES[name]
    x, dy = wgrad_operands(table, name, dtype)
    return grads_ref(c, x=x, dy=dy)[0]


@functools.lru_cache(maxsize=None)
def dgrad_operands(name, dtype):
    """(dy NHWC, w f32 [co, ci, k, k] holding values of the kernel's dtype, add NHWC), CPU."""
    c = DGRAD_CASES[name]
    g = torch.Generator().manual_seed(_seed(name))
    Ho, Wo = out_hw(c)
    w = torch.randn(c.co, c.ci, c.k, c.k, generator=g) * (c.ci * c.k * c.k) ** -0.5
    w = w.to(DTYPES[dtype]).float()
    dy = torch.randn(c.B, Ho, Wo, c.co, generator=g).to(DTYPES[dtype])
    add = torch.randn(c.B, c.H, c.W, c.ci, generator=g).to(DTYPES[dtype])
    return dy, w, add


@functools.lru_cache(maxsize=None)
def dgrad_ref(name, dtype):
    """dX f64 NHWC by autograd, without `add`."""
    c = DGRAD_CASES[name]
    dy, w, _ = dgrad_operands(name, dtype)
    return grads_ref(c, w=w, dy=dy)[1]


def grads_ref(c, dy, x=None, w=None):
    """(dW [co, ci, k, k] or None, dX NHWC or None) in f64: F.conv2d on the operands as given, then .backward."""
    xr = (torch.zeros(c.B, c.ci, c.H, c.W, dtype=torch.float64) if x is None else x.double().permute(0, 3, 1, 2).contiguous())
    wr = torch.zeros(c.co, c.ci, c.k, c.k, dtype=torch.float64) if w is None else w.double()
    xr.requires_grad_(w is not None)
    wr.requires_grad_(x is not None)
    F.conv2d(xr, wr, None, c.s, c.pad, c.dil).backward(dy.double().permute(0, 3, 1, 2))
    return (wr.grad if x is not None else None,
            xr.grad.permute(0, 2, 3, 1).contiguous() if w is not None else None)


def conv_grads_by_taps(c, x, w, dy):
    """The same two sums written out per filter tap (NumPy, f64, NHWC x / dy, [co, ci, k, k] w) -> (dW, dX):
        y[b, oy, ox, o] = sum_{u, v, i} w[o, i, u, v] x[b, oy s - pad + u dil, ox s - pad + v dil, i]
        dW[o, i, u, v]  = sum_{b, oy, ox} dy[b, oy, ox, o] x[b, oy s - pad + u dil, ox s - pad + v dil, i]
        dX[b, iy, ix, i] = sum over the (oy, u), (ox, v) that land on (iy, ix) of dy[b, oy, ox, o] w[o, i, u, v]"""
    x, w, dy = (np.asarray(t, np.float64) for t in (x, w, dy))
    Ho, Wo = out_hw(c)
    dW = np.zeros_like(w)
    dX = np.zeros_like(x)
    for u in range(c.k):
        for v in range(c.k):
            for oy in range(Ho):
                iy = oy * c.s - c.pad + u * c.dil
                if not 0 <= iy < c.H:
                    continue
                for ox in range(Wo):
                    ix = ox * c.s - c.pad + v * c.dil
                    if not 0 <= ix < c.W:
                        continue
                    dW[:, :, u, v] += np.einsum("bo,bi->oi", dy[:, oy, ox], x[:, iy, ix])
                    dX[:, iy, ix] += dy[:, oy, ox] @ w[:, :, u, v]
    return dW, dX


# ---- D: one off-square training iteration --------------------------------------------------------------------------------------
TRAIN_ARCH, TRAIN_BATCH = "drn_d_22", 2
TRAIN_H, TRAIN_W = 112, 80                                       # image rows x columns -> a grid of 7 rows x 5 columns
TRAIN_INSIZE = (TRAIN_W, TRAIN_H)                                # W first, as oracle/targets_ref.py and PPNLoss write it
TRAIN_OUTSIZE = (TRAIN_W // 16, TRAIN_H // 16)


@functools.lru_cache(maxsize=None)
def train_inputs():
    """(state dict, x f32 [B, 3, H, W], targets) of the off-square iteration."""
    from oracle import forward_ref as Fr, targets_ref as T
    from pytorch_pose_proposal_network_amd import prng, synth
    sd = synth.make_state_dict(TRAIN_ARCH, 13)
    x = Fr.normalize_u8(prng.u8_frames(23, TRAIN_BATCH, (TRAIN_H, TRAIN_W)))
    per = [T.encode_targets(synth.synthetic_people(33 + i, insize=TRAIN_INSIZE), insize=TRAIN_INSIZE, outsize=TRAIN_OUTSIZE)
           for i in range(TRAIN_BATCH)]
    tg = {k: np.ascontiguousarray(np.stack([p[k] for p in per])) for k in per[0]}
    return sd, x, tg


@functools.lru_cache(maxsize=None)
def train_ref(dtype_name):
    from oracle import train_ref as R
    sd, x, tg = train_inputs()
    return R.train_iteration_ref(sd, x, tg, [1.0] * 5, [1.0] * 5, TRAIN_ARCH, TRAIN_INSIZE,
                                 dtype=torch.float64 if dtype_name == "f64" else torch.float32)
