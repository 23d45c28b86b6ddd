"""Edge cases for the split-K convolution (csrc/conv_splitk.hip: conv_splitk_partial_kernel + conv_splitk_reduce_kernel behind
ppn_conv_desc.flags & PPN_CONV_SPLIT_K), an emulation of its slab partition, and operands on which every sum is exact.  Plain
helper module (no tests): tests/test_splitk_edges_cpu.py checks that the cases are what they claim, that the partition
emulation partitions, and which planted faults each detector sees; tests/test_splitk_edges_gpu.py runs the kernels.

Cases, operands, the f64 reference and the per-element bound are tests/forward_cases.py's (Conv, Epi, EPILOGUES, make_operands,
reference_of, ratio, worst).  THE BOUND IS UNCHANGED: summing the slabs 0 .. S-1 is one more summation order of the same K
products, which (K + 4) u already covers, and the reduce kernel computes both outputs from the f32 value v with one rounding per
store (conv_splitk.hip:203-229); PPN_CONV_OUT_BF16 on an f16 launch rounds to bf16, u_out = 2^-8 (reference_of(..., "bf16") on
the f16 operands).

Partition (csrc/splitk_partition.h and the header of conv_splitk.hip): the GEMM depth K = k k ci is walked in K steps of bk
elements (32 in f32, 64 in the 16-bit types), one step being bk consecutive input channels of one filter tap, in the order of the
packed weight rows:
    co >= 64   channel-chunk-major: step s is tap s % ntaps, channels (s / ntaps) bk ..
    co <  64   tap-major:           step s is tap s / (ci / bk), channels (s % (ci / bk)) bk ..
A slab is 512 consecutive K elements (16 / 8 steps); the last may be ragged.  workspace[slab][pixel][cout_pad] (f32) holds the
sum over the slab's terms; columns co .. cout_pad - 1 multiply zero weight rows and are 0.

Exact operands: small integers (and scales from {0.5, 1, 2}), so that every product, partial sum and epilogue value is exactly
representable in f32 whatever the order -- the expected output is the f64 result rounded ONCE to the storage type, and a kernel
must return exactly that.  This sees a single lost or doubled term at any depth, which the bound at K = 18432 cannot.
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

import forward_cases as FC
from forward_cases import Conv, Epi, EPILOGUES, make_operands, reference_of

SLAB = 512                                      # kSlabElems
TILE_P, TILE_C = 128, 64                        # kTileP, kTileC
BK = {"f32": 32, "bf16": 64, "f16": 64}
DTYPE_NAMES = FC.DTYPE_NAMES


def _all(slabs):
    return {d: slabs for d in DTYPE_NAMES}      # a slab is 512 K ELEMENTS: the same count in every dtype


# name -> (Conv, {dtype: expected slabs}, conditions on the route: forward_cases.check_purpose's names).  Every case is inside
# splitk_check's scope in all three dtypes (ci % 64 == 0, co % 8 == 0, k in {1, 3}) and keeps B Ho Wo co small.
CASES = {
    # K = 4608, the class the latency plans run (lowering.SPLITK_MIN_K).  Slab j starts at step 8 j (16 j in f32), tap 8 j % 9
    # (16 j % 9): never tap 0, so never on a channel-chunk boundary
    "nine_slabs": (Conv(1, 512, 64, 5, 7, 3, 1, 1, 1), _all(9), ("one_ptile",)),
    # co 72 -> cout_pad 128: two channel tiles, 56 dead workspace columns per row, slab stride M * 128 != M * 72
    "nine_slabs_d2_ct2": (Conv(2, 512, 72, 6, 5, 3, 1, 2, 2), _all(9), ("ct2", "one_ptile")),
    # K = 18432 (DRN-D-54's 2048-wide 3x3); 4 x 4 with dilation 2: every pixel is a border pixel
    "deep_36_slabs": (Conv(1, 2048, 64, 4, 4, 3, 1, 2, 2), _all(36), ("one_ptile",)),
    # reach 4 > the image: off-centre filter rows wholly in padding, whole K steps gather only the zero page
    "reach_gt_image": (Conv(2, 128, 64, 3, 5, 3, 1, 4, 4), _all(3), ("one_ptile",)),
    # divisor 1 on one axis / on both (div_wo, div_howo)
    "ho1": (Conv(2, 128, 128, 1, 37, 3, 1, 1, 1), _all(3), ("one_ptile",)),
    "wo1": (Conv(2, 128, 128, 37, 1, 3, 1, 1, 1), _all(3), ("one_ptile",)),
    "one_pixel": (Conv(3, 128, 64, 1, 1, 3, 1, 2, 2), _all(3), ("one_ptile",)),
    # stride 2, odd remainder on one axis; K = 576: the ragged last slab is ONE step (16-bit), two steps (f32)
    "s2_odd/3x3": (Conv(2, 64, 128, 18, 13, 3, 2, 1, 1), _all(2), ("one_ptile",)),
    "s2_odd/1x1": (Conv(2, 576, 64, 13, 18, 1, 2, 1, 0), _all(2), ("one_ptile",)),
    "valid": (Conv(1, 128, 64, 9, 12, 3, 1, 1, 0), _all(3), ("one_ptile",)),
    # pad 3 > reach 2: the outermost ring has no tap inside the image, its result is act1(b1) exactly
    "overpad": (Conv(1, 128, 64, 5, 6, 3, 1, 1, 3), _all(3), ("one_ptile",)),
    # 6 pixels per image: a 128-pixel tile spans 21 images; M = 240, partial second tile
    "many_images": (Conv(40, 64, 64, 2, 3, 3, 1, 1, 1), _all(2), ("imgs21", "tail")),
    "exact_tiles": (Conv(2, 64, 128, 8, 16, 3, 1, 1, 1), _all(2), ("notail",)),
    # co < 64: tap-major pack.  3 K steps per tap (6 in f32): slab 1 starts at step 8 (16) = tap 2, channel 128 -- mid-tap
    "tap_major_mid_tap": (Conv(1, 192, 40, 7, 9, 3, 1, 1, 1), _all(4), ("ct1p", "one_ptile")),
    # 8 live channels of a 64-wide workspace row.  ppn_conv_tiling pads co 8 to 16 (the generic kernel's 256 x 16 tile), which
    # splitk_check refuses (cout_pad % 64); the caller packs the weights to cout_pad 64 instead (cout_pad() below), no
    # dimension of the case changes
    "cout8": (Conv(1, 64, 8, 7, 9, 3, 1, 1, 1), _all(2), ("ct1p", "one_ptile")),
    # K = 64: ONE 16-bit K step -- prologue only, the loop body runs once without a prefetch (two steps in f32)
    "one_step": (Conv(1, 64, 64, 5, 5, 1, 1, 1, 0), _all(1), ("one_ptile",)),
}
CASE_EPILOGUES = ("bn_relu", "res_dual")
SWEEP_CASE = "nine_slabs_d2_ct2"                # all eight epilogues, and res_dual stored as bf16 from the f16 launch
EXACT_CASES = ("nine_slabs", "nine_slabs_d2_ct2", "deep_36_slabs", "tap_major_mid_tap", "s2_odd/1x1")
# residual + both outputs, on exact operands: forward_cases' res_dual (out_raw = acc + res shows every sum as it is), and the
# same behind scale1 / shift1 / ReLU
EXACT_EPILOGUES = {"res_dual": EPILOGUES["res_dual"], "bn_relu_res_dual": Epi(True, True, 1, True, True, 1, True, True)}
BATCH_CASES = {"nine_slabs_d2_ct2": 2, "many_images": 3}     # case -> how many of its first images are launched alone


def runs():
    """[(case, dtype, epilogue, stored as bf16)] of every bounded launch of the GPU test."""
    out = [(n, d, e, False) for n in CASES for d in DTYPE_NAMES for e in (EPILOGUES if n == SWEEP_CASE else CASE_EPILOGUES)]
    return out + [(SWEEP_CASE, "f16", "res_dual", True)]


def cout_pad(c):
    """Workspace row length and packed weight rows: ppn_conv_tiling's cout_pad wherever that is a multiple of the 64-channel
    tile (every case but cout8, tests/test_splitk_edges_cpu.py), else the next multiple."""
    return -(-c.co // TILE_C) * TILE_C


def tap_major(c):
    return c.co < 64                            # conv_splitk.hip: korder1 = cout >= 64


def kernel_name(dtype):
    return "conv_splitk_partial_kernel<%s, %d, %d, 2, 2>" % ({"f32": "float", "bf16": "__bf16", "f16": "_Float16"}[dtype],
                                                              TILE_P, TILE_C)


def purpose(name):
    """The case's route in forward_cases.check_purpose's form."""
    return ("splitk", TILE_P, TILE_C, False, CASES[name][2])


def _seed(name):
    return 7000 + sum(ord(ch) * (i + 3) for i, ch in enumerate(name)) % 100000


@functools.lru_cache(maxsize=None)
def operands(name, dtype):
    """forward_cases.make_operands of the case, fixed seed; shared, callers must not modify it."""
    return make_operands(CASES[name][0], dtype, _seed(name))


@functools.lru_cache(maxsize=None)
def _conv_f64(name, dtype):
    return FC.conv_f64(CASES[name][0], operands(name, dtype))


@functools.lru_cache(maxsize=None)
def reference(name, dtype, epi_name, out_bf16=False):
    """forward_cases.reference_of: ({"raw", "act"} f64 references, the same of the bounds).  out_bf16: u_out of a bf16 store."""
    return reference_of(CASES[name][0], operands(name, dtype), EPILOGUES[epi_name], "bf16" if out_bf16 else dtype,
                        _conv_f64(name, dtype))


# ---- the partition ------------------------------------------------------------------------------------------------------------

def k_steps(c, dtype, tap_major_order=None):
    """[(tap, first input channel)] of every K step, in the packed order."""
    bk, ntaps = BK[dtype], c.k * c.k
    assert c.ci % bk == 0
    cpt = c.ci // bk
    tm = tap_major(c) if tap_major_order is None else tap_major_order
    return [(s // cpt, (s % cpt) * bk) if tm else (s % ntaps, (s // ntaps) * bk) for s in range(ntaps * cpt)]


def slab_steps(c, dtype):
    """Per slab, its K steps as (tap, first channel)."""
    steps, per = k_steps(c, dtype), SLAB // BK[dtype]
    return [steps[i: i + per] for i in range(0, len(steps), per)]


def terms_of(c, dtype, steps):
    """bool [ntaps, ci]: the (tap, input channel) pairs a list of K steps covers."""
    mask = torch.zeros(c.k * c.k, c.ci, dtype=torch.bool)
    for tap, ci0 in steps:
        mask[tap, ci0: ci0 + BK[dtype]] = True
    return mask


def slab_terms(c, dtype):
    """For every slab, the set of (tap, input channel) pairs the partition assigns to it, as a bool mask [ntaps, ci]
    (tap = filter row * k + filter column)."""
    return [terms_of(c, dtype, steps) for steps in slab_steps(c, dtype)]


def masked_weight(c, w, mask):
    """w [co, ci, k, k] with the terms outside `mask` [ntaps, ci] set to zero."""
    return w * mask.t().reshape(1, c.ci, c.k, c.k).to(w.dtype)


def partials(c, x, w, masks):
    """[S, B, co, Ho, Wo]: the convolution restricted to each mask's terms, in the precision of x and w."""
    return torch.stack([F.conv2d(x, masked_weight(c, w, m), None, c.s, c.pad, c.dil) for m in masks])


def partials_f64(c, op, dtype):
    """(P, Pmag) [S, B, co, Ho, Wo] f64: each slab's piece of the sum, and the same of the magnitudes."""
    masks, x, w = slab_terms(c, dtype), op["x"].double(), op["w"].double()
    return partials(c, x, w, masks), partials(c, x.abs(), w.abs(), masks)


def partials_f32(c, op, dtype):
    return partials(c, op["x"], op["w"], slab_terms(c, dtype))


def reduce_f32(P, op, epi, dtype, out_bf16=False):
    """The reduce kernel: slabs summed 0 .. S-1 in f32, f32 epilogue, ONE rounding per output."""
    v = P[0].float()
    for s in range(1, len(P)):
        v = v + P[s].float()
    v, u = FC.epilogue(v, op, epi)
    store = "bf16" if out_bf16 else dtype
    out = {}
    if epi.raw:
        out["raw"] = FC.q(v, store)
    if epi.act:
        out["act"] = FC.q(u, store)
    return out


def emulate_f32(c, op, epi, dtype, out_bf16=False):
    """What a correct split-K pair may return: an f32 partial per slab, summed 0 .. S-1 in f32, f32 epilogue, one rounding."""
    return reduce_f32(partials_f32(c, op, dtype), op, epi, dtype, out_bf16)


def worst_ratio(got, ref, bound):
    return max(FC.ratio(got[k], ref[k], bound[k]) for k in ref)


# ---- exact operands -----------------------------------------------------------------------------------------------------------

X_MAX, W_MAX, V_MAX = 4, 2, 8                   # |x|, |w|; |res|, |b1|, |b2|
SCALES = (0.5, 1.0, 2.0)


def exact_operands(c, seed):
    """x, w, res, b1, b2 small integers, s1, s2 from {0.5, 1, 2}: representable in f32, bf16 and f16 alike, so one draw
    serves every dtype.  Use with ReLU or no activation only (LReLU's 0.1 is not exact): check_exact()."""
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = FC.out_hw(c)
    ri = lambda lim, *shape: torch.randint(-lim, lim + 1, shape, generator=g).float()                   # noqa: E731
    sc = lambda: torch.tensor(SCALES)[torch.randint(0, 3, (c.co,), generator=g)]                         # noqa: E731
    return {"x": ri(X_MAX, c.B, c.ci, c.H, c.W), "w": ri(W_MAX, c.co, c.ci, c.k, c.k), "s1": sc(), "b1": ri(V_MAX, c.co),
            "s2": sc(), "b2": ri(V_MAX, c.co), "res": ri(V_MAX, c.B, c.co, Ho, Wo)}


def check_exact(c, op, epi):
    """Asserts that every product, partial sum and epilogue value of the case on these operands is exact in f32 in ANY order of
    summation, that every operand is exact in bf16 and f16, and that no output overflows f16."""
    assert epi.act1 in (0, 1) and epi.act2 in (0, 1), "LReLU's 0.1 is not exactly representable"
    for k in ("x", "w", "res", "b1", "b2"):
        assert torch.equal(op[k], op[k].round()) and float(op[k].abs().max()) <= 256        # integers of <= 8 bits
    mx, mw = float(op["x"].abs().max()), float(op["w"].abs().max())
    s1, s2 = (float(op[k].abs().max()) if on else 1.0 for k, on in (("s1", epi.s1), ("s2", epi.s2b2)))
    assert {float(t) for k in ("s1", "s2") for t in op[k]} <= set(SCALES)
    # any partial sum of the K integer products is an integer below K max|x| max|w|; scaled by a power of two and shifted by
    # integers it stays a multiple of 1/4 far below 2^24 / 4 -- the factor 2 is headroom
    worst = ((FC.depth(c) * mx * mw * s1 + V_MAX) + V_MAX) * s2 + V_MAX
    assert worst * 2 < 2 ** 22, worst
    acc = F.conv2d(op["x"].double(), op["w"].double(), None, c.s, c.pad, c.dil)
    v, u = FC.epilogue(acc, op, epi)
    assert float(v.abs().max()) < 65504 and (u is None or float(u.abs().max()) < 65504)
    return v, u


def exact_expected(c, op, epi, dtype, out_bf16=False):
    """{"raw", "act"}: the f64 result rounded once to the storage type (as f32 tensors)."""
    v, u = check_exact(c, op, epi)
    store = FC.DTYPES["bf16" if out_bf16 else dtype]
    out = {}
    if epi.raw:
        out["raw"] = v.to(store).float()
    if epi.act:
        out["act"] = u.to(store).float()
    return out


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """(operands, {epilogue name: {dtype: expected}}) of an EXACT_CASES entry; shared, not to be modified."""
    c = CASES[name][0]
    op = exact_operands(c, _seed(name) + 1)
    return op, {en: {d: exact_expected(c, op, epi, d) for d in DTYPE_NAMES} for en, epi in EXACT_EPILOGUES.items()}
