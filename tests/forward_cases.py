"""Edge cases for the forward convolutions (csrc/conv.hip, csrc/conv_big.hip, csrc/conv64.hip behind ppn_conv2d_fused), their
f64 reference and a DERIVED per-element error bound.  Plain helper module (no tests): tests/test_forward_edges_cpu.py checks
that the cases are what they claim, that the reference is right and that the bound sees planted faults;
tests/test_forward_edges_gpu.py runs the kernels on them.

A case is Conv(B, ci, co, H, W, k, s, dil, pad): x NCHW [B, ci, H, W], weight [co, ci, k, k]; an epilogue is Epi (below).

Reference: F.conv2d in f64 on the operands ALREADY ROUNDED to the storage type, then the epilogue in f64 in the kernels' order
(conv64.hip:17, conv.hip:17):
    v = act1(acc * s1 + b1) (+ res);   out_raw = v;   out_act = act2(v * s2 + b2)
References are computed once per (case, dtype, epilogue) and shared: callers must not modify what they get.

Bound (per element; u = 2^-24, K = k * k * ci, S = conv2d(|x|, |w|) in f64):
    A         = (K + 4) u (S |s1| + |b1|)        f32 products and accumulation in any order ((n - 1) u sum |terms| is the
                                                 standard bound of an f32 sum of n terms in any order; bf16 x bf16 and f16 x f16
                                                 products are exact in f32), scale, shift, LReLU's multiplication
    bound_raw = u_out |ref_raw| + A (+ 2 u |res|) + tiny
    bound_act = u_out |ref_act| + |s2| (A + 2 u |res|) + 4 u (|v s2| + |b2|) + tiny
    u_out     = 2^-8 (bf16), 2^-11 (f16), 2^-23 (f32 stores);  tiny = 2^-126
ReLU and LReLU are 1-Lipschitz, so the error of their argument passes through unamplified.  Both outputs are computed from the
f32 value v (conv.hip:234-247, conv_big.hip:886-918, conv64.hip:253-276: out_act is NOT computed from the rounded out_raw), so
there is one rounding to the storage type per output and no further term.  The bound may be widened only by a named term for
a rounding step the kernel's source shows, with the line cited here; never to fit what a kernel returned.

What tests/test_forward_edges_cpu.py proves about it (a torch f32 emulation with one final rounding stays at ratio <= 1;
planted faults give ratio > 1 on a case with K <= 4608): see that file.  At K = 18432 (d54_2048_512 of test_conv_gpu.py) the
worst-case K u term is too loose to see a single lost element; no single-element sensitivity is claimed there.
"""
from __future__ import annotations

import collections
import functools

import torch
import torch.nn.functional as F

Conv = collections.namedtuple("Conv", "B ci co H W k s dil pad")
# s1 / b1 / res / s2b2: present or not; act1 / act2: 0 none, 1 ReLU, 2 LReLU(0.1); raw / act: which outputs are wanted
Epi = collections.namedtuple("Epi", "s1 b1 act1 res s2b2 act2 raw act")

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTYPE_NAMES = ("f32", "bf16", "f16")
U = 2.0 ** -24
U_OUT = {"f32": 2.0 ** -23, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TINY = 2.0 ** -126

EPILOGUES = {
    "plain": Epi(False, False, 0, False, False, 0, True, False),            # no scale or shift
    "bias_lrelu": Epi(False, True, 2, False, False, 0, True, False),
    "bn_relu": Epi(True, True, 1, False, False, 0, True, False),
    "bn": Epi(True, True, 0, False, False, 0, True, False),                 # BN, no activation
    "res_raw": Epi(False, False, 0, True, False, 0, True, False),           # residual, raw only
    "res_dual": Epi(False, False, 0, True, True, 1, True, True),            # residual + second output (conv2 of a BasicBlock)
    "act_only": Epi(True, True, 0, False, True, 1, False, True),            # second output only
    "res_lrelu2": Epi(False, False, 0, True, True, 2, True, True),          # residual + LReLU second output
}


def eff(c):
    return c.dil * (c.k - 1) + 1


def out_hw(c):
    return (c.H + 2 * c.pad - eff(c)) // c.s + 1, (c.W + 2 * c.pad - eff(c)) // c.s + 1


def pixels(c):
    Ho, Wo = out_hw(c)
    return c.B * Ho * Wo


def depth(c):
    return c.k * c.k * c.ci


# ---- the cases ----------------------------------------------------------------------------------------------------------------
# name -> (Conv, forced large tile or None, {dtype: purpose}).  A purpose is (kind, bp, bc, smallc, conditions): the kernel kind
# ("big" conv_igemm_big_kernel, "generic" conv_igemm_kernel, "conv64" conv64_kernel) and tile the (case, dtype) is meant to reach
# and a tuple of named conditions on the route, all checked by check_purpose() against what csrc/conv_route.cpp says
# (tests/test_forward_edges_cpu.py) -- a case that stops serving its purpose after a dispatch change fails there, not silently
# on the GPU.  Every case runs in every dtype: the dispatch refuses none of them.
#   imgs21     a pixel tile spans >= 21 images
#   notail     pixels % bp == 0 (an empty tail)
#   tail       pixels % bp != 0
#   one_ptile  a single, partial pixel tile
#   ct2        two channel tiles, the second partial
#   ct1p       one channel tile, partial (cout < bc)
#   kpad       the packed GEMM depth is larger than k * k * ci (zero weight columns, taps past the last read as zero)


def _all(kind, bp, bc, smallc, *cond):
    return {d: (kind, bp, bc, smallc, cond) for d in DTYPE_NAMES}


def _p16(p32, p16):
    return {"f32": p32, "bf16": p16, "f16": p16}


CASES = {
    # off-centre filter rows wholly in the padding (reach 4 > image): 64-channel large tile, then the 128- and 256-channel ones
    "reach_gt_image": (Conv(2, 64, 64, 3, 5, 3, 1, 4, 4), None, _all("big", 128, 64, False, "one_ptile")),
    "reach_gt_image_wide": (Conv(1, 128, 256, 3, 5, 3, 1, 4, 4), None, _all("big", 128, 128, False, "one_ptile")),
    "reach_gt_image_wide/256": (Conv(1, 128, 256, 3, 5, 3, 1, 4, 4), (128, 256), _all("big", 128, 256, False, "one_ptile")),
    # divisor 1 on one axis / on both (make_fastdiv(1) for div_wo / div_howo)
    "ho1": (Conv(2, 64, 128, 1, 37, 3, 1, 1, 1), None, _all("big", 128, 128, False, "one_ptile")),
    "wo1": (Conv(2, 64, 128, 37, 1, 3, 1, 1, 1), None, _all("big", 128, 128, False, "one_ptile")),
    "one_pixel": (Conv(3, 128, 64, 1, 1, 3, 1, 2, 2), None, _all("big", 128, 64, False, "one_ptile")),
    # stride 2 with an odd remainder on one axis only
    "s2_odd/3x3": (Conv(2, 64, 128, 18, 13, 3, 2, 1, 1), None, _all("big", 128, 128, False, "one_ptile")),
    "s2_odd/1x1": (Conv(2, 64, 128, 13, 18, 1, 2, 1, 0), None, _all("big", 128, 128, False, "one_ptile")),
    # pad 0 with 3x3 (Ho < H: outside conv64's scope)
    "valid": (Conv(1, 64, 64, 9, 12, 3, 1, 1, 0), None, _all("big", 128, 64, False, "one_ptile")),
    # pad 3 > the filter's reach dil (k - 1) = 2: the outermost ring of output pixels has no tap inside the image, its result is
    # act1(b1) (with pad 2 the last tap of the first row would still be row 0 of the image)
    "overpad": (Conv(1, 64, 64, 5, 6, 3, 1, 1, 3), None, _all("big", 128, 64, False, "one_ptile")),
    # 6 pixels per image: a 128-pixel tile spans 21 images; the image is smaller than conv64's 8 x 16 tile
    "many_images": (Conv(40, 64, 64, 2, 3, 3, 1, 1, 1), None,
                    _p16(("big", 128, 64, False, ("imgs21", "tail")), ("conv64", 0, 0, False, ()))),
    # M = 256: no tail on the 128-pixel tile and on the (forced) 256-pixel one
    "exact_tiles": (Conv(2, 64, 128, 8, 16, 3, 1, 1, 1), None, _all("big", 128, 128, False, "notail")),
    "exact_tiles/256": (Conv(2, 64, 128, 8, 16, 3, 1, 1, 1), (256, 128), _all("big", 256, 128, False, "notail")),
    # Cin = 8: K 72 -> 128 (16-bit) / 96 (f32); the 256 x 16 tile
    "cin8": (Conv(2, 8, 16, 9, 11, 3, 1, 1, 1), None, _all("generic", 256, 16, True, "kpad", "one_ptile")),
    # 5x5 on the small-Cin tile (K 400 -> 448 / 416; Cout 24 on the 32-channel tile) and on the 64-channel large tile (25 taps)
    "cin16_5x5": (Conv(2, 16, 24, 11, 9, 5, 1, 1, 2), None, _all("generic", 256, 32, True, "kpad", "ct1p", "one_ptile")),
    "c64_5x5": (Conv(1, 64, 64, 7, 9, 5, 1, 1, 2), None, _all("big", 128, 64, False, "one_ptile")),
    # partial channel tiles: 8 of 16 and 40 of 64 on the generic kernel, 72 = 64 + 8 live channels on the large-tile one
    "cout8": (Conv(1, 64, 8, 7, 9, 3, 1, 1, 1), None, _all("generic", 256, 16, False, "ct1p", "one_ptile")),
    "cout40": (Conv(1, 64, 40, 7, 9, 3, 1, 1, 1), None, _all("generic", 128, 64, False, "ct1p", "one_ptile")),
    "cout72": (Conv(1, 64, 72, 7, 9, 3, 1, 1, 1), None, _all("big", 128, 64, False, "ct2", "one_ptile")),
    # Cin 32 is below the K step in the 16-bit types only (f32's K step is 32: the large tile)
    "c32_1x1_s2": (Conv(1, 32, 64, 20, 20, 1, 2, 1, 0), None,
                   _p16(("big", 128, 64, False, ("one_ptile",)), ("generic", 128, 64, True, ("kpad", "one_ptile")))),
}
# the geometry cases run these two epilogues: the single-output one (the 16-bit single-pass epilogue where the tile has it) and
# the residual + second output one (the chunked f32 epilogue)
CASE_EPILOGUES = ("bn_relu", "res_dual")

# one ragged geometry per kernel kind, all eight epilogues
SWEEP = {
    "sweep/generic": (Conv(1, 32, 40, 7, 9, 3, 1, 1, 1), None,
                      _p16(("generic", 128, 64, False, ("ct1p", "one_ptile")), ("generic", 128, 64, True, ("ct1p", "kpad", "one_ptile")))),
    "sweep/big": (Conv(3, 64, 200, 17, 19, 3, 1, 1, 1), None, _all("big", 128, 128, False, "ct2", "tail")),
    "sweep/conv64": (Conv(2, 64, 64, 19, 37, 3, 1, 1, 1), None,
                     _p16(("big", 128, 64, False, ("tail",)), ("conv64", 0, 0, False, ()))),
}
ALL = dict(CASES, **SWEEP)
# (case, dtype) pairs that are ALSO run with the filter bank kernel switched off: the two kernels must agree bit for bit
CONV64_OFF = {"many_images": ("big", 128, 64, False, ("imgs21", "tail")), "sweep/conv64": ("big", 128, 64, False, ("tail",))}
# the shape of test_conv_tiles_gpu.py::test_forced_tile_single_output (K = 1152): the documented reason for the per-element bound
FORCED_TILE_SHAPE = Conv(2, 128, 200, 20, 23, 3, 1, 2, 2)


def runs():
    """[(case name, dtype name, epilogue name)] of everything the GPU test launches."""
    out = [(n, d, e) for n in CASES for d in DTYPE_NAMES for e in CASE_EPILOGUES]
    return out + [(n, d, e) for n in SWEEP for d in DTYPE_NAMES for e in EPILOGUES]


def kernel_name(purpose, dtype):
    """ppn_last_conv_kernel() of a purpose: the instantiation's name as csrc/conv_route.cpp kernel_name() writes it."""
    kind, bp, bc, smallc, _ = purpose
    elem = {"f32": "float", "bf16": "__bf16", "f16": "_Float16"}[dtype]
    if kind == "conv64":
        return "conv64_kernel<%s>" % elem
    if kind == "big":
        return "conv_igemm_big_kernel<%s, %d, %d, 8, false>" % (elem, bp, bc)
    return "conv_igemm_kernel<%s, %d, %d, %d, %d, %s>" % (elem, bp, bc, 4 if bc <= 32 else 2, 1 if bc <= 32 else 2,
                                                           "true" if smallc else "false")


def check_purpose(c, purpose, seg, k_total):
    """Why the route segment `seg` (a dict of tests/test_conv_route_cpu.py's SEG fields) does not serve `purpose`, or None."""
    kind, bp, bc, _, cond = purpose
    if seg["kind"] != kind:
        return "kernel kind %s, wanted %s" % (seg["kind"], kind)
    if kind == "conv64":
        return None
    if (seg["bp"], seg["bc"]) != (bp, bc):
        return "tile %dx%d, wanted %dx%d" % (seg["bp"], seg["bc"], bp, bc)
    m, (Ho, Wo) = pixels(c), out_hw(c)
    checks = {
        "imgs21": bp // (Ho * Wo) >= 21 and m >= bp,
        "notail": m % bp == 0 and seg["n_ptiles"] == m // bp,
        "tail": m % bp != 0 and seg["n_ptiles"] == m // bp + 1 >= 2,
        "one_ptile": m < bp and seg["n_ptiles"] == 1,
        "ct2": seg["n_ctiles"] == 2 and bc < c.co < 2 * bc,
        "ct1p": seg["n_ctiles"] == 1 and c.co < bc,
        "kpad": k_total > depth(c),
    }
    for name in cond:
        if not checks[name]:
            return "condition %s does not hold (M %d, n_ptiles %d, n_ctiles %d, k_total %d)" % (
                name, m, seg["n_ptiles"], seg["n_ctiles"], k_total)
    return None


# ---- operands, reference, bound -----------------------------------------------------------------------------------------------

def _seed(name):
    return 2000 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100000


def q(t, dtype):
    """Round to the storage type first (q() of test_conv_gpu.py, by dtype name): only accumulation and epilogue error is measured."""
    return t.to(DTYPES[dtype]).float()


def make_operands(c, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    Ho, Wo = out_hw(c)
    return {
        "x": q(torch.randn(c.B, c.ci, c.H, c.W, generator=g), dtype),
        "w": q(torch.randn(c.co, c.ci, c.k, c.k, generator=g) * (2.0 / depth(c)) ** 0.5, dtype),
        "s1": 0.5 + torch.rand(c.co, generator=g), "b1": torch.randn(c.co, generator=g) * 0.3,
        "s2": 0.5 + torch.rand(c.co, generator=g), "b2": torch.randn(c.co, generator=g) * 0.3,
        "res": q(torch.randn(c.B, c.co, Ho, Wo, generator=g), dtype),
    }


@functools.lru_cache(maxsize=None)
def operands(name, dtype):
    """x [B, ci, H, W], w [co, ci, k, k], res [B, co, Ho, Wo] (f32 tensors holding values of the storage type) and the f32
    per-channel vectors s1, b1, s2, b2.  Fixed seed per case; the epilogue picks what it uses."""
    return make_operands(ALL[name][0], dtype, _seed(name))


def act(v, a):
    return (lambda t: t, F.relu, lambda t: F.leaky_relu(t, 0.1))[a](v)


def epilogue(acc, op, epi):
    """(v, out_act or None) from the accumulators in the kernels' order, in acc's precision."""
    ch = lambda t: t.to(acc.dtype).view(1, -1, 1, 1)                                                     # noqa: E731
    v = acc
    if epi.s1:
        v = v * ch(op["s1"])
    if epi.b1:
        v = v + ch(op["b1"])
    v = act(v, epi.act1)
    if epi.res:
        v = v + op["res"].to(acc.dtype)
    u = act(v * ch(op["s2"]) + ch(op["b2"]), epi.act2) if epi.s2b2 else act(v, epi.act2)
    return v, (u if epi.act else None)


def conv_f64(c, op):
    """(acc, S): F.conv2d of the operands and of their magnitudes, f64."""
    x, w = op["x"].double(), op["w"].double()
    return F.conv2d(x, w, None, c.s, c.pad, c.dil), F.conv2d(x.abs(), w.abs(), None, c.s, c.pad, c.dil)


@functools.lru_cache(maxsize=None)
def _conv_f64(name, dtype):
    return conv_f64(ALL[name][0], operands(name, dtype))


def reference_of(c, op, epi, dtype, accs=None):
    """({"raw": ref, "act": ref}, {"raw": bound, "act": bound}), f64 NCHW, for the outputs the epilogue wants."""
    d = lambda t: t.double()                                                                             # noqa: E731
    acc, S = accs if accs is not None else conv_f64(c, op)
    v, u = epilogue(acc, op, epi)
    ch = lambda t: t.double().abs().view(1, -1, 1, 1)                                                    # noqa: E731
    A = (depth(c) + 4) * U * (S * (ch(op["s1"]) if epi.s1 else 1.0) + (ch(op["b1"]) if epi.b1 else 0.0))
    R = 2 * U * d(op["res"]).abs() if epi.res else 0.0
    ref, bound = {}, {}
    if epi.raw:
        ref["raw"] = v
        bound["raw"] = U_OUT[dtype] * v.abs() + A + R + TINY
    if epi.act:
        s2, b2 = (ch(op["s2"]), ch(op["b2"])) if epi.s2b2 else (1.0, 0.0)
        ref["act"] = u
        bound["act"] = U_OUT[dtype] * u.abs() + s2 * (A + R) + 4 * U * (v.abs() * s2 + b2) + TINY
    return ref, bound


@functools.lru_cache(maxsize=None)
def reference(name, dtype, epi_name):
    return reference_of(ALL[name][0], operands(name, dtype), EPILOGUES[epi_name], dtype, _conv_f64(name, dtype))


def ratio(got, ref, bound):
    """max(err / bound) over the tensor; a case passes at ratio <= 1.  A NaN in `got` gives inf."""
    r = (got.double() - ref).abs() / bound
    return float("inf") if torch.isnan(r).any() else float(r.max())


def worst(got, ref, bound):
    """(ratio, (b, channel, oy, ox)) of the worst element: where a finding sits."""
    r = torch.nan_to_num((got.double() - ref).abs() / bound, nan=float("inf"))
    i = int(r.argmax())
    return float(r.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape))


def ratios_of(dtype, x, w, stride=1, dil=1, pad=0, s1=None, b1=None, act1=0, residual=None, s2=None, b2=None, act2=0, raw=None,
              act=None):
    """The per-element bound for a launch of test_conv_gpu.run_conv with operands of the caller's own (already rounded to the
    storage type): {"raw": ratio, "act": ratio} for the outputs given (NCHW f32, as run_conv returns them)."""
    B, ci, H, W = x.shape
    co, _, k, _ = w.shape
    c = Conv(B, ci, co, H, W, k, stride, dil, pad)
    zero = torch.zeros(co)
    op = {"x": x, "w": w, "s1": s1 if s1 is not None else zero, "b1": b1 if b1 is not None else zero,
          "s2": s2 if s2 is not None else zero, "b2": b2 if b2 is not None else zero, "res": residual}
    assert (s2 is None) == (b2 is None)
    epi = Epi(s1 is not None, b1 is not None, act1, residual is not None, s2 is not None, act2, raw is not None, act is not None)
    ref, bound = reference_of(c, op, epi, dtype)
    got = {"raw": raw, "act": act}
    return {k_: ratio(got[k_], ref[k_], bound[k_]) for k_ in ref}


def conv_by_taps(c, x, w):
    """The convolution written out per filter tap (f64): y[b, o, oy, ox] = sum_{u, v, i} w[o, i, u, v] x[b, i, oy s - pad + u dil,
    ox s - pad + v dil], taps outside the image contributing nothing."""
    x, w = x.double(), w.double()
    Ho, Wo = out_hw(c)
    y = torch.zeros(c.B, c.co, Ho, Wo, dtype=torch.float64)
    for u in range(c.k):
        for v in range(c.k):
            for oy in range(Ho):
                iy = oy * c.s - c.pad + u * c.dil
                if not 0 <= iy < c.H:
                    continue
                for ox in range(Wo):
                    ix = ox * c.s - c.pad + v * c.dil
                    if 0 <= ix < c.W:
                        y[:, :, oy, ox] += x[:, :, iy, ix] @ w[:, :, u, v].t()
    return y


def no_tap_inside(c):
    """bool [Ho, Wo]: output pixels none of whose taps lies inside the image."""
    def axis(n, no):
        return torch.tensor([not any(0 <= o * c.s - c.pad + t * c.dil < n for t in range(c.k)) for o in range(no)])
    Ho, Wo = out_hw(c)
    return axis(c.H, Ho).view(-1, 1) | axis(c.W, Wo).view(1, -1)
