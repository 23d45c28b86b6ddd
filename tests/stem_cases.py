"""Edge cases for the stem kernels (csrc/stem.hip, stem3x3.hip, stem01.hip, stem012.hip, stem012_x3.hip): case lists, input
builders, the f64 references with the kernels' rounding points, and the error bounds the GPU results are held to.  Plain
helper module (no tests, no GPU, no import of the library): tests/test_stem_edges_cpu.py checks that the references are
right, that the bounds hold for an independent f32 emulation and that they notice defects; tests/test_stem_edges_gpu.py
runs the kernels.

Tensors are NCHW f64 inside this module and NHWC at its border (what the kernels store).  References and operands are
computed once per case and shared: callers must not modify what they get.

Bounds (u = 2^-24, one f32 rounding):
  single layer   operands already rounded to the kernel's storage type T; ref = relu(scale * conv64(a, w) + shift);
                 E_acc = (K + 4) u (|scale| sum|a||w| + |shift|), K = accumulated terms (147 / 144; 196 with the inside
                 channel), +4 = the epilogue's roundings (acc * scale + shift, contracted into an FMA or not).
                 MI355X_MICROARCH.md calls the f32 MFMA "exact f32" and documents no accumulation rounding of the 16-bit
                 MFMAs worse than one per term, so K u it is.
                 bound = E_acc + 1/2 ulp_T(|ref| + E_acc), per element.  No tolerance constant.
  fused, no twin the same with the patch, the weights and the two intermediate tensors rounded to the internal type (IEEE
                 half saturating at 65504) and the error carried from layer to layer:
                 e_L = |scale_L| conv(e_{L-1}, |w_L|) + E_acc + 1/2 ulp   (ReLU and the clamp are 1-Lipschitz);
                 E_acc takes |a| + e_{L-1} for |a|.  The second output relu(v * s3 + b3) is computed from the UNROUNDED v:
                 e_act = |s3| e_v + 2 u (|s3| (|v| + e_v) + |b3|) + 1/2 ulp.
  u8 table       ((float)x - mean) / std in IEEE f32 (numpy float32) rounded to the storage type.  ambiguous_entries()
                 lists the (channel, value) pairs whose storage rounding changes within +-4 f32 ulps of that quotient;
                 frames of kind "random" avoid them, every other frame adds one storage ulp per affected tap.
  exact input    u8 frames with half internals: the patch holds x - 128 and an inside channel, the weights are half(w / std)
                 and half(sum_c w_c (128 - mean_c) / std_c) (exact_in_weights); a weight whose rounding to half changes
                 within +-8 f32 ulps adds one half ulp of itself per tap in the same way.
"""
from __future__ import annotations

import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
F16_MAX = 65504.0
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
TYPES = {"f32": (torch.float32, 24, -126), "bf16": (torch.bfloat16, 8, -126), "f16": (torch.float16, 11, -14)}

# ---- the kernels' geometry, restated from their constants ---------------------------------------------------------------
# stem012.hip / stem012_x3.hip: a work unit is SW2 = 48 layer-2 columns x BAND2 = 16 layer-2 rows of one frame, walked in
# chunks of 2 layer-2 rows; units = B * ceil(Ho / 16) * ceil(Wo / 48), Ho = (H - 1) / 2 + 1.  The launchers cap the grid at
# 256 * per_cu = 512 work-groups (stem012, per_cu = 2) and 256 (stem012_x3): later units reuse the patch and the rings.
SW2, BAND2, CHUNK2 = 48, 16, 2
FUSED_GRID_CAP = {"stem012": 512, "stem012_x3": 256}
# stem.hip: 16 x 64 output tile, grid capped at 256 * 4.  stem01.hip: 16 x 78 tile, one work-group per tile (no cap).
STEM7_TILE, STEM7_GRID_CAP = (16, 64), 1024
STEM01_TILE = (16, 78)


def stem3_geo(T, stride):
    """Geo<T, COUT, S> of stem3x3.hip: (TH, TW) output tile, LDS bytes of the (TH*S+2) x (TW*S+2) x 16 patch, and the grid
    cap 256 * per_cu with per_cu from the LDS footprint (<= 40 KiB: 4, <= 53 KiB: 3, <= 80 KiB: 2, else 1)."""
    f32 = T == "f32"
    th = (8 if f32 else 16) if stride == 1 else 8
    tw = 32 if (f32 and stride == 2) else 64
    lds = (th * stride + 2) * (tw * stride + 2) * 16 * (4 if f32 else 2)
    per_cu = 4 if lds <= 40 * 1024 else 3 if lds <= 53 * 1024 else 2 if lds <= 80 * 1024 else 1
    return types.SimpleNamespace(th=th, tw=tw, lds=lds, cap=256 * per_cu)


def out_hw(h, w, stride=2):
    return (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1


def fused_units(b, h, w):
    ho, wo = out_hw(h, w)
    return b * ((ho + BAND2 - 1) // BAND2) * ((wo + SW2 - 1) // SW2)


def tiles(b, h, w, tile):
    return b * ((h + tile[0] - 1) // tile[0]) * ((w + tile[1] - 1) // tile[1])


def raw_s2_shape(b, h, w):
    ho, wo = out_hw(h, w)
    return (b, (ho + 1) // 2, (wo + 1) // 2, 32)


# ---- sizes (B, H, W) ----------------------------------------------------------------------------------------------------
# Fused stems.  TINY: smaller than the 7x7 filter, the 10-row patch and the 5- / 6-row rings.  BANDS: Ho = 15, 16, 16, 17, 18
# (a band of 15, of exactly 16 rows, 16 with an odd last input row, a second band of one row = half a chunk, and of one
# whole chunk) at odd widths, so the u8 row phases (b*H + y) * W * 3 mod 4 take all four values.  STRIPS: Wo = 48, 48, 49, 49,
# 96, 97 (a strip of exactly 48 columns from an odd and an even width, a second strip of ONE column, two full strips, a third
# strip of one column).  PHASE: five 5x7 frames of 105 bytes, frame bases at byte phases 0, 1, 2, 3, 0.  CAP: 130 frames of
# 33x97 = 130 * 2 * 2 = 520 units, past both grid caps, under 2 MB of input.
TINY = [(1, 1, 1), (1, 1, 7), (1, 7, 1), (1, 2, 2), (1, 3, 5), (1, 6, 6), (1, 4, 9)]
BANDS = [(1, h, w) for h in (29, 31, 32, 33, 35) for w in (41, 43)]
STRIPS = [(1, 9, w) for w in (95, 96, 97, 98, 191, 193)]
PHASE = [(5, 5, 7)]
CAP = [(130, 33, 97)]
FUSED_SIZES = BANDS + STRIPS + PHASE + CAP
CONTENT_SIZES = [(1, 33, 97), (2, 9, 98), (1, 35, 43), (3, 5, 7)]
CONTENT_KINDS = ["all256", "const0", "const128", "const255", "impulse", "ident", "neg", "sat"]


def _edge3(th, tw):
    return [(th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (th - 1, tw + 1), (th + 1, tw - 1)]


TINY_HW = [s[1:] for s in TINY]
STEM7_SIZES = [(1, h, w) for h, w in _edge3(*STEM7_TILE) + TINY_HW]
STEM01_SIZES = [(1, h, w) for h, w in _edge3(*STEM01_TILE) + TINY_HW]
STEM7_CAP = (257, 17, 65)               # 2 x 2 tiles per frame: 1028 tiles > 1024


def stem3_sizes(T, stride):
    """INPUT sizes whose output is tile-1, tile, tile+1 (mixed) of this instantiation, plus the tiny sizes.  Stride 2:
    output n comes from input 2n - 1 (odd) and 2n (even); both parities occur."""
    g = stem3_geo(T, stride)
    inp = (lambda n, k: n) if stride == 1 else (lambda n, k: 2 * n - (k & 1))
    return [(1, inp(h, k), inp(w, k + 1)) for k, (h, w) in enumerate(_edge3(g.th, g.tw))] + [(1, h, w) for h, w in TINY_HW]


# Content cases of the layer kernels: a 2 x 2-tile image (output tile + 2 in both dimensions, so the impulses on both sides
# of the tile seam exist and are no corner) and one image smaller than the filter.
STEM7_CONTENTS = ["const0", "const255", "impulse"]
STEM7_CONTENT_SIZES = [(1, STEM7_TILE[0] + 2, STEM7_TILE[1] + 2), (1, 3, 5)]
STEM3_CONTENTS = ["const", "impulse"]


def stem3_content_sizes(T, stride):
    g = stem3_geo(T, stride)
    return [(1, g.th + 2, g.tw + 2) if stride == 1 else (1, 2 * g.th + 3, 2 * g.tw + 4), (1, 3, 5)]


def stem3_seam(T, stride):
    """Input (row, column) under the centre tap of the second tile's first output row / column."""
    g = stem3_geo(T, stride)
    return (stride * g.th, stride * g.tw)


def stem3_cap_size(T, stride):
    """Copies of a 2 x 2-tile image (output (TH+1) x (TW+1)) until the tile count passes the cap."""
    g = stem3_geo(T, stride)
    h, w = (g.th + 1, g.tw + 1) if stride == 1 else (2 * g.th + 1, 2 * g.tw + 1)
    return (g.cap // 4 + 1, h, w)


# ---- number formats ---------------------------------------------------------------------------------------------------------

def rnd(x, T, clamp=True):
    """f64 -> storage type T -> f64.  IEEE half saturates at 65504 like to_store<> (stem012.hip)."""
    dt = TYPES[T][0]
    if T == "f16" and clamp:
        x = x.clamp(max=F16_MAX)
    return x.to(torch.float32).to(dt).double()


def ulp(x, T):
    """Spacing of T's values at |x| (f64 tensor), the subnormal spacing below the smallest normal."""
    _, p, emin = TYPES[T]
    e = torch.frexp(x.abs().clamp_min(2.0 ** emin)).exponent          # |x| = m 2^e, 1/2 <= m < 1
    return torch.ldexp(torch.ones_like(x), e - p)


def store_bound(p, d, T):
    """|stored - p| for a kernel whose f32 value is within d of p and is then rounded to T (clamped first for half)."""
    m = p.abs() + d
    if T == "f16":
        m = m.clamp(max=F16_MAX)
    return d + 0.5 * ulp(m, T)


# ---- input normalisation ------------------------------------------------------------------------------------------------

def normalise(frames):
    """u8 [B,H,W,3] numpy -> f32 NCHW torch: ((float)x - mean) / std in IEEE f32, as stem.hip and the table of stem012.hip."""
    m, s = np.asarray(MEAN, np.float32), np.asarray(STD, np.float32)
    v = (frames.astype(np.float32) - m) / s
    assert v.dtype == np.float32
    return torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)))


@functools.lru_cache(None)
def ambiguous_entries(T, ulps=4):
    """(channel, u8 value) pairs of the 3 x 256 table whose rounding to T changes within +-ulps f32 ulps of the quotient."""
    if T == "f32":
        return ()
    m, s = np.asarray(MEAN, np.float32), np.asarray(STD, np.float32)
    v = ((np.arange(256, dtype=np.float32)[None, :] - m[:, None]) / s[:, None]).astype(np.float32)
    lo, hi = v.copy(), v.copy()
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    r = lambda a: torch.from_numpy(a).to(TYPES[T][0]).float().numpy()
    return tuple((int(c), int(i)) for c, i in np.argwhere(r(lo) != r(hi)))


@functools.lru_cache(None)
def unambiguous_values():
    """u8 values that are unambiguous in every channel for bf16 and f16."""
    bad = {i for T in ("bf16", "f16") for _, i in ambiguous_entries(T)}
    return np.array([i for i in range(256) if i not in bad], np.uint8)


def ambiguity_mask(frames, T):
    """bool NCHW: the pixel's table entry is ambiguous for T."""
    m = np.zeros(frames.shape, bool)
    for c, i in ambiguous_entries(T):
        m[..., c] |= frames[..., c] == i
    return torch.from_numpy(m.transpose(0, 3, 1, 2).copy())


# ---- parameters and frames --------------------------------------------------------------------------------------------------

def _randn(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(None)
def params(kind="draw"):
    """w[3], s[4], b[4] (CPU f32): the draw of tests/test_stem_x3_gpu.py::_Stem, then
    draw: shift0 = shift1 = +2 (a padding computed as relu(bn(conv(0))) is an O(1) error at the border);
    neg:  every other channel's BN scale negative, shifts of the size of the convolution's spread (half the outputs at the kink);
    sat:  ident with scale0 ~ 3e6: layer-0 outputs pass 65504 and the pass-through layers carry the clamped ring values to
          both outputs, so a missing clamp (an inf, or the NaN of inf - inf that the ReLU turns into 0) is an error of
          65504 against a bound of a few percent of it (with the draw's layers 1 and 2 the propagated bound is as large as
          the outputs);
    ident: layers 1 and 2 pass their centre tap through (w = 1 at the centre of channel c -> c and c -> c + 16, scale 1,
          shift 0) and shift0 is small: the outputs are layer 0's at the even pixels, an impulse's response is the flipped
          7x7 filter, and the propagated bound stays at a few half ulps instead of growing by sum|w| ~ 14 per layer."""
    w = [_randn(16, 3, 7, 7, seed=31, scale=0.002), _randn(16, 16, 3, 3, seed=32, scale=0.12),
         _randn(32, 16, 3, 3, seed=33, scale=0.12)]
    gen = torch.Generator().manual_seed(34)
    s = [0.5 + torch.rand(n, generator=gen) for n in (16, 16, 32, 32)]
    b = [_randn(n, seed=35 + i, scale=0.3) for i, n in enumerate((16, 16, 32, 32))]
    if kind == "draw":
        b[0], b[1] = torch.full((16,), 2.0), torch.full((16,), 2.0)
    elif kind == "neg":
        for i in range(4):
            s[i] = s[i] * torch.tensor([1.0, -1.0]).repeat(s[i].numel() // 2)
        b = [_randn(n, seed=45 + i, scale=sc) for i, (n, sc) in enumerate(((16, 0.01), (16, 0.01), (32, 0.01), (32, 0.01)))]
    elif kind in ("ident", "sat"):
        w[1], w[2] = torch.zeros(16, 16, 3, 3), torch.zeros(32, 16, 3, 3)
        for c in range(16):
            w[1][c, c, 1, 1] = w[2][c, c, 1, 1] = w[2][c + 16, c, 1, 1] = 1.0
        s[1], s[2] = torch.ones(16), torch.ones(32)
        b[0], b[1], b[2] = _randn(16, seed=55, scale=0.01), torch.zeros(16), torch.zeros(32)
        if kind == "sat":
            s[0] = s[0] * 3e6
    else:
        assert kind == "plain"
    return types.SimpleNamespace(w=[t.contiguous() for t in w], s=[t.contiguous() for t in s], b=[t.contiguous() for t in b])


def params_of(content):
    return params(content if content in ("neg", "sat", "ident") else "ident" if content == "impulse" else "draw")


@functools.lru_cache(None)
def frames(content, B, H, W, seed=17):
    """u8 [B,H,W,3] numpy.  random / neg / sat / ident: uniform over the unambiguous values; all256: uniform over all values;
    constN; impulse: 128 with single 255 pixels at the four corners and on both sides of the strip seam (layer-2 columns
    47 | 48 = input columns 95 | 96) and the band seam (layer-2 rows 15 | 16 = input rows 31 | 32) of the fused stems and of
    the 16x64 tile seam of stem.hip (rows 15 | 16, columns 63 | 64), where the frame has them."""
    rng = np.random.default_rng(seed * 1000003 + B * 10007 + H * 101 + W)
    if content in ("random", "neg", "sat", "ident"):
        vals = unambiguous_values()
        f = vals[rng.integers(0, len(vals), size=(B, H, W, 3))]
    elif content == "all256":
        f = rng.integers(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    elif content.startswith("const"):
        f = np.full((B, H, W, 3), int(content[5:]), np.uint8)
    else:
        assert content == "impulse"
        f = np.full((B, H, W, 3), 128, np.uint8)
        for k, (y, x) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (31, 95), (32, 96), (31, 3), (32, 5),
                                    (2, 95), (4, 96), (15, 63), (16, 64))):     # the last two: stem.hip's 16x64 tile seam
            if 0 <= y < H and 0 <= x < W:
                f[k % B, y, x, k % 3] = 255
    f = np.ascontiguousarray(f, np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(None)
def activations(T, B, H, W, seed=7, content="random", seam=None):
    """NHWC input of a stem3x3 launch, already in T (as f32 values).  random: half-normal with a fifth of exact zeros, like
    a ReLU output; const: 1.5 everywhere (every output sees the same taps, fewer of them at the border); impulse: zeros with
    single pixels of 1.0 (one channel each) at the four corners and on both sides of `seam` = (row, column), the first input
    row / column of the second tile, where the image has them."""
    if content == "const":
        return torch.full((B, H, W, 16), 1.5)
    if content == "impulse":
        x = torch.zeros(B, H, W, 16)
        sy, sx = seam
        for k, (y, c) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (sy - 1, sx - 1), (sy, sx), (sy - 1, 1),
                                    (1, sx))):
            if 0 <= y < H and 0 <= c < W:
                x[k % B, y, c, (5 * k) % 16] = 1.0
        return x
    assert content == "random"
    g = torch.Generator().manual_seed(seed * 7919 + H * 131 + W)
    x = torch.randn(B, H, W, 16, generator=g).abs() * (torch.rand(B, H, W, 16, generator=g) > 0.2)
    return x.to(TYPES[T][0]).float().contiguous()


# ---- f64 references -------------------------------------------------------------------------------------------------------

def _v(t):
    return t.double().view(1, -1, 1, 1)


def layer_ref(a, w, s, b, stride, pad, K, relu=True, e_in=None, e_w=None):
    """a, w: f64, already rounded to the storage type.  -> (p, d): p = [relu](s * conv(a, w) + b) in f64 and d >= |the
    kernel's f32 value before its store - p|, for a kernel whose input is within e_in of a and whose weights within e_w of w."""
    c = F.conv2d(a, w, None, stride, pad)
    aa = a.abs() if e_in is None else a.abs() + e_in
    m = F.conv2d(aa, w.abs(), None, stride, pad)
    sv = _v(s) if s is not None else 1.0
    bv = _v(b) if b is not None else 0.0
    p = c * sv + bv
    d = (K + 4) * U * (m * abs(sv) + abs(bv))
    if e_in is not None:
        d = d + F.conv2d(e_in, w.abs(), None, stride, pad) * abs(sv)
    if e_w is not None:
        d = d + F.conv2d(aa, e_w, None, stride, pad) * abs(sv)
    return (p.clamp_min(0.0) if relu else p), d


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def single_ref(a_nchw, w, s, b, stride, pad, T, relu=True, s2=None, b2=None):
    """Single layer, bound 1: operands rounded to T here.  -> dict raw=(ref, bound) [act=(ref, bound)] NHWC f64."""
    a, wq = rnd(a_nchw.double(), T), rnd(w.double(), T)
    p, d = layer_ref(a, wq, s, b, stride, pad, K=w[0].numel(), relu=relu)
    out = {"raw": (nhwc(p), nhwc(store_bound(p, d, T)))}
    if s2 is not None:
        out["act"] = tuple(nhwc(t) for t in _act_ref(p, d, s2, b2, T))
    return out


def _act_ref(p, d, s3, b3, T):
    pa = (p * _v(s3) + _v(b3)).clamp_min(0.0)
    da = _v(s3).abs() * d + 2 * U * (_v(s3).abs() * (p.abs() + d) + _v(b3).abs())
    return pa, store_bound(pa, da, T)


def exact_in_weights(w0, T="f16", ulps=8):
    """kExactIn (stem012.hip): [16][4][7][7] = half(w_c / std_c) and the inside channel half(sum_c w_c (128 - mean_c) / std_c),
    every step in f32 in the kernel's order.  The compiler may contract the sum's steps into FMAs and the divisions need not
    be IEEE-rounded, so a weight whose rounding to half changes within +-ulps f32 ulps of the value computed here is
    AMBIGUOUS: e_w holds one storage ulp for it (the candidates are neighbours), 0 elsewhere.
    -> (weights as f64, e_w, the f32 values before the rounding to half)."""
    w = w0.numpy().astype(np.float32)
    m, s = np.asarray(MEAN, np.float32), np.asarray(STD, np.float32)
    out = np.zeros((16, 4, 7, 7), np.float32)
    v = np.zeros((16, 7, 7), np.float32)
    for c in range(3):
        out[:, c] = w[:, c] / s[c]
        v = (v + w[:, c] * ((np.float32(128.0) - m[c]) / s[c])).astype(np.float32)
    out[:, 3] = v
    lo, hi = out.copy(), out.copy()
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    q = rnd(torch.from_numpy(out).double(), T)
    amb = rnd(torch.from_numpy(lo).double(), T) != rnd(torch.from_numpy(hi).double(), T)
    return q, amb.double() * ulp(q, T), torch.from_numpy(out)


def fused_ref(P, fr=None, xn=None, internal="f16", out="f16", exact_in=False, layers=3):
    """The fused stem with its rounding points in f64.  fr: u8 frames (table or exact-input path), xn: f32 NCHW input.
    -> namespace raw=(ref, bound), act=(ref, bound) NHWC f64, overflow0 = number of layer-0 values past 65504 before the
    clamp, a0 / a1 = the emulated intermediate tensors (NCHW).  layers=2: layers 0 and 1 only (stem01), raw = layer 1."""
    H = internal
    w = [rnd(t.double(), H) for t in P.w]
    e_patch, e_w0, K0 = None, None, 147
    if exact_in:
        assert fr is not None
        x = torch.from_numpy(fr.transpose(0, 3, 1, 2).copy()).double() - 128.0
        patch = torch.cat([x, torch.ones_like(x[:, :1])], 1)
        (w[0], e_w0, _), K0 = exact_in_weights(P.w[0], H), 196
    else:
        v = normalise(fr) if fr is not None else xn
        patch = rnd(v.double(), H)
        if fr is not None and ambiguity_mask(fr, H).any():
            e_patch = ambiguity_mask(fr, H).double() * ulp(patch, H)
    p0, d0 = layer_ref(patch, w[0], P.s[0], P.b[0], 1, 3, K0, e_in=e_patch, e_w=e_w0)
    a0, e0 = rnd(p0, H), store_bound(p0, d0, H)
    p1, d1 = layer_ref(a0, w[1], P.s[1], P.b[1], 1, 1, 144, e_in=e0)
    res = types.SimpleNamespace(a0=a0, overflow0=int((p0 > F16_MAX).sum()), overflow1=int((p1 > F16_MAX).sum()))
    clampo = (lambda t: t.clamp(max=F16_MAX)) if out == "f16" else (lambda t: t)
    if layers == 2:
        res.raw = (nhwc(clampo(p1)), nhwc(store_bound(p1, d1, out)))
        return res
    a1, e1 = rnd(p1, H), store_bound(p1, d1, H)
    p2, d2 = layer_ref(a1, w[2], P.s[2], P.b[2], 2, 1, 144, e_in=e1)
    pa, ba = _act_ref(p2, d2, P.s[3], P.b[3], out)
    res.a1 = a1
    res.raw = (nhwc(clampo(p2)), nhwc(store_bound(p2, d2, out)))
    res.act = (nhwc(clampo(pa)), nhwc(ba))
    return res


def plain_ref(P, xn):
    """fp64, no rounding point: the three layers and relu(bn1(x)) -> NHWC (raw, act): the reference of STEM_X3_TOL."""
    y = F.relu(F.conv2d(xn.double(), P.w[0].double(), None, 1, 3) * _v(P.s[0]) + _v(P.b[0]))
    y = F.relu(F.conv2d(y, P.w[1].double(), None, 1, 1) * _v(P.s[1]) + _v(P.b[1]))
    y = F.relu(F.conv2d(y, P.w[2].double(), None, 2, 1) * _v(P.s[2]) + _v(P.b[2]))
    return nhwc(y), nhwc(F.relu(y * _v(P.s[3]) + _v(P.b[3])))


def ratio(got, ref_bound):
    """max err / bound over the tensor (inf for a NaN / inf in got)."""
    ref, bound = ref_bound
    r = (got.double() - ref).abs() / bound
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def bf16_interval_ok(out_bf16, out_f16):
    """Bound 5: both outputs are store roundings of the same f32 value v; v lies within half an f16 ulp of out_f16, so
    bf16(lo) <= out_bf16 <= bf16(hi) with [lo, hi] = out_f16 -+ 1/2 ulp_f16 (rounding is monotone)."""
    x = out_f16.double()
    h = 0.5 * ulp(x, "f16")
    # below a power of two the spacing under x is half of ulp(x): the wider interval is still a valid enclosure of v
    lo, hi = rnd((x - h).clamp_min(0.0), "bf16"), rnd(x + h, "bf16")
    g = out_bf16.double()
    return bool(((lo <= g) & (g <= hi)).all())


# ---- independent f32 emulation (torch CPU float32 convolutions) and its mutants -------------------------------------------

MUTANTS = ("pad_u8_zero", "l1_pad_relu_shift0", "swap_rb", "strip_shift", "stale_ring", "no_clamp")


def _q32(t, T, clamp=True):
    if T == "f16" and clamp:
        t = t.clamp(max=F16_MAX)
    return t.to(TYPES[T][0]).float()


def _conv32(a, w, s, b, stride, pad, padval=None):
    if padval is not None and pad:
        ap = padval.view(1, -1, 1, 1).expand(a.shape[0], -1, a.shape[2] + 2 * pad, a.shape[3] + 2 * pad).clone()
        ap[:, :, pad:-pad, pad:-pad] = a
        a, pad = ap, 0
    t = F.conv2d(a, w, None, stride, pad) * s.view(1, -1, 1, 1)
    return (t + b.view(1, -1, 1, 1)).clamp_min(0.0)


def fused_emu32(P, fr=None, xn=None, internal="f16", out="f16", exact_in=False, mutant=None, layers=3):
    """What a correct kernel may return: float32 convolutions of the rounded operands, intermediates rounded at the kernel's
    points.  -> (raw, act) NHWC in f32 holding values of the output type.  mutant: one of MUTANTS, a defect of the kind the
    GPU tests are there to notice."""
    H, clamp = internal, mutant != "no_clamp"
    w = [_q32(t, H) for t in P.w]
    if mutant == "swap_rb":
        if fr is not None:
            fr = fr[..., ::-1]
        else:
            xn = xn.flip(1)
    padval = None
    if exact_in:
        x = torch.from_numpy(fr.transpose(0, 3, 1, 2).copy()).float() - 128.0
        patch = torch.cat([x, torch.ones_like(x[:, :1])], 1)
        # derived here in torch float32, NOT taken from exact_in_weights (which the reference uses): an error in w / std or in
        # the inside channel there must not cancel between reference and emulation.  torch's sum need not add in the kernel's
        # order; the reference's e_w covers that
        m, sd = torch.tensor(MEAN), torch.tensor(STD)
        w4 = (P.w[0] * ((128.0 - m) / sd).view(1, 3, 1, 1)).sum(1, keepdim=True)
        w[0] = _q32(torch.cat([P.w[0] / sd.view(1, 3, 1, 1), w4], 1), H)
        if mutant == "pad_u8_zero":
            padval = torch.tensor([-128.0, -128.0, -128.0, 1.0])
    else:
        patch = _q32(normalise(fr) if fr is not None else xn, H)
        if mutant == "pad_u8_zero":
            padval = _q32(normalise(np.zeros((1, 1, 1, 3), np.uint8)).view(3), H)
    a0 = _q32(_conv32(patch, w[0], P.s[0], P.b[0], 1, 3, padval), H, clamp)
    pad1 = _q32(P.b[0].clamp_min(0.0), H) if mutant == "l1_pad_relu_shift0" else None
    t1 = _conv32(a0, w[1], P.s[1], P.b[1], 1, 1, pad1)
    if layers == 2:
        return nhwc(_q32(t1, out, clamp)), None
    a1 = _q32(t1, H, clamp)
    v = _conv32(a1, w[2], P.s[2], P.b[2], 2, 1)
    if mutant == "stale_ring" and v.shape[2] > BAND2:
        # the first layer-2 row of the second band reads layer-1 row 2*16 - 1 from a ring slot that still holds the row
        # R1 = 5 rows earlier
        am = a1.clone()
        am[:, :, 2 * BAND2 - 1] = a1[:, :, 2 * BAND2 - 1 - 5]
        v[:, :, BAND2] = _conv32(am, w[2], P.s[2], P.b[2], 2, 1)[:, :, BAND2]
    if mutant == "strip_shift" and v.shape[3] > SW2:
        # the second strip computes every column one to the left of where it stores it
        n = min(2 * SW2, v.shape[3]) - SW2
        v = v.clone()
        v[:, :, :, SW2:SW2 + n] = v[:, :, :, SW2 - 1:SW2 - 1 + n].clone()
    u = (v * P.s[3].view(1, -1, 1, 1) + P.b[3].view(1, -1, 1, 1)).clamp_min(0.0)
    return nhwc(_q32(v, out, clamp)), nhwc(_q32(u, out, clamp))


# ---- the fused variants the GPU test runs -----------------------------------------------------------------------------------
# name -> (internal type, output type).  u8 frames with half internals take the exact-input path (kExactIn).
VARIANTS = {"bf16": ("bf16", "bf16"), "f16": ("f16", "f16"), "f16_bf16": ("f16", "bf16")}


def is_exact_in(variant, u8):
    return bool(u8) and VARIANTS[variant][0] == "f16"


@functools.lru_cache(maxsize=64)
def fused_case_ref(content, B, H, W, variant, u8):
    internal, out = VARIANTS[variant]
    fr = frames(content, B, H, W)
    P = params_of(content)
    if u8:
        return fused_ref(P, fr=fr, internal=internal, out=out, exact_in=is_exact_in(variant, True))
    return fused_ref(P, xn=normalise(fr), internal=internal, out=out)


def fused_runs(sizes, contents=("random",), variants=tuple(VARIANTS)):
    return [(v, bool(u8), c, s) for v in variants for u8 in (1, 0) for c in contents for s in sizes]


def run_id(r):
    v, u8, c, (B, H, W) = r
    return f"{v}-{'u8' if u8 else 'f32in'}-{c}-{B}x{H}x{W}"
