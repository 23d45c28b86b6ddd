"""The stem kernels (csrc/stem.hip, stem3x3.hip, stem01.hip, stem012.hip, stem012_x3.hip) on the cases of tests/stem_cases.py:
every dtype variant of the fused stem (PPN_BF16, PPN_F16, PPN_STEM_IO(PPN_F16, PPN_BF16), each with PPN_STEM_RAW_S2, the
exact-input path u8 frames take with half internals, the split-f16 stem) and the layer kernels (ppn_stem7x7 in eval and
train mode, ppn_stem01, stem3x3 at both strides) in f32 and bf16, at tile / strip / band / image edges, past every
launcher's grid cap, on constant, impulse, negative-scale and saturating content.

Every output is allocated with a NaN body and a 4096-element sentinel tail: after the launch the body holds no NaN and the
tail is untouched.  Values are held to the per-element bounds of stem_cases.py (no tolerance constant) or, where a kernel has
a bitwise twin, to torch.equal.  The tests print the worst err / bound of every output (lines starting STEM_EDGE;
profiles/stem_edge_errors.txt holds one run's) and assert that none exceeds 1."""
import collections
import ctypes as C

import pytest
import torch

import stem_cases as SC
from test_stem_x3_gpu import STEM_X3_TOL

pytestmark = pytest.mark.gpu

TAIL = 4096                                  # sentinel elements behind every output: 8 KiB (16-bit) / 16 KiB (f32)
SENTINEL = -777.0
WORST = collections.defaultdict(float)       # (kernel, variant, output) -> worst err / bound of this run


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class _Out:
    """An output tensor with a NaN body and a sentinel tail."""

    def __init__(self, shape, dtype):
        self.n = 1
        for s in shape:
            self.n *= s
        self.buf = torch.full((self.n + TAIL,), float("nan"), dtype=dtype, device="cuda")
        self.buf[self.n:] = SENTINEL
        self.t = self.buf[:self.n].view(shape)

    def ptr(self):
        return self.t.data_ptr()

    def checked(self, what):
        assert not torch.isnan(self.t).any(), f"{what}: a NaN is left in the body"
        assert torch.equal(self.buf[self.n:], torch.full_like(self.buf[self.n:], SENTINEL)), f"{what}: the tail was written"
        return self.t


def _tdt(T):
    return SC.TYPES[T][0]


def _code(T):
    from pytorch_pose_proposal_network_amd import lib as L
    return {"f32": L.PPN_F32, "bf16": L.PPN_BF16, "f16": L.PPN_F16}[T]


class _Dev:
    """A parameter set of stem_cases.params on the device."""

    def __init__(self, P):
        self.P = P
        self.w = [t.cuda() for t in P.w]
        self.s = [t.cuda() for t in P.s]
        self.b = [t.cuda() for t in P.b]
        self.m3, self.s3 = (C.c_float * 3)(*SC.MEAN), (C.c_float * 3)(*SC.STD)
        self.zero = torch.zeros(64, device="cuda")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _src(content, B, H, W, u8):
    fr = SC.frames(content, B, H, W)
    return (torch.from_numpy(fr.copy()) if u8 else SC.normalise(fr)).contiguous().cuda()


def _stem7(D, T, u8, src, B, H, W, train=False):
    from pytorch_pose_proposal_network_amd import lib as L
    out = _Out((B, H, W, 16), _tdt(T))
    L.check(L.load().ppn_stem7x7(_code(T), int(u8), src.data_ptr(), B, H, W, D.w[0].data_ptr(),
                                 None if train else D.s[0].data_ptr(), None if train else D.b[0].data_ptr(), D.m3, D.s3,
                                 out.ptr(), _stream()), "ppn_stem7x7")
    torch.cuda.synchronize()
    return out.checked("ppn_stem7x7")


def _stem01(D, T, u8, src, B, H, W):
    from pytorch_pose_proposal_network_amd import lib as L
    out = _Out((B, H, W, 16), _tdt(T))
    L.check(L.load().ppn_stem01(_code(T), int(u8), src.data_ptr(), B, H, W, D.w[0].data_ptr(), D.s[0].data_ptr(),
                                D.b[0].data_ptr(), D.m3, D.s3, D.w[1].data_ptr(), D.s[1].data_ptr(), D.b[1].data_ptr(),
                                out.ptr(), _stream()), "ppn_stem01")
    torch.cuda.synchronize()
    return out.checked("ppn_stem01")


def _conv3(D, T, x, layer, stride, act):
    """stem3x3 through ppn_conv2d_fused: x NHWC on the device in T, weights / BN of stem layer `layer` (1: 16 -> 16,
    2: 16 -> 32)."""
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    B, H, W, _ = x.shape
    cout = D.w[layer].shape[0]
    Ho, Wo = SC.out_hw(H, W, stride)
    raw, a = _Out((B, Ho, Wo, cout), _tdt(T)), (_Out((B, Ho, Wo, cout), _tdt(T)) if act else None)
    _, _, _, ktot, cpad = L.conv_tiling(_code(T), 16, cout, 3)
    d = L.ConvDesc()
    d.dtype, d.batch, d.in_h, d.in_w, d.cin = _code(T), B, H, W, 16
    d.out_h, d.out_w, d.cout = Ho, Wo, cout
    d.ksize, d.stride, d.dilation, d.pad = 3, stride, 1, 1
    d.k_total, d.cout_pad, d.act1, d.act2 = ktot, cpad, 1, int(act)
    d.src, d.weight, d.zero_page = x.data_ptr(), D.w[layer].data_ptr(), D.zero.data_ptr()
    d.scale1, d.shift1, d.out_raw = D.s[layer].data_ptr(), D.b[layer].data_ptr(), raw.ptr()
    if act:
        s3, b3 = D.s[3][:cout].contiguous(), D.b[3][:cout].contiguous()
        d.scale2, d.shift2, d.out_act = s3.data_ptr(), b3.data_ptr(), a.ptr()
    L.check(lib.ppn_conv2d_fused(C.byref(d), _stream()), "ppn_conv2d_fused")
    name = lib.ppn_last_conv_kernel().decode()
    assert name == f"stem3x3_kernel<{'float' if T == 'f32' else '__bf16'}, {cout}, {stride}>", name
    torch.cuda.synchronize()
    return raw.checked(name + " raw"), (a.checked(name + " act") if act else None)


def _fused_code(variant, raw_s2=False):
    from pytorch_pose_proposal_network_amd import lib as L
    code = {"bf16": L.PPN_BF16, "f16": L.PPN_F16, "f16_bf16": L.PPN_STEM_IO(L.PPN_F16, L.PPN_BF16),
            "x3": L.PPN_STEM_IO(L.PPN_F16X3, L.PPN_F32)}[variant]
    return code | (L.PPN_STEM_RAW_S2 if raw_s2 else 0)


def _fused(D, variant, u8, src, B, H, W, raw=True, act=True, raw_s2=False, plain_entry=False):
    """ppn_stem012_dt (or ppn_stem012, the bf16 entry point) -> (raw, act), guards checked."""
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    odt = torch.float32 if variant == "x3" else _tdt(SC.VARIANTS[variant][1])
    Ho, Wo = SC.out_hw(H, W)
    o_raw = _Out(SC.raw_s2_shape(B, H, W) if raw_s2 else (B, Ho, Wo, 32), odt) if raw else None
    o_act = _Out((B, Ho, Wo, 32), odt) if act else None
    args = [int(u8), src.data_ptr(), B, H, W, D.w[0].data_ptr(), D.s[0].data_ptr(), D.b[0].data_ptr(), D.m3, D.s3,
            D.w[1].data_ptr(), D.s[1].data_ptr(), D.b[1].data_ptr(), D.w[2].data_ptr(), D.s[2].data_ptr(), D.b[2].data_ptr(),
            D.s[3].data_ptr(), D.b[3].data_ptr(), o_raw.ptr() if raw else None, o_act.ptr() if act else None, _stream()]
    if plain_entry:
        assert variant == "bf16" and not raw_s2
        L.check(lib.ppn_stem012(*args), "ppn_stem012")
    else:
        L.check(lib.ppn_stem012_dt(_fused_code(variant, raw_s2), *args), "ppn_stem012_dt")
    torch.cuda.synchronize()
    what = f"stem012 {variant}{'+raw_s2' if raw_s2 else ''}"
    return (o_raw.checked(what + " raw") if raw else None), (o_act.checked(what + " act") if act else None)


def _chain(D, T, u8, src, B, H, W, layers=3):
    """ppn_stem7x7 -> stem3x3<16,1> [-> stem3x3<32,2>] in T: the layer-by-layer twin of the fused kernels."""
    t0 = _stem7(D, T, u8, src, B, H, W)
    t1, _ = _conv3(D, T, t0, 1, 1, act=False)
    if layers == 2:
        return t0, t1, None, None
    raw, act = _conv3(D, T, t1, 2, 2, act=True)
    return t0, t1, raw, act


def _report(kernel, variant, tag, ratios, extra=""):
    for k, v in ratios.items():
        WORST[(kernel, variant, k)] = max(WORST[(kernel, variant, k)], v)
    print(f"STEM_EDGE {kernel} {variant} {tag}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + extra)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (kernel, variant, tag, bad)


def _sz(s):
    return "x".join(str(v) for v in s)


# ---- layer kernels --------------------------------------------------------------------------------------------------------

def _check_stem7(T, u8, train, size, content="random"):
    B, H, W = size
    D = _Dev(SC.params("draw"))
    got = _stem7(D, T, u8, _src(content, B, H, W, u8), B, H, W, train=train)
    xn = SC.normalise(SC.frames(content, B, H, W))
    P = D.P
    ref = SC.single_ref(xn, P.w[0], None if train else P.s[0], None if train else P.b[0], 1, 3, T, relu=not train)
    _report("stem7x7", f"{T}{'-train' if train else ''}",
            f"{'u8' if u8 else 'f32in'} {'' if content == 'random' else content + ' '}{_sz(size)}",
            {"out": SC.ratio(got.cpu(), ref["raw"])})


@pytest.mark.parametrize("size", SC.STEM7_SIZES, ids=_sz)
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32in"])
@pytest.mark.parametrize("T", ["f32", "bf16"])
def test_stem7x7_edges(T, u8, mode, size):
    """ppn_stem7x7 at tile-1 / tile / tile+1 of its 16x64 tile and on images smaller than the filter, with BN + ReLU and in
    train mode (scale == shift == NULL: the plain convolution, no ReLU), against the f64 convolution (single-layer bound)."""
    _check_stem7(T, u8, mode == "train", size)


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("T", ["f32", "bf16"])
def test_stem7x7_past_the_grid_cap(T, mode):
    """257 frames of 2 x 2 tiles = 1028 tiles on a grid capped at 1024: some work-groups stage a second patch."""
    assert SC.tiles(*SC.STEM7_CAP, SC.STEM7_TILE) > SC.STEM7_GRID_CAP
    _check_stem7(T, True, mode == "train", SC.STEM7_CAP)


@pytest.mark.parametrize("size", SC.STEM7_CONTENT_SIZES, ids=_sz)
@pytest.mark.parametrize("content", SC.STEM7_CONTENTS)
@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32in"])
@pytest.mark.parametrize("T", ["f32", "bf16"])
def test_stem7x7_content(T, u8, mode, content, size):
    """Constant frames of 0 and 255 (with shift0 = 2 and u8 0 normalising to about -2, a border padded with anything but the
    normalised zero is far outside the bound) and impulses at the corners and on both sides of the 16x64 tile seam (the
    response is the flipped filter), on a 2 x 2-tile image and on one smaller than the filter."""
    _check_stem7(T, u8, mode == "train", size, content)


def _check_stem3(T, stride, size, content="random"):
    B, H, W = size
    D = _Dev(SC.params("draw"))
    x = SC.activations(T, B, H, W, content=content, seam=SC.stem3_seam(T, stride))
    act = stride == 2
    raw, a = _conv3(D, T, x.to(_tdt(T)).cuda(), stride, stride, act=act)
    P = D.P
    cout = P.w[stride].shape[0]
    ref = SC.single_ref(SC.nchw(x), P.w[stride], P.s[stride], P.b[stride], stride, 1, T,
                        s2=P.s[3][:cout] if act else None, b2=P.b[3][:cout] if act else None)
    ratios = {"raw": SC.ratio(raw.cpu(), ref["raw"])}
    if act:
        ratios["act"] = SC.ratio(a.cpu(), ref["act"])
    _report(f"stem3x3<{cout},{stride}>", T, ("" if content == "random" else content + " ") + _sz(size), ratios)


def _stem3_runs():
    return [(T, s, size) for T in ("f32", "bf16") for s in (1, 2) for size in SC.stem3_sizes(T, s)]


@pytest.mark.parametrize("T,stride,size", _stem3_runs(), ids=lambda v: _sz(v) if isinstance(v, tuple) else str(v))
def test_stem3x3_edges(T, stride, size):
    """stem3x3<16,1> and stem3x3<32,2> (the latter with its second output) through ppn_conv2d_fused, at tile-1 / tile / tile+1
    of each instantiation's Geo tile and on tiny images; the kernel name is asserted."""
    _check_stem3(T, stride, size)


@pytest.mark.parametrize("T,stride,content,size", [(T, s, c, size) for T in ("f32", "bf16") for s in (1, 2)
                                                   for c in SC.STEM3_CONTENTS for size in SC.stem3_content_sizes(T, s)],
                         ids=lambda v: _sz(v) if isinstance(v, tuple) else str(v))
def test_stem3x3_content(T, stride, content, size):
    """A constant activation (every output sees the same taps, fewer at the border: the padding is zero) and impulses at
    the corners and on both sides of the tile seam (the response is the flipped 3x3 filter, a misaddressed tap moves it), on
    a 2 x 2-tile image and on a 3x5 one."""
    _check_stem3(T, stride, size, content)


@pytest.mark.parametrize("T,stride", [(T, s) for T in ("f32", "bf16") for s in (1, 2)])
def test_stem3x3_past_the_grid_cap(T, stride):
    g, size = SC.stem3_geo(T, stride), SC.stem3_cap_size(T, stride)
    assert SC.tiles(size[0], *SC.out_hw(size[1], size[2], stride), (g.th, g.tw)) > g.cap
    _check_stem3(T, stride, size)


@pytest.mark.parametrize("size", SC.STEM01_SIZES + [(3, 33, 157)], ids=_sz)
@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32in"])
@pytest.mark.parametrize("T", ["f32", "bf16"])
def test_stem01_edges(T, u8, size):
    """ppn_stem01 (layer 0 + layer 1 in one launch; one work-group per 16x78 tile, so no grid cap) at tile-1 / tile / tile+1,
    on tiny images and on three frames of 3 x 3 tiles.  stem01.hip has the rounding points and the MFMA order of stem.hip
    followed by stem3x3<16,1> (same k layouts, same epilogue expressions, zero outside the image), so it is held to
    torch.equal with that chain, and to the fused bound of stem_cases.py as well."""
    B, H, W = size
    D = _Dev(SC.params("draw"))
    src = _src("random", B, H, W, u8)
    got = _stem01(D, T, u8, src, B, H, W)
    _, t1, _, _ = _chain(D, T, u8, src, B, H, W, layers=2)
    fr = SC.frames("random", B, H, W)
    ref = SC.fused_ref(D.P, fr=fr, internal=T, out=T, layers=2) if u8 else \
        SC.fused_ref(D.P, xn=SC.normalise(fr), internal=T, out=T, layers=2)
    _report("stem01", T, f"{'u8' if u8 else 'f32in'} {_sz(size)}", {"out": SC.ratio(got.cpu(), ref.raw)},
            f", differs from the chain in {int((_bits(got) != _bits(t1)).sum())} elements")
    assert _same(got, t1)


# ---- fused stems ------------------------------------------------------------------------------------------------------------

def _input_id(variant, u8):
    """u8 frames take the exact-input path (kExactIn) with half internals and the normalisation table with bf16 internals."""
    if not u8:
        return "f32in"
    return "u8table" if variant.split("+")[0] == "bf16" else "u8exact"


def _vi(variants):
    return [pytest.param(v, u8, id=f"{v}-{_input_id(v, u8)}") for v in variants for u8 in (True, False)]


FUSED_VARIANTS = ["bf16", "f16", "f16_bf16", "bf16+raw_s2", "f16+raw_s2", "f16_bf16+raw_s2"]


def _check_fused(variant, u8, content, size):
    B, H, W = size
    D = _Dev(SC.params_of(content))
    src = _src(content, B, H, W, u8)
    tag = f"{_input_id(variant, u8)} {content} {_sz(size)}"
    if variant.endswith("+raw_s2"):
        # bound 6: out_raw holds the even pixels of the full tensor, out_act is the unflagged launch's, bit for bit
        base = variant[:-7]
        raw, act = _fused(D, base, u8, src, B, H, W)
        raw2, act2 = _fused(D, base, u8, src, B, H, W, raw_s2=True)
        assert tuple(raw2.shape) == SC.raw_s2_shape(B, H, W)
        assert _same(raw2, raw[:, ::2, ::2].contiguous()) and _same(act2, act)
        raw3, _ = _fused(D, base, u8, src, B, H, W, act=False, raw_s2=True)
        assert _same(raw3, raw2)
        print(f"STEM_EDGE stem012 {variant} {tag}: raw == full[:, ::2, ::2], act == unflagged, bit for bit")
        return
    raw, act = _fused(D, variant, u8, src, B, H, W)
    raw_only, _ = _fused(D, variant, u8, src, B, H, W, act=False)
    _, act_only = _fused(D, variant, u8, src, B, H, W, raw=False)
    assert _same(raw, raw_only) and _same(act, act_only)                   # each output alone: the same values
    ref = SC.fused_case_ref(content, B, H, W, variant, u8)
    ratios = {"raw": SC.ratio(raw.cpu(), ref.raw), "act": SC.ratio(act.cpu(), ref.act)}
    extra = ""
    if variant == "bf16":
        # bound 3: the bf16 chain, bit for bit, through both entry points
        praw, pact = _fused(D, variant, u8, src, B, H, W, plain_entry=True)
        _, _, craw, cact = _chain(D, "bf16", u8, src, B, H, W)
        assert _same(praw, raw) and _same(pact, act)
        assert _same(raw, craw), int((_bits(raw) != _bits(craw)).sum())
        assert _same(act, cact), int((_bits(act) != _bits(cact)).sum())
        extra = ", == ppn_stem012 == the bf16 chain bit for bit"
    if variant == "f16_bf16":
        # bound 5: the same f32 values stored as bf16 and as half
        hraw, hact = _fused(D, "f16", u8, src, B, H, W)
        small = max(float(hraw.float().max()), float(hact.float().max())) < 60000.0
        assert small or content == "sat"
        if small:
            assert SC.bf16_interval_ok(raw.cpu(), hraw.cpu()) and SC.bf16_interval_ok(act.cpu(), hact.cpu())
            extra = ", within the bf16 roundings of the f16 outputs +- 1/2 ulp"
    if content == "sat":
        assert torch.isfinite(raw.float()).all() and torch.isfinite(act.float()).all()
        extra += f", {ref.overflow0} layer-0 values past 65504"
    _report("stem012", variant, tag, ratios, extra)


def _check_x3(u8, size):
    B, H, W = size
    D = _Dev(SC.params("draw"))
    src = _src("random", B, H, W, u8)
    raw, act = _fused(D, "x3", u8, src, B, H, W)
    raw_only, _ = _fused(D, "x3", u8, src, B, H, W, act=False)
    _, act_only = _fused(D, "x3", u8, src, B, H, W, raw=False)
    assert _same(raw, raw_only) and _same(act, act_only)
    rr, ra = SC.plain_ref(D.P, SC.normalise(SC.frames("random", B, H, W)))
    ratios = {}
    for k, got, ref in (("raw", raw, rr), ("act", act, ra)):
        ratios[k] = float((got.cpu().double() - ref).abs().max()) / max(1.0, float(ref.abs().max())) / STEM_X3_TOL
    _report("stem012_x3", "x3", f"{'u8exact' if u8 else 'f32in'} random {_sz(size)} (x STEM_X3_TOL)", ratios)


@pytest.mark.parametrize("size", SC.TINY, ids=_sz)
@pytest.mark.parametrize("variant,u8", _vi(FUSED_VARIANTS + ["x3"]))
def test_fused_stem_tiny(variant, u8, size):
    """Images smaller than the 7x7 filter, the 10-row patch and the 5- / 6-row rings, in a function of their own.

    Index arithmetic of stem012.hip / stem012_x3.hip for H or W below 7 (one unit: strip 0, band 0, xib = -5, xs = 0):
      request_input  only rows 0 <= gy < H are requested; a row's dwords k satisfy A + 4k < S + nb_row with
                     nb_row = 3 min(115, W) and A = S & ~3, so the last dword read is the aligned dword that holds the row's
                     last byte: at most 3 bytes past the tensor's end, inside the same aligned dword (never another page),
                     and at most 3 bytes before a row's first byte, which for b = gy = 0 is the tensor's first byte (A = S = 0).
                     LDS side: lane k lands at raw_p + r * 368 + 4k with k < 92: inside the row's 368 bytes, r < 10.
      convert_input  reads the raw rows UNCONDITIONALLY at prow * 368 + 2k * 368 + 3 (gx - xs) + phase + {0, 1, 2} <= 9 * 368 +
                     3 * 119 + 3 + 2 < 10 * 368 (stale LDS, never global memory) and masks with colok && 0 <= gy < H; the
                     f32 source is only dereferenced under that mask.  Patch writes: py < nrows <= 10, px < 120.
      ring warm-up   layer0(2 R2 - 2, 3) and layer1(2 R2 - 1, 1) write ring slots (gy + 2 R) % R >= 0 for gy >= -2 and store
                     zeros outside the image (rowok && 0 <= gx < W); the chunk loop runs once (R2e = Ho <= 4), rows past H are
                     zero rows, and layer2 stores only oy < Ho && ox < Wo, for RAW_S2 at ((oy >> 1), (ox >> 1)) of the
                     [(Ho + 1) / 2, (Wo + 1) / 2] tensor.
    No tiny size reads or writes out of bounds, so none is rejected."""
    if variant == "x3":
        _check_x3(u8, size)
    else:
        _check_fused(variant, u8, "random", size)


@pytest.mark.parametrize("size", SC.FUSED_SIZES, ids=_sz)
@pytest.mark.parametrize("variant,u8", _vi(FUSED_VARIANTS + ["x3"]))
def test_fused_stem_sizes(variant, u8, size):
    """Bands of 15 / 16 / 17 / 18 layer-2 rows at odd widths (u8 row phases 1 and 3), strips of exactly 48 columns and
    one-column second / third strips, five 5x7 frames (frame bases on all four byte phases) and 130 frames of 33x97 = 520
    units, past the grid cap of 512 (stem012) and 256 (stem012_x3): a work-group's second unit reuses patch and rings."""
    if size in SC.CAP:
        assert SC.fused_units(*size) > max(SC.FUSED_GRID_CAP.values())
    if variant == "x3":
        _check_x3(u8, size)
    else:
        _check_fused(variant, u8, "random", size)


@pytest.mark.parametrize("size", SC.CONTENT_SIZES, ids=_sz)
@pytest.mark.parametrize("content", SC.CONTENT_KINDS)
@pytest.mark.parametrize("variant,u8", _vi(["bf16", "f16", "f16_bf16"]))
def test_fused_stem_content(variant, u8, content, size):
    """All 256 u8 values (ambiguous table entries widen the bound by one storage ulp per tap), constant frames of 0 / 128 /
    255 (the padding is zero in NORMALISED space; u8 0 normalises to about -2), impulses at the corners and on both sides of
    the strip and band seams through pass-through layers 1 and 2 (the response is the flipped 7x7 filter), negative BN scales
    with half the outputs at the ReLU kink, and scale0 ~ 3e6: the half rings saturate at 65504 and everything stays finite."""
    _check_fused(variant, u8, content, size)


def test_zz_worst_ratios():
    """Prints this run's worst err / bound per kernel, variant and output (nothing to assert: every test asserted its own)."""
    for (kernel, variant, out), v in sorted(WORST.items()):
        print(f"STEM_EDGE WORST {kernel} {variant} {out}: {v:.3f}")
