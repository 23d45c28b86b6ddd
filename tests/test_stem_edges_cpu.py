"""CPU checks of tests/stem_cases.py: the f64 references are the convolutions they claim to be, an independent float32
emulation of a correct kernel stays inside every bound on every case the GPU test runs, emulated defects (wrong padding,
swapped channels, a shifted strip, a stale ring row, a missing clamp) do not, and the case lists reach the edges they are
for (grid caps, strip / band seams, byte phases, the ambiguous table entries, the half overflow)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stem_cases as SC


def _direct_conv(a, w, stride, pad):
    """Convolution written out with unfold + matmul (no conv2d)."""
    B, C, H, W = a.shape
    co, _, k, _ = w.shape
    cols = F.unfold(a, k, padding=pad, stride=stride)                      # [B, C k k, L]
    ho, wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return (w.reshape(co, -1) @ cols).view(B, co, ho, wo)


CPU_SIZES = SC.TINY + SC.BANDS[::3] + SC.STRIPS[1::2] + SC.PHASE + [(3, 33, 97)]      # CAP's frame size, three frames of it


@pytest.mark.parametrize("size", CPU_SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("content", ["random", "neg"])
def test_layer_reference_is_the_convolution(content, size):
    """On a case's own operands (the quantised patch and the two emulated intermediate tensors of the bf16 stem), each layer
    of the reference is the f64 convolution + affine + ReLU.  layer_ref calls F.conv2d, so the torch.equal against F.conv2d
    only pins that it stays that; the independent check is the convolution written out with unfold + matmul, which shares
    no code with conv2d's direct path.  Run on these sizes and two parameter sets, not on every case of the GPU test."""
    B, H, W = size
    P = SC.params_of(content)
    xn = SC.normalise(SC.frames(content, B, H, W))
    res = SC.fused_ref(P, xn=xn, internal="bf16", out="bf16")
    w = [SC.rnd(t.double(), "bf16") for t in P.w]
    for a, L, stride, pad in ((SC.rnd(xn.double(), "bf16"), 0, 1, 3), (res.a0, 1, 1, 1), (res.a1, 2, 2, 1)):
        p, d = SC.layer_ref(a, w[L], P.s[L], P.b[L], stride, pad, K=w[L][0].numel())
        assert torch.equal(p, F.relu(F.conv2d(a, w[L], None, stride, pad) * SC._v(P.s[L]) + SC._v(P.b[L])))
        exp = F.relu(_direct_conv(a, w[L], stride, pad) * SC._v(P.s[L]) + SC._v(P.b[L]))
        assert float((p - exp).abs().max()) <= 1e-12 * max(1.0, float(exp.abs().max()))
        assert (d > 0).all()
    assert torch.equal(SC.nhwc(p), res.raw[0])                             # ... and the chain of them is fused_ref's output


def test_exact_input_form_is_the_normalised_convolution():
    """conv(w / std, x - 128) + conv(w4, inside) == conv(w, (x - mean) / std) with zero padding in NORMALISED space, to the
    rounding of half(w / std): the inside channel carries the padding."""
    P = SC.params("draw")
    fr = SC.frames("random", 2, 9, 11)
    _, _, w4f = SC.exact_in_weights(P.w[0])
    x = torch.from_numpy(fr.transpose(0, 3, 1, 2).copy()).double() - 128.0
    patch = torch.cat([x, torch.ones_like(x[:, :1])], 1)
    got = F.conv2d(patch, w4f.double(), None, 1, 3)
    ref = F.conv2d(SC.normalise(fr).double(), P.w[0].double(), None, 1, 3)
    assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


def test_ulp_and_rounding():
    x = torch.tensor([1.0, 1.5, 2.0, 3.999, 0.0, 65504.0, 1e-30], dtype=torch.float64)
    assert SC.ulp(x, "f16").tolist()[:6] == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -9, 2.0 ** -24, 32.0]
    assert SC.ulp(x, "bf16").tolist()[:4] == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6]
    assert SC.ulp(x, "f32").tolist()[:3] == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22]
    assert SC.rnd(torch.tensor([1e6], dtype=torch.float64), "f16").item() == 65504.0
    assert torch.isinf(SC.rnd(torch.tensor([1e6], dtype=torch.float64), "f16", clamp=False)).all()
    # rnd goes f64 -> f32 -> T like the kernels (f32 value, then the store): on f32-representable values that is ONE rounding,
    # within half an ulp of T.  (An f64 value within half an f32 ulp of a midpoint of T may end 1/2 ulp_T + 1/2 ulp_f32 away.)
    g = torch.Generator().manual_seed(5)
    for T in ("f16", "bf16"):
        v = (torch.rand(4000, generator=g) * 100).double()
        assert ((SC.rnd(v, T) - v).abs() <= 0.5 * SC.ulp(v, T)).all()
        v = torch.rand(4000, generator=g, dtype=torch.float64) * 100
        assert ((SC.rnd(v, T) - v).abs() <= 0.5 * SC.ulp(v, T) + 0.5 * SC.ulp(v, "f32")).all()


def test_ambiguous_table_entries():
    assert SC.ambiguous_entries("bf16") == ((1, 20), (1, 55), (1, 97), (1, 181))
    assert SC.ambiguous_entries("f16") == ((1, 118), (1, 132), (1, 146), (1, 160), (1, 174), (1, 188), (1, 202), (1, 216),
                                           (1, 251))
    vals = SC.unambiguous_values()
    assert len(vals) == 256 - 13 and {0, 128, 255} <= set(vals.tolist())
    for kind in ("random", "neg", "sat", "ident", "const0", "const128", "const255", "impulse"):
        fr = SC.frames(kind, 2, 9, 98)
        assert not SC.ambiguity_mask(fr, "bf16").any() and not SC.ambiguity_mask(fr, "f16").any()
    fr = SC.frames("all256", 1, 33, 97)
    assert SC.ambiguity_mask(fr, "bf16").any() and SC.ambiguity_mask(fr, "f16").any()
    assert len(np.unique(fr)) == 256


def test_exact_input_weights_and_their_ambiguous_entries():
    """half(w / std) and the inside-channel weight (a three-term f32 sum, contracted into FMAs or not): the f64 value rounds
    to the emulation's half or, where the entry is flagged ambiguous, to a neighbour of it; few entries are flagged."""
    for kind in ("draw", "neg", "sat"):
        w0 = SC.params(kind).w[0]
        q, e_w, _ = SC.exact_in_weights(w0)
        m, s = torch.tensor(SC.MEAN).float().double(), torch.tensor(SC.STD).float().double()
        w4 = (w0.double() * ((128.0 - m) / s).view(1, 3, 1, 1)).sum(1, keepdim=True)
        v64 = torch.cat([w0.double() / s.view(1, 3, 1, 1), w4], 1)
        assert ((SC.rnd(v64, "f16") - q).abs() <= e_w).all()
        assert 0 < int((e_w > 0).sum()) < 0.02 * e_w.numel()


def test_sizes_reach_the_edges():
    ho = sorted({SC.out_hw(h, w)[0] for _, h, w in SC.BANDS})
    assert ho == [15, 16, 17, 18]
    assert sorted({SC.out_hw(h, w)[1] for _, h, w in SC.STRIPS}) == [48, 49, 96, 97]
    # u8 row phases: (row index * W * 3) mod 4 takes all four values in the odd-width band cases and over the PHASE frames
    for _, h, w in SC.BANDS:
        assert {(y * w * 3) % 4 for y in range(h)} == {0, 1, 2, 3}
    (b, h, w), = SC.PHASE
    assert {(i * h * w * 3) % 4 for i in range(b)} == {0, 1, 2, 3}
    (b, h, w), = SC.CAP
    assert SC.fused_units(b, h, w) == 520 > max(SC.FUSED_GRID_CAP.values()) and b * h * w * 3 < 2e6
    assert SC.tiles(*SC.STEM7_CAP, SC.STEM7_TILE) > SC.STEM7_GRID_CAP
    for T in ("f32", "bf16"):
        for stride in (1, 2):
            g = SC.stem3_geo(T, stride)
            b, h, w = SC.stem3_cap_size(T, stride)
            assert SC.tiles(b, *SC.out_hw(h, w, stride), (g.th, g.tw)) == 4 * b > g.cap
            outs = [SC.out_hw(h, w, stride) for _, h, w in SC.stem3_sizes(T, stride)[:5]]
            assert sorted({o[0] for o in outs}) == [g.th - 1, g.th, g.th + 1]
            assert sorted({o[1] for o in outs}) == [g.tw - 1, g.tw, g.tw + 1]
    assert [SC.stem3_geo(T, s).cap for T in ("bf16", "f32") for s in (1, 2)] == [1024, 512, 768, 512]
    assert SC.raw_s2_shape(1, 29, 41) == (1, 8, 11, 32) and SC.raw_s2_shape(1, 31, 43) == (1, 8, 11, 32)
    assert SC.raw_s2_shape(1, 33, 97) == (1, 9, 25, 32) and SC.raw_s2_shape(1, 1, 1) == (1, 1, 1, 32)
    assert {SC.out_hw(h, w)[0] % 2 for _, h, w in SC.FUSED_SIZES} == {0, 1}
    assert {SC.out_hw(h, w)[1] % 2 for _, h, w in SC.FUSED_SIZES} == {0, 1}


def _emu_ratios(run, mutant=None):
    variant, u8, content, (B, H, W) = run
    internal, out = SC.VARIANTS[variant]
    ref = SC.fused_case_ref(content, B, H, W, variant, u8)
    fr, P = SC.frames(content, B, H, W), SC.params_of(content)
    kw = dict(fr=fr, exact_in=SC.is_exact_in(variant, True)) if u8 else dict(xn=SC.normalise(fr))
    raw, act = SC.fused_emu32(P, internal=internal, out=out, mutant=mutant, **kw)
    return SC.ratio(raw, ref.raw), SC.ratio(act, ref.act)


@pytest.mark.parametrize("run", SC.fused_runs(CPU_SIZES) + SC.fused_runs(SC.CONTENT_SIZES, SC.CONTENT_KINDS), ids=SC.run_id)
def test_f32_emulation_stays_inside_the_fused_bound(run):
    r = _emu_ratios(run)
    assert max(r) <= 1.0, r


def test_saturation_case_overflows():
    for B, H, W in SC.CONTENT_SIZES:
        for u8 in (True, False):
            ref = SC.fused_case_ref("sat", B, H, W, "f16", u8)
            assert ref.overflow0 > 0.05 * ref.a0.numel(), (B, H, W, u8, ref.overflow0)
            assert float(ref.a0.max()) == SC.F16_MAX
            assert float(ref.raw[0].max()) == SC.F16_MAX == float(ref.act[0].max())     # the outputs saturate too
            # ... and a clamped value's bound is a fraction of it: an output of 0 or inf in its place is far outside
            sat = ref.raw[0] == SC.F16_MAX
            assert float(ref.raw[1][sat].max()) < 0.25 * SC.F16_MAX
    for kind in ("random", "all256", "const255", "impulse", "neg"):
        ref = SC.fused_case_ref(kind, 1, 33, 97, "f16", True)
        assert ref.overflow0 == 0 and max(float(ref.raw[0].max()), float(ref.act[0].max())) < 60000.0


# what test_stem_edges_gpu.py runs on the fused stems: random frames on the size lists, every other content on CONTENT_SIZES
GPU_FUSED_RUNS = set(SC.fused_runs(SC.TINY + SC.FUSED_SIZES) + SC.fused_runs(SC.CONTENT_SIZES, SC.CONTENT_KINDS))
MUTANT_RUNS = SC.fused_runs(SC.CONTENT_SIZES[:2], ("all256", "neg", "ident", "sat", "impulse"), ("f16",)) + \
    SC.fused_runs([(1, 33, 43), (1, 9, 97)], variants=("f16",))


@pytest.mark.parametrize("mutant", SC.MUTANTS)
def test_fused_bound_notices_the_defect(mutant):
    """Each defect leaves the bound on at least one (variant, input, content, size) the GPU test runs."""
    assert set(MUTANT_RUNS) <= GPU_FUSED_RUNS
    worst = {SC.run_id(r): max(_emu_ratios(r, mutant)) for r in MUTANT_RUNS}
    caught = {k: v for k, v in worst.items() if v > 1.0}
    print(f"{mutant}: caught by {len(caught)}/{len(worst)} runs, worst {max(worst.values()):.3g}")
    assert caught, worst


@pytest.mark.parametrize("T", ["f32", "bf16"])
def test_f32_emulation_stays_inside_the_single_layer_bound(T):
    dt = SC.TYPES[T][0]
    P = SC.params("draw")
    for B, H, W in SC.STEM7_SIZES[:3] + SC.STEM7_SIZES[5:]:
        xn = SC.normalise(SC.frames("random", B, H, W))
        for s, b, relu in ((P.s[0], P.b[0], True), (None, None, False)):
            ref = SC.single_ref(xn, P.w[0], s, b, 1, 3, T, relu=relu)
            t = F.conv2d(xn.to(dt).float(), P.w[0].to(dt).float(), None, 1, 3)
            if s is not None:
                t = (t * s.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)).clamp_min(0.0)
            assert SC.ratio(SC.nhwc(t.to(dt).float()), ref["raw"]) <= 1.0
            # padding with the u8 value 0 instead of the normalised 0 leaves the bound wherever there is a border
            zero = SC.normalise(np.zeros((1, 1, 1, 3), np.uint8)).view(3).to(dt).float()
            bad = SC._conv32(xn.to(dt).float(), P.w[0].to(dt).float(), P.s[0], P.b[0], 1, 3, zero)
            if s is not None:
                assert SC.ratio(SC.nhwc(bad.to(dt).float()), ref["raw"]) > 1.0
    # the content cases of the layer kernels: constant frames and impulses
    for content in SC.STEM7_CONTENTS:
        for B, H, W in SC.STEM7_CONTENT_SIZES:
            xn = SC.normalise(SC.frames(content, B, H, W))
            ref = SC.single_ref(xn, P.w[0], P.s[0], P.b[0], 1, 3, T)
            t = SC._conv32(xn.to(dt).float(), P.w[0].to(dt).float(), P.s[0], P.b[0], 1, 3)
            assert SC.ratio(SC.nhwc(t.to(dt).float()), ref["raw"]) <= 1.0
    B, H, W = SC.STEM7_CONTENT_SIZES[0]
    assert (SC.frames("impulse", B, H, W) == 255).sum() == 6                # four corners, both sides of the tile seam
    for stride in (1, 2):
        runs = [("random", s) for s in SC.stem3_sizes(T, stride)[:2] + SC.stem3_sizes(T, stride)[5:]] + \
            [(c, s) for c in SC.STEM3_CONTENTS for s in SC.stem3_content_sizes(T, stride)]
        B, H, W = SC.stem3_content_sizes(T, stride)[0]
        assert int(SC.activations(T, B, H, W, content="impulse", seam=SC.stem3_seam(T, stride)).sum()) == 8
        for content, (B, H, W) in runs:
            x = SC.nchw(SC.activations(T, B, H, W, content=content, seam=SC.stem3_seam(T, stride)))
            w = P.w[stride]
            ref = SC.single_ref(x, w, P.s[stride], P.b[stride], stride, 1, T, s2=P.s[3][:w.shape[0]], b2=P.b[3][:w.shape[0]])
            v = SC._conv32(x, w.to(dt).float(), P.s[stride], P.b[stride], stride, 1)
            u = (v * P.s[3][:w.shape[0]].view(1, -1, 1, 1) + P.b[3][:w.shape[0]].view(1, -1, 1, 1)).clamp_min(0.0)
            assert SC.ratio(SC.nhwc(v.to(dt).float()), ref["raw"]) <= 1.0
            assert SC.ratio(SC.nhwc(u.to(dt).float()), ref["act"]) <= 1.0


def test_bf16_interval_rule():
    v = torch.rand(20000) * 100.0
    f16, bf = v.to(torch.float16), v.to(torch.bfloat16)
    assert SC.bf16_interval_ok(bf, f16)
    assert not SC.bf16_interval_ok((v * 1.02).to(torch.bfloat16), f16)
