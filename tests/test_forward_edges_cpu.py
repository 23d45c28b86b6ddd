"""CPU: the forward-convolution edge cases (tests/forward_cases.py) are what they claim.  No GPU.

* the f64 reference equals an explicit loop over the filter taps, and the all-padding pixels of `overpad` equal act1(b1);
* the derived per-element bound holds (ratio <= 1) for a torch emulation of the kernels' arithmetic -- f32 convolution, f32
  epilogue in the stated order, ONE rounding to the storage type -- on every (case, dtype, epilogue);
* the bound SEES the faults a convolution kernel can have: each fault below is planted in the emulation on the named case
  (K <= 4608) and must give ratio > 1 in every dtype; and a lost input element passes the old 2e-2 * max rule on the forced-tile
  shape of test_conv_tiles_gpu.py, which is why the per-element bound exists;
* every (case, dtype) reaches the kernel, tile and tile counts it is recorded for: its descriptor goes through
  csrc/conv_route.cpp (tools/conv_route_check.cpp, built as tests/test_conv_route_cpu.py builds it)."""
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import forward_cases as FC
from conv_route_cases import load as load_fixture
from test_conv_route_cpu import CSRC, ROOT, SEG

DT = FC.DTYPE_NAMES


def emulate(c, op, epi, dtype, acc=None, s1b1=None, res_mask=None):
    """What a correct kernel may return: f32 accumulation (torch's order), f32 epilogue, one rounding to the storage type.
    acc / s1b1 / res_mask: where the planted faults go in."""
    if acc is None:
        acc = F.conv2d(op["x"], op["w"], None, c.s, c.pad, c.dil)
    o = dict(op)
    if s1b1 is not None:
        o["s1"], o["b1"] = s1b1
    if res_mask is not None:
        o["res"] = op["res"] * res_mask
    v, u = FC.epilogue(acc.float(), o, epi)
    out = {}
    if epi.raw:
        out["raw"] = FC.q(v, dtype)
    if epi.act:
        out["act"] = FC.q(u, dtype)
    return out


def worst_ratio(got, ref, bound):
    return max(FC.ratio(got[k], ref[k], bound[k]) for k in ref)


# ---- reference ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FC.ALL))
def test_reference_equals_the_loop_over_taps(name):
    c = FC.ALL[name][0]
    for dtype in DT:
        op = FC.operands(name, dtype)
        acc, S = FC.conv_f64(c, op)
        taps = FC.conv_by_taps(c, op["x"], op["w"])
        assert taps.shape == acc.shape == (c.B, c.co) + FC.out_hw(c)
        assert float((acc - taps).abs().max()) <= 1e-12 * max(1.0, float(taps.abs().max()))
        mag = FC.conv_by_taps(c, op["x"].abs(), op["w"].abs())
        assert float((S - mag).abs().max()) <= 1e-12 * max(1.0, float(mag.abs().max()))
        # the epilogue, restated per element in Python floats (f64) on a few elements
        ref, _ = FC.reference(name, dtype, "res_lrelu2")
        lrelu = lambda t: t if t > 0 else 0.1 * t                                                       # noqa: E731
        for (b, o, y, x) in ((0, 0, 0, 0), (c.B - 1, c.co - 1, acc.shape[2] - 1, acc.shape[3] - 1)):
            v = float(taps[b, o, y, x]) + float(op["res"][b, o, y, x])
            assert abs(float(ref["raw"][b, o, y, x]) - v) <= 1e-12 * max(1.0, abs(v))
            u = lrelu(v * float(op["s2"][o]) + float(op["b2"][o]))
            assert abs(float(ref["act"][b, o, y, x]) - u) <= 1e-12 * max(1.0, abs(u))


def test_overpad_pixels_without_a_tap_equal_act1_of_b1():
    c = FC.ALL["overpad"][0]
    ring = FC.no_tap_inside(c)
    Ho, Wo = FC.out_hw(c)
    assert ring.shape == (Ho, Wo) and ring[0].all() and ring[-1].all() and ring[:, 0].all() and ring[:, -1].all()
    assert not ring[1:-1, 1:-1].any() and c.pad > c.dil * (c.k - 1)
    for dtype in DT:
        op = FC.operands("overpad", dtype)
        ref, _ = FC.reference("overpad", dtype, "bn_relu")
        want = F.relu(op["b1"].double()).view(1, -1, 1, 1).expand_as(ref["raw"])
        assert torch.equal(ref["raw"][:, :, ring], want[:, :, ring])
        assert not torch.equal(ref["raw"][:, :, ~ring], want[:, :, ~ring])
    # every other case has at least one tap inside every output pixel
    assert [n for n, (cc, _, _) in FC.ALL.items() if FC.no_tap_inside(cc).any()] == ["overpad"]


def test_cases_are_the_edges_they_claim():
    C = {n: v[0] for n, v in FC.ALL.items()}
    for n in ("reach_gt_image", "reach_gt_image_wide", "reach_gt_image_wide/256"):      # off-centre filter rows wholly in padding
        c = C[n]
        assert c.dil >= c.H and c.pad == c.dil and FC.out_hw(c) == (c.H, c.W)
    assert FC.out_hw(C["ho1"])[0] == 1 and FC.out_hw(C["wo1"])[1] == 1 and FC.out_hw(C["one_pixel"]) == (1, 1)
    for n in ("s2_odd/3x3", "s2_odd/1x1"):
        c = C[n]
        odd = [(d + 2 * c.pad - c.k) % 2 for d in (c.H, c.W)]
        assert c.s == 2 and sorted(odd) == [0, 1]
    c = C["valid"]
    assert c.pad == 0 and c.k == 3 and FC.out_hw(c)[0] < c.H
    c = C["many_images"]
    assert c.H < 8 and c.W < 16 and 128 // (c.H * c.W) >= 21
    assert FC.pixels(C["exact_tiles"]) == 256
    assert {C[n].co for n in ("cout8", "cin16_5x5", "cout40", "cout72")} == {8, 24, 40, 72}
    assert C["cin8"].ci == 8 and C["cin16_5x5"].k == 5 and C["c64_5x5"].k == 5
    assert all(FC.depth(c) <= 4608 for c in C.values())
    assert len(FC.EPILOGUES) == 8 and len(set(FC.EPILOGUES.values())) == 8


# ---- the bound holds for correct arithmetic -------------------------------------------------------------------------------------

def test_bound_holds_for_the_f32_emulation():
    worst = {d: (0.0, None) for d in DT}
    for name, dtype, en in FC.runs():
        c, epi = FC.ALL[name][0], FC.EPILOGUES[en]
        ref, bound = FC.reference(name, dtype, en)
        r = worst_ratio(emulate(c, FC.operands(name, dtype), epi, dtype), ref, bound)
        assert r <= 1.0, (name, dtype, en, r)
        if r > worst[dtype][0]:
            worst[dtype] = (r, (name, en))
    for d in DT:
        print("FWD_EDGE_CPU emulation worst ratio %s: %.3f at %s" % (d, worst[d][0], worst[d][1]))
    # the roundings to the storage type are what fills the bound in the 16-bit types
    assert worst["bf16"][0] > 0.4 and worst["f16"][0] > 0.4


# ---- the bound sees planted faults ------------------------------------------------------------------------------------------------

def _typical_element(x, b, y, xx):
    """The channel at (b, y, xx) whose magnitude is closest to the median magnitude of the tensor: a typical element, neither
    a large nor a near-zero one."""
    return int((x[b, :, y, xx].abs() - x.abs().median()).abs().argmin())


def _lose_one_input_element(c, op):
    x = op["x"].clone()
    b, y, xx = c.B - 1, c.H // 2, c.W // 2
    x[b, _typical_element(x, b, y, xx), y, xx] = 0.0
    return dict(acc=F.conv2d(x, op["w"], None, c.s, c.pad, c.dil))


def _drop_one_tap_at_a_border_pixel(c, op):
    """Output pixel (0, 0) of the last image without its last tap (which lies inside the image)."""
    acc = F.conv2d(op["x"], op["w"], None, c.s, c.pad, c.dil)
    iy = ix = -c.pad + (c.k - 1) * c.dil
    assert 0 <= iy < c.H and 0 <= ix < c.W and c.pad > 0
    acc[-1, :, 0, 0] -= op["w"][:, :, -1, -1] @ op["x"][-1, :, iy, ix]
    return dict(acc=acc)


def _padding_reads_the_neighbouring_row(c, op):
    """Column -1 of a row is the last column of the row above in memory, column W the first of the row below."""
    p = c.pad
    xp = F.pad(op["x"], (p, p, p, p))
    for j in range(p):
        xp[:, :, p + 1: p + c.H, p - 1 - j] = op["x"][:, :, : c.H - 1, c.W - 1 - j]
        xp[:, :, p: p + c.H - 1, p + c.W + j] = op["x"][:, :, 1:, j]
    return dict(acc=F.conv2d(xp, op["w"], None, c.s, 0, c.dil))


def _seam_pixel_reads_the_previous_image(c, op):
    """One pixel of the top row of image 1 takes its upper filter row from the last row of image 0."""
    acc = F.conv2d(op["x"], op["w"], None, c.s, c.pad, c.dil)
    assert c.pad == 1 and c.k == 3 and c.dil == 1 and c.s == 1 and c.B > 1
    ox = c.W // 2
    for v in range(3):
        ix = ox - 1 + v
        if 0 <= ix < c.W:
            acc[1, :, 0, ox] += op["w"][:, :, 0, v] @ op["x"][0, :, c.H - 1, ix]
    return dict(acc=acc)


def _scale_shift_from_the_next_channel(c, op, tile=64):
    """The last channel tile reads scale1 / shift1 one channel too far (its last channel: the tile's first)."""
    lo = (c.co - 1) // tile * tile
    s1, b1 = op["s1"].clone(), op["b1"].clone()
    s1[lo:], b1[lo:] = torch.roll(op["s1"][lo:], -1), torch.roll(op["b1"][lo:], -1)
    return dict(s1b1=(s1, b1))


def _residual_skipped_one_in_1000(c, op):
    keep = (torch.rand(op["res"].shape, generator=torch.Generator().manual_seed(7)) >= 1e-3).float()
    assert 0 < int((keep == 0).sum()) <= 2e-3 * keep.numel()
    return dict(res_mask=keep)


def _k_padding_times_nonzero_weights(c, op, kstep=64):
    """The GEMM depth is padded to the K step: the padding columns read the centre pixel's channels again instead of zeros,
    against weight columns that are not zero."""
    acc = F.conv2d(op["x"], op["w"], None, c.s, c.pad, c.dil)
    npad = -FC.depth(c) % kstep
    assert npad > 0 and c.s == 1 and FC.out_hw(c) == (c.H, c.W)
    g = torch.Generator().manual_seed(11)
    wg = torch.randn(c.co, npad, generator=g) * (2.0 / FC.depth(c)) ** 0.5
    xg = op["x"][:, torch.arange(npad) % c.ci]                                   # [B, npad, H, W]
    return dict(acc=acc + torch.einsum("on,bnhw->bohw", wg, xg))


# fault -> (the case that catches it, the epilogue it is planted under, how)
FAULTS = {
    "one input element lost": ("reach_gt_image", "bn_relu", _lose_one_input_element),
    "one tap dropped at one border pixel": ("exact_tiles", "bn_relu", _drop_one_tap_at_a_border_pixel),
    "padding read as the neighbouring row": ("exact_tiles", "bn_relu", _padding_reads_the_neighbouring_row),
    "seam pixel takes its upper row from the previous image": ("many_images", "bn_relu", _seam_pixel_reads_the_previous_image),
    "scale/shift from channel c+1 in the last channel tile": ("cout72", "bn_relu", _scale_shift_from_the_next_channel),
    "residual add skipped at 1 element in 1000": ("sweep/big", "res_raw", _residual_skipped_one_in_1000),
    "K padding columns multiplied by nonzero weights": ("cin8", "bn_relu", _k_padding_times_nonzero_weights),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_bound_sees_the_planted_fault(fault):
    name, en, plant = FAULTS[fault]
    c, epi = FC.ALL[name][0], FC.EPILOGUES[en]
    assert FC.depth(c) <= 4608
    for dtype in DT:
        op = FC.operands(name, dtype)
        ref, bound = FC.reference(name, dtype, en)
        clean = worst_ratio(emulate(c, op, epi, dtype), ref, bound)
        r = worst_ratio(emulate(c, op, epi, dtype, **plant(c, op)), ref, bound)
        print("FWD_EDGE_CPU fault '%s' on %s %s: ratio %.1f (clean %.2f)" % (fault, name, dtype, r, clean))
        assert clean <= 1.0 < r, (fault, name, dtype, clean, r)


@pytest.mark.parametrize("dtype,tol,old_rule_misses", [("bf16", 2e-2, True), ("f16", 3e-3, False)])
def test_lost_input_element_passes_the_old_max_rule_on_the_forced_tile_shape(dtype, tol, old_rule_misses):
    """2 x 128 x 20 x 23 -> 200, 3x3 dilation 2 (test_conv_tiles_gpu.py::test_forced_tile_single_output): one wrong load of a
    typical element feeding nine taps stays under bf16's 2e-2 * max(1, max |ref|), and the per-element bound catches it.  (The
    f16 rule, 3e-3 * max, does see a lost element of this size on this shape; smaller faults pass it alike.)"""
    c, epi = FC.FORCED_TILE_SHAPE, FC.EPILOGUES["bn_relu"]
    op = FC.make_operands(c, dtype, 31)
    ref, bound = FC.reference_of(c, op, epi, dtype)
    clean = emulate(c, op, epi, dtype)
    bad = emulate(c, op, epi, dtype, **_lose_one_input_element(c, op))
    old = tol * max(1.0, float(ref["raw"].abs().max()))
    err_clean, err_bad = (float((g["raw"].double() - ref["raw"]).abs().max()) for g in (clean, bad))
    r_clean, r_bad = worst_ratio(clean, ref, bound), worst_ratio(bad, ref, bound)
    print("FWD_EDGE_CPU forced-tile shape %s: old tolerance %.3f, clean err %.4f (ratio %.2f), one element lost err %.4f (ratio %.1f)"
          % (dtype, old, err_clean, r_clean, err_bad, r_bad))
    assert err_clean <= old and r_clean <= 1.0
    assert err_bad > 2 * err_clean and (err_bad <= old) == old_rule_misses
    assert r_bad > 1.0


# ---- purposes: what csrc/conv_route.cpp says about every (case, dtype) ----------------------------------------------------------

def _entries():
    """[(case, dtype, purpose, conv64 knob)]: every (case, dtype), then the conv64-off forms."""
    out = [(n, d, why[d], 1) for n, (_, _, why) in FC.ALL.items() for d in DT]
    return out + [(n, d, p, 0) for n, p in FC.CONV64_OFF.items() for d in ("bf16", "f16")]


@pytest.fixture(scope="module")
def routed(tmp_path_factory):
    from pytorch_pose_proposal_network_amd import lib as L
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("route") / "conv_route_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "conv_route_check.cpp"), os.path.join(CSRC, "conv_route.cpp"), "-o", exe],
                   check=True)
    fields, _ = load_fixture()
    assert len(fields) == 53
    code = {"f32": L.PPN_F32, "bf16": L.PPN_BF16, "f16": L.PPN_F16}
    lines, ktots = [], []
    for name, dtype, _, conv64 in _entries():
        c, force, _ = FC.ALL[name]
        Ho, Wo = FC.out_hw(c)
        _, _, _, ktot, cpad = L.conv_tiling(code[dtype], c.ci, c.co, c.k)
        v = dict.fromkeys(fields, 0)
        v.update(dtype=code[dtype], batch=c.B, in_h=c.H, in_w=c.W, cin=c.ci, out_h=Ho, out_w=Wo, cout=c.co, ksize=c.k, stride=c.s,
                 dilation=c.dil, pad=c.pad, k_total=ktot, cout_pad=cpad, act1=1, src=1, weight=1, scale1=1, shift1=1, out_raw=1,
                 zero_page=1)
        knobs = [0] + list(force or (0, 0)) + [conv64, 1]
        lines.append(" ".join(str(x) for x in [v[f] for f in fields] + knobs))
        ktots.append(ktot)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PPN_")}
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = []
    for line in out.stdout.split("\n")[:-1]:
        p = line.split("\t")
        n = int(p[2])
        segs = [dict(zip(SEG, p[4 + 10 * i: 14 + 10 * i])) for i in range(n)]
        for s in segs:
            s.update({k: int(s[k]) for k in SEG[2:]})
        got.append({"rc": int(p[0]), "error": p[1], "segs": segs})
    assert len(got) == len(lines)
    return list(zip(_entries(), ktots, got))


def test_every_case_reaches_the_kernel_and_tile_it_is_for(routed):
    for (name, dtype, purpose, conv64), ktot, g in routed:
        c = FC.ALL[name][0]
        assert g["rc"] == 0, (name, dtype, g["error"])                    # the dispatch refuses none of the cases
        assert len(g["segs"]) == 1
        seg = g["segs"][0]
        assert (seg["m_lo"], seg["m_hi"]) == (0, FC.pixels(c))
        assert seg["name"] == FC.kernel_name(purpose, dtype), (name, dtype, conv64, seg["name"])
        assert FC.check_purpose(c, purpose, seg, ktot) is None, (name, dtype, conv64, FC.check_purpose(c, purpose, seg, ktot))


def test_the_purposes_cover_what_the_issue_lists(routed):
    by = {(n, d, k): (p, kt, g["segs"][0]) for (n, d, p, k), kt, g in routed}
    assert 128 // 6 >= 21 and by[("many_images", "f32", 1)][2]["n_ptiles"] == 2
    for d in ("bf16", "f16"):
        assert by[("many_images", d, 1)][2]["kind"] == "conv64" and by[("many_images", d, 0)][2]["kind"] == "big"
        assert by[("sweep/conv64", d, 1)][2]["kind"] == "conv64" and by[("sweep/conv64", d, 0)][2]["kind"] == "big"
        assert by[("c32_1x1_s2", d, 1)][2]["kind"] == "generic"
    for d in DT:
        assert FC.pixels(FC.ALL["exact_tiles"][0]) % by[("exact_tiles", d, 1)][2]["bp"] == 0
        assert by[("exact_tiles/256", d, 1)][2]["n_ptiles"] == 1 and by[("exact_tiles", d, 1)][2]["n_ptiles"] == 2
        assert by[("cout72", d, 1)][2]["n_ctiles"] == 2
        assert by[("cin8", d, 1)][1] == (96 if d == "f32" else 128)
        assert by[("cin16_5x5", d, 1)][1] == (416 if d == "f32" else 448)
    kinds = {(g["kind"], g["bp"], g["bc"]) for _, _, g in by.values()}
    assert {("generic", 256, 16), ("generic", 256, 32), ("generic", 128, 64), ("big", 128, 64), ("big", 128, 128),
            ("big", 128, 256), ("big", 256, 128), ("conv64", 0, 0)} <= kinds
