"""CPU: the split-K edge cases (tests/splitk_cases.py) are what they claim, the partition emulation partitions, and the two
detectors of tests/test_splitk_edges_gpu.py see the faults a split-K pair can have.  No GPU.

* the f64 reference of every case equals an explicit loop over the filter taps, the all-padding ring of `overpad` equals
  act1(b1), and each case has the property it is listed for (reach, divisor, ragged slab length, mid-tap slab start, ...);
* slab_terms() puts every (tap, input channel) term into exactly one slab and counts the slabs as ppn_conv_splitk_workspace
  does (host-only entry point; libppn.so is built on demand);
* every (case, dtype) routes to conv_splitk_partial_kernel<elem, 128, 64, 2, 2> with the expected tile counts
  (tools/conv_route_check.cpp, as tests/test_forward_edges_cpu.py drives it);
* the emulation of a correct pair -- an f32 partial per slab, summed 0 .. S-1 in f32, f32 epilogue, one rounding -- stays at
  ratio <= 1 under forward_cases' UNCHANGED bound, and on the exact operands equals the once-rounded f64 result bit for bit;
* each planted fault gives ratio > 1 AND a difference on the exact operands -- except one lost input element at K = 18432, which
  the bound does NOT see and the exact comparison does: that is why the exact test exists."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

import forward_cases as FC
import splitk_cases as SK
from conv_route_cases import load as load_fixture
from test_conv_route_cpu import CSRC, ROOT, SEG

DT = SK.DTYPE_NAMES
CONVS = {n: v[0] for n, v in SK.CASES.items()}


@pytest.fixture(scope="module")
def L():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def _desc_fields(L, c, dtype):
    Ho, Wo = FC.out_hw(c)
    code = {"f32": L.PPN_F32, "bf16": L.PPN_BF16, "f16": L.PPN_F16}[dtype]
    return dict(dtype=code, batch=c.B, in_h=c.H, in_w=c.W, cin=c.ci, out_h=Ho, out_w=Wo, cout=c.co, ksize=c.k, stride=c.s,
                dilation=c.dil, pad=c.pad, k_total=FC.depth(c), cout_pad=SK.cout_pad(c), act1=1, flags=L.PPN_CONV_SPLIT_K)


# ---- reference and cases ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SK.CASES))
def test_reference_equals_the_loop_over_taps(name):
    c = CONVS[name]
    for dtype in ("bf16",) if FC.depth(c) > 4608 else DT:       # the 2048-wide case once: the loop does not depend on the dtype
        op = SK.operands(name, dtype)
        acc, S = FC.conv_f64(c, op)
        taps = FC.conv_by_taps(c, op["x"], op["w"])
        assert taps.shape == acc.shape == (c.B, c.co) + FC.out_hw(c)
        assert float((acc - taps).abs().max()) <= 1e-12 * max(1.0, float(taps.abs().max()))
        mag = FC.conv_by_taps(c, op["x"].abs(), op["w"].abs())
        assert float((S - mag).abs().max()) <= 1e-12 * max(1.0, float(mag.abs().max()))


def test_overpad_ring_equals_act1_of_b1():
    c = CONVS["overpad"]
    ring = FC.no_tap_inside(c)
    assert ring[0].all() and ring[-1].all() and ring[:, 0].all() and ring[:, -1].all() and not ring[1:-1, 1:-1].any()
    assert c.pad > c.dil * (c.k - 1)
    for dtype in DT:
        op = SK.operands("overpad", dtype)
        ref, _ = SK.reference("overpad", dtype, "bn_relu")
        want = F.relu(op["b1"].double()).view(1, -1, 1, 1).expand_as(ref["raw"])
        assert torch.equal(ref["raw"][:, :, ring], want[:, :, ring])
        assert not torch.equal(ref["raw"][:, :, ~ring], want[:, :, ~ring])
    assert [n for n, c in CONVS.items() if FC.no_tap_inside(c).any()] == ["overpad"]


def test_cases_are_the_edges_they_claim():
    for n, c in CONVS.items():                                   # splitk_check's scope, in every dtype
        assert c.ci % 64 == 0 and c.co % 8 == 0 and c.k in (1, 3), n
        assert FC.pixels(c) * c.co <= 40000, n                   # a launch stays milliseconds
    # slab counts: ceil(K / 512), the same in every dtype
    for n, (c, slabs, _) in SK.CASES.items():
        assert all(slabs[d] == -(-FC.depth(c) // SK.SLAB) == len(SK.slab_terms(c, d)) for d in DT), n
    assert FC.depth(CONVS["nine_slabs"]) == 4608 and SK.CASES["nine_slabs"][1]["bf16"] == 9
    assert FC.depth(CONVS["deep_36_slabs"]) == 18432 and SK.CASES["deep_36_slabs"][1]["bf16"] == 36
    assert max(max(s.values()) for _, s, _ in SK.CASES.values()) == 36
    # nine_slabs: no slab after the first starts on a channel-chunk boundary (tap 0 of the channel-chunk-major order)
    for n in ("nine_slabs", "nine_slabs_d2_ct2"):
        for d in DT:
            starts = [steps[0] for steps in SK.slab_steps(CONVS[n], d)]
            assert starts[0] == (0, 0) and all(tap != 0 for tap, _ in starts[1:]), (n, d, starts)
    c = CONVS["nine_slabs_d2_ct2"]
    assert SK.cout_pad(c) == 128 == 2 * SK.TILE_C and SK.cout_pad(c) - c.co == 56 and c.dil == 2
    # every pixel of deep_36_slabs is a border pixel: some tap of it lies outside the image
    c = CONVS["deep_36_slabs"]
    assert FC.out_hw(c) == (c.H, c.W) and all(min(o, n - 1 - o) < c.dil for n in (c.H, c.W) for o in range(n))
    c = CONVS["reach_gt_image"]                                  # off-centre filter rows wholly in padding
    assert c.dil >= c.H and c.pad == c.dil and FC.out_hw(c) == (c.H, c.W)
    assert FC.out_hw(CONVS["ho1"])[0] == 1 and FC.out_hw(CONVS["wo1"])[1] == 1 and FC.out_hw(CONVS["one_pixel"]) == (1, 1)
    assert FC.out_hw(CONVS["ho1"])[1] > 1 and FC.out_hw(CONVS["wo1"])[0] > 1 and FC.pixels(CONVS["one_pixel"]) == 3
    for n in ("s2_odd/3x3", "s2_odd/1x1"):
        c = CONVS[n]
        odd = [(dim + 2 * c.pad - c.k) % 2 for dim in (c.H, c.W)]
        assert c.s == 2 and sorted(odd) == [0, 1] and FC.depth(c) == 576
        # the ragged last slab: 64 K elements = one 16-bit step, two f32 steps
        assert [len(SK.slab_steps(c, d)[-1]) for d in DT] == [2, 1, 1]
        assert [len(SK.slab_steps(c, d)[0]) for d in DT] == [16, 8, 8]
        assert all(int(SK.slab_terms(c, d)[-1].sum()) == 64 for d in DT)
    assert CONVS["s2_odd/1x1"].k == 1 and CONVS["s2_odd/1x1"].pad == 0
    c = CONVS["valid"]
    assert c.pad == 0 and c.k == 3 and FC.out_hw(c)[0] < c.H
    c = CONVS["many_images"]
    Ho, Wo = FC.out_hw(c)
    assert 21 <= SK.TILE_P // (Ho * Wo) and FC.pixels(c) == 240 and FC.pixels(c) % SK.TILE_P != 0
    assert FC.pixels(CONVS["exact_tiles"]) % SK.TILE_P == 0 and FC.pixels(CONVS["exact_tiles"]) == 256
    # tap-major pack; slab 1 starts in the middle of a tap (not at its first channel), in every dtype
    c = CONVS["tap_major_mid_tap"]
    assert SK.tap_major(c) and c.co < 64
    for d in DT:
        assert c.ci // SK.BK[d] == (6 if d == "f32" else 3)
        tap, ci0 = SK.slab_steps(c, d)[1][0]
        assert (tap, ci0) == (2, 128), (d, tap, ci0)
        assert (SK.SLAB // SK.BK[d]) % (c.ci // SK.BK[d]) != 0   # 8 steps per slab, 3 per tap
    # ... and it is the tap-major order that makes the difference: the other formula starts slab 1 elsewhere
    assert SK.k_steps(c, "bf16", tap_major_order=False)[8] != SK.k_steps(c, "bf16")[8]
    assert [n for n, c in CONVS.items() if SK.tap_major(c)] == ["tap_major_mid_tap", "cout8"]
    assert CONVS["cout8"].co == 8 and SK.cout_pad(CONVS["cout8"]) == 64
    c = CONVS["one_step"]
    assert FC.depth(c) == 64 and [len(SK.k_steps(c, d)) for d in DT] == [2, 1, 1]
    # the epilogues: two per case, all eight on the sweep case, the bf16 store once
    rs = SK.runs()
    assert len(rs) == len(set(rs)) == (len(CONVS) - 1) * 3 * 2 + 3 * 8 + 1
    assert {e for n, _, e, _ in rs if n == SK.SWEEP_CASE} == set(FC.EPILOGUES) and len(FC.EPILOGUES) == 8
    assert [r for r in rs if r[3]] == [("nine_slabs_d2_ct2", "f16", "res_dual", True)]
    assert set(SK.EXACT_CASES) | set(SK.BATCH_CASES) <= set(CONVS)


# ---- the partition ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SK.CASES))
def test_slab_terms_partition_the_depth(name, L):
    c = CONVS[name]
    lib = L.load()
    for dtype in DT:
        masks = SK.slab_terms(c, dtype)
        count = torch.stack(masks).sum(0)
        assert count.shape == (c.k * c.k, c.ci) and bool((count == 1).all()), "a term in no slab or in two"
        assert all(int(m.sum()) == SK.SLAB for m in masks[:-1]) and 0 < int(masks[-1].sum()) <= SK.SLAB
        # each K step is bk consecutive channels of ONE tap, and the steps come in the packed order
        steps = [s for slab in SK.slab_steps(c, dtype) for s in slab]
        assert steps == SK.k_steps(c, dtype) and len(set(steps)) == len(steps) == FC.depth(c) // SK.BK[dtype]
        n, slabs = C.c_int64(), C.c_int32()
        d = L.ConvDesc(**_desc_fields(L, c, dtype))
        assert lib.ppn_conv_splitk_workspace(C.byref(d), C.byref(n), C.byref(slabs)) == 0, lib.ppn_last_error()
        assert slabs.value == len(masks) == SK.CASES[name][1][dtype]
        assert n.value == slabs.value * FC.pixels(c) * SK.cout_pad(c) * 4
        # cout_pad is ppn_conv_tiling's wherever the split-K tile divides that; the tap-major order is its k_order 0
        _, _, korder, ktot, cpad = L.conv_tiling(d.dtype, c.ci, c.co, c.k)
        assert ktot == FC.depth(c) and (korder == 0) == SK.tap_major(c)
        if name == "cout8":
            assert cpad == 16 and SK.cout_pad(c) == 64
            d.cout_pad = cpad                                   # the library's own pad is outside the kernel's scope, and refused
            assert lib.ppn_conv_splitk_workspace(C.byref(d), None, None) == -3 and b"cout_pad" in lib.ppn_last_error()
        else:
            assert cpad == SK.cout_pad(c)


# ---- the route --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def routed(tmp_path_factory, L):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("route") / "conv_route_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "conv_route_check.cpp"), os.path.join(CSRC, "conv_route.cpp"), "-o", exe],
                   check=True)
    fields, _ = load_fixture()
    assert len(fields) == 53
    entries = [(n, d) for n in SK.CASES for d in DT]
    lines = []
    for name, dtype in entries:
        c = CONVS[name]
        v = dict.fromkeys(fields, 0)
        v.update(_desc_fields(L, c, dtype), src=1, weight=1, scale1=1, shift1=1, out_raw=1, zero_page=1, splitk_ws=1,
                 splitk_ws_bytes=1 << 40)
        lines.append(" ".join(str(x) for x in [v[f] for f in fields] + [0, 0, 0, 1, 1]))
    env = {k: v for k, v in os.environ.items() if not k.startswith("PPN_")}
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = []
    for line in out.stdout.split("\n")[:-1]:
        p = line.split("\t")
        segs = [dict(zip(SEG, p[4 + 10 * i: 14 + 10 * i])) for i in range(int(p[2]))]
        for s in segs:
            s.update({k: int(s[k]) for k in SEG[2:]})
        got.append({"rc": int(p[0]), "error": p[1], "segs": segs})
    assert len(got) == len(lines)
    return list(zip(entries, got))


def test_every_case_reaches_the_split_k_kernel(routed):
    for (name, dtype), g in routed:
        c = CONVS[name]
        assert g["rc"] == 0, (name, dtype, g["error"])           # a case that stops reaching the kernel fails here
        assert len(g["segs"]) == 1
        seg = g["segs"][0]
        assert (seg["m_lo"], seg["m_hi"]) == (0, FC.pixels(c))
        assert seg["name"] == SK.kernel_name(dtype) and seg["kind"] == "splitk", (name, dtype, seg["name"])
        assert seg["n_ptiles"] == -(-FC.pixels(c) // SK.TILE_P) and seg["n_ctiles"] == SK.cout_pad(c) // SK.TILE_C
        why = FC.check_purpose(c, SK.purpose(name), seg, FC.depth(c))
        assert why is None, (name, dtype, why)
    by = {k: g["segs"][0] for k, g in routed}
    assert by[("many_images", "bf16")]["n_ptiles"] == 2 and by[("exact_tiles", "f32")]["n_ptiles"] == 2
    assert by[("nine_slabs_d2_ct2", "f16")]["n_ctiles"] == 2 and by[("cout8", "f32")]["n_ctiles"] == 1


# ---- the emulation of a correct pair ------------------------------------------------------------------------------------------------

def test_bound_holds_for_the_slab_by_slab_emulation():
    worst = {d: (0.0, None) for d in DT}
    for name, dtype, en, ob in SK.runs():
        c, epi = CONVS[name], FC.EPILOGUES[en]
        ref, bound = SK.reference(name, dtype, en, ob)
        r = SK.worst_ratio(SK.emulate_f32(c, SK.operands(name, dtype), epi, dtype, ob), ref, bound)
        assert r <= 1.0, (name, dtype, en, ob, r)
        if r > worst[dtype][0]:
            worst[dtype] = (r, (name, en, ob))
    for d in DT:
        print("SPLITK_EDGE_CPU emulation worst ratio %s: %.3f at %s" % (d, worst[d][0], worst[d][1]))
    assert worst["bf16"][0] > 0.4 and worst["f16"][0] > 0.4      # the store's rounding is what fills the 16-bit bound


def test_partials_add_up_to_the_reference():
    for name in SK.CASES:
        c = CONVS[name]
        P, Pmag = SK.partials_f64(c, SK.operands(name, "f16"), "f16")
        acc, S = SK._conv_f64(name, "f16")
        assert P.shape == (SK.CASES[name][1]["f16"], c.B, c.co) + FC.out_hw(c)
        assert float((P.sum(0) - acc).abs().max()) <= 1e-12 * max(1.0, float(acc.abs().max()))
        assert float((Pmag.sum(0) - S).abs().max()) <= 1e-12 * float(S.abs().max())


@pytest.mark.parametrize("name", SK.EXACT_CASES)
def test_emulation_is_exact_on_the_exact_operands(name):
    c = CONVS[name]
    op, want = SK.exact_case(name)
    for en, epi in SK.EXACT_EPILOGUES.items():
        for dtype in DT:
            for k in ("x", "w", "res"):
                assert torch.equal(FC.q(op[k], dtype), op[k])     # the operands are what the storage type holds
            got = SK.emulate_f32(c, op, epi, dtype)
            assert set(got) == set(want[en][dtype]) == {"raw", "act"}
            for k in got:
                assert torch.equal(got[k], want[en][dtype][k]), (name, en, dtype, k)
    # the sums are large enough for a 16-bit store to round (the exact test is not a test of small numbers only)
    assert float(want["res_dual"]["f32"]["raw"].abs().max()) > 256
    # the bf16 store of an f16 launch rounds the same f32 value once
    epi = SK.EXACT_EPILOGUES["res_dual"]
    assert torch.equal(SK.emulate_f32(c, op, epi, "f16", True)["raw"], SK.exact_expected(c, op, epi, "f16", True)["raw"])


def test_exact_operands_refuse_what_is_not_exact():
    c = CONVS["nine_slabs"]
    op = SK.exact_operands(c, 3)
    with pytest.raises(AssertionError):
        SK.check_exact(c, op, FC.EPILOGUES["res_lrelu2"])         # LReLU
    with pytest.raises(AssertionError):
        SK.check_exact(c, dict(op, x=op["x"] * 4096), FC.EPILOGUES["res_dual"])      # sums beyond the exact range
    with pytest.raises(AssertionError):
        SK.check_exact(c, dict(op, x=op["x"] + 0.5), FC.EPILOGUES["res_dual"])


# ---- planted faults -----------------------------------------------------------------------------------------------------------------
# A fault is planted in the emulation: fault(c, op, dtype) -> the f32 partials [S', B, co, Ho, Wo] the reduce step then sums.

def _moved_step(c, op, dtype, w_step, x_step):
    """The contribution of one K step whose weights (tap, channels of w_step) meet the activations of x_step: zero where
    x_step is past the last tap."""
    bk = SK.BK[dtype]
    (tw, cw), (tx, cx) = w_step, x_step
    w = torch.zeros_like(op["w"])
    if tx < c.k * c.k and cx + bk <= c.ci:
        w[:, cx: cx + bk, tx // c.k, tx % c.k] = op["w"][:, cw: cw + bk, tw // c.k, tw % c.k]
    return F.conv2d(op["x"], w, None, c.s, c.pad, c.dil)


def _slab_left_out(c, op, dtype):
    P = SK.partials_f32(c, op, dtype)
    return torch.cat([P[:4], P[5:]])


def _slab_summed_twice(c, op, dtype):
    P = SK.partials_f32(c, op, dtype)
    return torch.cat([P, P[4:5]])


def _ragged_last_slab_skipped(c, op, dtype):
    assert FC.depth(c) % SK.SLAB != 0
    return SK.partials_f32(c, op, dtype)[:-1]


def _slab_starts_one_step_late(c, op, dtype, slab=4):
    steps = SK.slab_steps(c, dtype)
    masks = [SK.terms_of(c, dtype, s[1:] if j == slab else s) for j, s in enumerate(steps)]
    return SK.partials(c, op["x"], op["w"], masks)


def _first_step_with_the_previous_taps_offset(c, op, dtype, slab=1):
    """Slab 1's first K step gathers its activations one tap to the left of where its weights belong."""
    P = _slab_starts_one_step_late(c, op, dtype, slab)
    tap, ci0 = SK.slab_steps(c, dtype)[slab][0]
    assert tap >= 1
    P[slab] += _moved_step(c, op, dtype, (tap, ci0), (tap - 1, ci0))
    return P


def _rows_strided_by_co(c, op, dtype):
    """The partial kernel writes workspace rows of cout_pad floats, the reduce kernel reads them co apart."""
    P = SK.partials_f32(c, op, dtype)
    S, M, cp = P.shape[0], FC.pixels(c), SK.cout_pad(c)
    assert cp != c.co
    ws = torch.zeros(S, M, cp)
    ws[:, :, : c.co] = P.permute(0, 1, 3, 4, 2).reshape(S, M, c.co)
    read = ws.reshape(S, M * cp)[:, : M * c.co].reshape(S, c.B, *FC.out_hw(c), c.co)
    return read.permute(0, 1, 4, 2, 3).contiguous()


def _tap_major_start_by_the_other_formula(c, op, dtype):
    """Every slab's first (tap, channel) comes from the channel-chunk-major formula (s % ntaps, s / ntaps) and is then advanced
    in the tap-major order; the weights are the packed rows' own."""
    assert SK.tap_major(c)
    bk, ntaps, per = SK.BK[dtype], c.k * c.k, SK.SLAB // SK.BK[dtype]
    out = []
    for j, steps in enumerate(SK.slab_steps(c, dtype)):
        s0 = j * per
        tap, ci0 = s0 % ntaps, (s0 // ntaps) * bk
        acc = 0
        for w_step in steps:
            acc = acc + _moved_step(c, op, dtype, w_step, (tap, ci0))
            ci0 += bk
            if ci0 >= c.ci:
                ci0, tap = 0, tap + 1
        out.append(acc)
    return torch.stack(out)


def _border_mask_ignored_at_a_corner(c, op, dtype):
    """Output pixel (0, 0) of the last image, centre-row left tap: column -dil of row 0 is masked; unmasked, the address is
    column W - dil of the last row of the image before."""
    P = SK.partials_f32(c, op, dtype)
    assert c.B > 1 and c.pad == c.dil and 0 < c.W - c.dil and c.s == 1
    P[0][-1, :, 0, 0] += op["w"][:, :, 1, 0] @ op["x"][-2, :, c.H - 1, c.W - c.dil]
    return P


def _one_input_element_lost(c, op, dtype):
    x = op["x"].clone()
    b, y, xx = c.B - 1, c.H // 2, c.W // 2
    mag = x[b, :, y, xx].abs()
    ch = int((mag - x.abs().median()).abs().argmin())            # a typical element, neither large nor near zero
    assert x[b, ch, y, xx] != 0
    x[b, ch, y, xx] = 0.0
    return SK.partials(c, x, op["w"], SK.slab_terms(c, dtype))


# fault -> (case, epilogue, how, the bound sees it)
FAULTS = {
    "a slab left out of the sum": ("nine_slabs", "bn_relu", _slab_left_out, True),
    "a slab summed twice": ("nine_slabs", "bn_relu", _slab_summed_twice, True),
    "the ragged last slab skipped": ("s2_odd/1x1", "res_dual", _ragged_last_slab_skipped, True),
    "a slab starting one K step late": ("nine_slabs", "bn_relu", _slab_starts_one_step_late, True),
    "a slab's first step using the previous tap's offset": ("nine_slabs", "bn_relu", _first_step_with_the_previous_taps_offset,
                                                            True),
    "workspace rows strided by co instead of cout_pad": ("nine_slabs_d2_ct2", "res_dual", _rows_strided_by_co, True),
    "tap-major slab start by the channel-chunk-major formula": ("tap_major_mid_tap", "bn_relu",
                                                                _tap_major_start_by_the_other_formula, True),
    "border mask of one tap ignored at a corner pixel": ("reach_gt_image", "bn_relu", _border_mask_ignored_at_a_corner, True),
    # K = 18432: (K + 4) u S is several times the contribution of one element -- the bound does NOT see this one; the
    # exact-operand comparison does, which is why tests/test_splitk_edges_gpu.py has it
    "one lost input element at K = 18432": ("deep_36_slabs", "res_dual", _one_input_element_lost, False),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_detectors_see_the_planted_fault(fault):
    name, en, plant, bound_sees = FAULTS[fault]
    c, epi = CONVS[name], FC.EPILOGUES[en]
    for dtype in DT:
        op = SK.operands(name, dtype)
        ref, bound = SK.reference(name, dtype, en)
        clean = SK.worst_ratio(SK.emulate_f32(c, op, epi, dtype), ref, bound)
        r = SK.worst_ratio(SK.reduce_f32(plant(c, op, dtype), op, epi, dtype), ref, bound)
        print("SPLITK_EDGE_CPU fault '%s' on %s %s: ratio %.2f (clean %.2f)" % (fault, name, dtype, r, clean))
        assert clean <= 1.0
        assert (r > 1.0) == bound_sees, (fault, name, dtype, r)
    # the exact-operand form: any fault changes bits, in every dtype and on both outputs' raw sum
    xop = SK.exact_operands(c, 5)
    xepi = SK.EXACT_EPILOGUES["res_dual"]
    for dtype in DT:
        want = SK.exact_expected(c, xop, xepi, dtype)
        assert torch.equal(SK.emulate_f32(c, xop, xepi, dtype)["raw"], want["raw"])
        bad = SK.reduce_f32(plant(c, xop, dtype), xop, xepi, dtype)
        n = int((bad["raw"] != want["raw"]).sum())
        print("SPLITK_EDGE_CPU fault '%s' on %s %s, exact operands: %d of %d elements differ" % (
            fault, name, dtype, n, want["raw"].numel()))
        assert n > 0, (fault, name, dtype)
