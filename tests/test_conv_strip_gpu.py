"""Strip loader of the large-tile convolution kernel (csrc/conv_big.hip, template flag SP; include/ppn.h
ppn_last_conv_strip / ppn_set_conv_strip_enabled).

3x3 stride-1 "same" convolutions of the 16-bit modes whose 192-pixel tiles are whole image rows stage ONE activation strip per
filter row instead of one stage per tap.  Weights, K order and the MFMA sequence are those of the per-tap loader, so

* every eligible launch must be BIT-identical with the switch on and off, and report ppn_last_conv_strip() = 1 / 0 (a silent
  fall-back cannot pass); the shapes are the smallest that reach every mechanism: R = 4, 8, 6, 2 image rows per tile, strips
  of 224, 256, 240 and 208 rows, dilation 1 / 2 / 4 (at 4x48 with dilation 4 every dy != 1 row is padding), MFMA pixel tiles
  that straddle image rows (Wo = 24), one tile and several tiles through the XCD remap (batch 1 / 3), one 64-channel slab
  and three (the strip-buffer parity wraps), both NHWC epilogues;
* one case per dtype is checked against torch CPU f32 conv2d with the tolerance of test_conv_tiles_gpu.py, so "both paths
  wrong alike" cannot pass;
* launches the loader does not cover report 0 and equal the switched-off result;
* a plan (ppn_plan_run: direct runs, then the captured graph) takes the same decision and gives the same bits."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import forward_cases as FC
from test_conv_gpu import BF16_TOL, F16_TOL, q, rnd, run_conv

pytestmark = pytest.mark.gpu

COUT = 256
GEOMS = [(4, 48, 1), (4, 48, 2), (4, 48, 4), (8, 24, 1), (8, 24, 2), (8, 24, 4), (6, 32, 1), (6, 32, 2), (2, 96, 1)]


def _dt(name):
    from pytorch_pose_proposal_network_amd import lib as L
    return {"bf16": L.PPN_BF16, "f16": L.PPN_F16}[name]


def _kname(dtype_name, bp=192, bc=256, sc=False):
    return "conv_igemm_big_kernel<%s, %d, %d, 8, %s>" % ({"bf16": "__bf16", "f16": "_Float16"}[dtype_name], bp, bc,
                                                         "true" if sc else "false")


@pytest.fixture
def strip():
    """strip(on): the process-wide switch; the 192x256 tile is forced for the test and both are restored after it."""
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    L.check(lib.ppn_set_conv_tile_override(192, 256), "ppn_set_conv_tile_override")

    def switch(on):
        L.check(lib.ppn_set_conv_strip_enabled(int(on)), "ppn_set_conv_strip_enabled")

    switch(True)
    yield switch
    switch(True)
    L.check(lib.ppn_set_conv_tile_override(0, 0), "ppn_set_conv_tile_override")


def _both(strip, x, w, dtype, kernel, want_on, **kw):
    """The same launch with the switch on and off -> (outputs on, outputs off); asserts the kernel name both times, the strip
    report `want_on` / 0, and that the outputs are free of NaN inside the launched range and bit-identical."""
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    outs = []
    for on in (True, False):
        strip(on)
        info = {}
        res = run_conv(x, w, dtype, info=info, **kw)
        took = lib.ppn_last_conv_strip()
        assert info["kernel"] == kernel, info["kernel"]
        assert took == (want_on if on else 0), (on, took)
        outs.append([t for t in res if t is not None])
    for a, b in zip(*outs):
        assert torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0))
    return outs


def _operands(dtype, B, Cin, Ho, Wo, k=3, H=None, W=None, cout=COUT, seed=0):
    x = q(rnd(B, Cin, H or Ho, W or Wo, seed=700 + seed), dtype)
    w = q(rnd(cout, Cin, k, k, seed=710 + seed, scale=(2.0 / (Cin * k * k)) ** 0.5), dtype)
    s1 = 0.5 + torch.rand(cout, generator=torch.Generator().manual_seed(720 + seed))
    b1 = rnd(cout, seed=730 + seed, scale=0.3)
    return x, w, s1, b1


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
@pytest.mark.parametrize("batch,cin", [(1, 64), (3, 192)])
@pytest.mark.parametrize("geom", GEOMS, ids=["%dx%d_d%d" % g for g in GEOMS])
def test_strip_is_bit_identical_single_output(strip, geom, batch, cin, dtype_name):
    Ho, Wo, dil = geom
    dtype = _dt(dtype_name)
    x, w, s1, b1 = _operands(dtype, batch, cin, Ho, Wo)
    (on,), _ = _both(strip, x, w, dtype, _kname(dtype_name), 1, dil=dil, pad=dil, s1=s1, b1=b1, act1=1)
    assert not torch.isnan(on).any()


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
@pytest.mark.parametrize("batch,cin", [(1, 192), (3, 64)])
def test_strip_is_bit_identical_residual_and_second_output(strip, batch, cin, dtype_name):
    """conv2 of a BasicBlock (raw = acc + residual, act = relu(bn_next(raw))): the chunked f32 epilogue."""
    dtype = _dt(dtype_name)
    Ho, Wo, dil = 4, 48, 2
    x, w, s2, b2 = _operands(dtype, batch, cin, Ho, Wo, seed=1)
    res = q(rnd(batch, COUT, Ho, Wo, seed=741), dtype)
    (raw, act), _ = _both(strip, x, w, dtype, _kname(dtype_name), 1, dil=dil, pad=dil, residual=res, s2=s2, b2=b2, act2=1,
                          want_act=True)
    assert not torch.isnan(raw).any() and not torch.isnan(act).any()


@pytest.mark.parametrize("dtype_name,geom", [("bf16", (8, 24, 2)), ("f16", (4, 48, 4))])
def test_strip_against_torch_cpu_f32(strip, dtype_name, geom):
    Ho, Wo, dil = geom
    dtype = _dt(dtype_name)
    x, w, s1, b1 = _operands(dtype, 3, 192, Ho, Wo, seed=2)
    (on,), _ = _both(strip, x, w, dtype, _kname(dtype_name), 1, dil=dil, pad=dil, s1=s1, b1=b1, act1=1)
    ref = F.relu(F.conv2d(x, w, None, 1, dil, dil) * s1.view(1, -1, 1, 1) + b1.view(1, -1, 1, 1))
    tol = {"bf16": BF16_TOL, "f16": F16_TOL}[dtype_name] * max(1.0, float(ref.abs().max()))
    err = float((on - ref).abs().max())
    print("max |gpu - cpu f32| = %.3g (tolerance %.3g)" % (err, tol))
    assert not torch.isnan(on).any() and err <= tol
    # per element against f64 (tests/forward_cases.py): the strip loader has no f32 form to hold it tighter
    r = FC.ratios_of(dtype_name, x, w, 1, dil, dil, s1, b1, act1=1, raw=on)
    print("per-element bound: ratio %.3f" % r["raw"])
    assert r["raw"] <= 1.0


def test_ineligible_launches_keep_the_per_tap_loader(strip):
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    dtype, name = L.PPN_BF16, _kname("bf16")
    # Wo = 20 does not divide 192
    x, w, s1, b1 = _operands(dtype, 2, 64, 12, 20, seed=3)
    _both(strip, x, w, dtype, name, 0, dil=1, pad=1, s1=s1, b1=b1, act1=1)
    # stride 2 (output 4 x 48 from 8 x 96)
    x, w, s1, b1 = _operands(dtype, 1, 64, 4, 48, H=8, W=96, seed=4)
    _both(strip, x, w, dtype, name, 0, stride=2, dil=1, pad=1, s1=s1, b1=b1, act1=1)
    # 1x1
    x, w, s1, b1 = _operands(dtype, 1, 64, 4, 48, k=1, seed=5)
    _both(strip, x, w, dtype, name, 0, s1=s1, b1=b1, act1=1)
    # a ragged last tile (pixel range of 500 of the 576 pixels), and a range that begins inside a tile
    x, w, s1, b1 = _operands(dtype, 3, 64, 4, 48, seed=6)
    _both(strip, x, w, dtype, name, 0, dil=1, pad=1, s1=s1, b1=b1, act1=1, ranges=[(0, 500, None)])
    _both(strip, x, w, dtype, name, 0, dil=1, pad=1, s1=s1, b1=b1, act1=1, ranges=[(96, 384, None)])
    # ... while whole tiles of a range take the strips
    _both(strip, x, w, dtype, name, 1, dil=1, pad=1, s1=s1, b1=b1, act1=1, ranges=[(192, 384, None)])
    # a fused projection shortcut
    x, w, _, b1 = _operands(dtype, 1, 64, 4, 48, seed=7)
    x2 = q(rnd(1, 64, 7, 95, seed=751), dtype)
    w2 = q(rnd(COUT, 64, 1, 1, seed=752, scale=0.1), dtype)
    _both(strip, x, w, dtype, _kname("bf16", sc=True), 0, dil=1, pad=1, b1=b1, shortcut=(x2, w2, 2))
    # forced 192x128 and 256x256 tiles
    x, w, s1, b1 = _operands(dtype, 3, 64, 4, 48, seed=8)
    for bp, bc in ((192, 128), (256, 256)):
        L.check(lib.ppn_set_conv_tile_override(bp, bc), "ppn_set_conv_tile_override")
        _both(strip, x, w, dtype, _kname("bf16", bp, bc), 0, dil=1, pad=1, s1=s1, b1=b1, act1=1)


def _device_conv(x, w, dtype, dil):
    """A 3x3 stride-1 "same" descriptor on device tensors -> (desc, out tensor NHWC, keep-alive list)."""
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    dev = torch.device("cuda")
    tdt = {L.PPN_BF16: torch.bfloat16, L.PPN_F16: torch.float16}[dtype]
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    kstep, _, korder, ktot, cpad = L.conv_tiling(dtype, Cin, Cout, 3)
    st = torch.cuda.current_stream().cuda_stream
    wd = w.contiguous().to(dev)
    packed = torch.empty(cpad, ktot, dtype=tdt, device=dev)
    L.check(lib.ppn_pack_weight(dtype, wd.data_ptr(), Cout, Cin, 3, cpad, ktot, korder, kstep, packed.data_ptr(), st))
    xs = x.permute(0, 2, 3, 1).contiguous().to(dev, tdt)
    zero = torch.zeros(64, device=dev)
    out = torch.full((B, H, W, Cout), float("nan"), device=dev).to(tdt)
    d = L.ConvDesc()
    d.dtype, d.batch, d.in_h, d.in_w, d.cin = dtype, B, H, W, Cin
    d.out_h, d.out_w, d.cout = H, W, Cout
    d.ksize, d.stride, d.dilation, d.pad = 3, 1, dil, dil
    d.k_total, d.cout_pad = ktot, cpad
    d.src, d.weight, d.zero_page, d.out_raw = xs.data_ptr(), packed.data_ptr(), zero.data_ptr(), out.data_ptr()
    return d, out, [wd, packed, xs, zero]


def test_stats_mode_keeps_the_per_tap_loader(strip):
    """ppn_conv_desc.stats_mode = 1 (BatchNorm sums from the epilogue): its own instantiation, never the strip loader."""
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    dtype = L.PPN_BF16
    x, w, _, _ = _operands(dtype, 3, 64, 4, 48, seed=9)
    st = torch.cuda.current_stream().cuda_stream
    got = []
    for on in (True, False):
        strip(on)
        d, out, keep = _device_conv(x, w, dtype, 1)
        part = torch.zeros(3 * COUT * 2, dtype=torch.float64, device="cuda")
        tiles = C.c_int32(-1)
        d.stats_mode, d.stats_partial, d.stats_tiles = 1, part.data_ptr(), C.pointer(tiles)
        L.check(lib.ppn_conv2d_fused(C.byref(d), st), "ppn_conv2d_fused")
        torch.cuda.synchronize()
        assert lib.ppn_last_conv_kernel().decode() == "conv_igemm_big_kernel<__bf16, 192, 256, 8, false, false, true>"
        assert lib.ppn_last_conv_strip() == 0 and tiles.value == 3
        got.append((out.float().cpu(), part.cpu()))
    assert not torch.isnan(got[0][0]).any()
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


def test_plan_takes_the_same_decision(strip):
    """Two chained launches at 4 x 48 (dilation 2, then 1) through ppn_plan_run -- two direct runs, then the captured graph --
    equal the direct ppn_conv2d_fused calls, with the switch on and off."""
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    dtype = L.PPN_BF16
    x, w1, _, _ = _operands(dtype, 3, 64, 4, 48, seed=10)
    w2 = q(rnd(COUT, COUT, 3, 3, seed=761, scale=(2.0 / (COUT * 9)) ** 0.5), dtype)
    side = torch.cuda.Stream()                                    # the legacy default stream cannot be captured
    results = []
    with torch.cuda.stream(side):
        st = side.cuda_stream
        for on in (True, False):
            strip(on)
            d1, mid, keep1 = _device_conv(x, w1, dtype, 2)
            d2, out, keep2 = _device_conv(torch.zeros(3, COUT, 4, 48), w2, dtype, 1)
            d2.src = mid.data_ptr()
            for d in (d1, d2):
                L.check(lib.ppn_conv2d_fused(C.byref(d), st), "ppn_conv2d_fused")
                assert lib.ppn_last_conv_kernel().decode() == _kname("bf16") and lib.ppn_last_conv_strip() == int(on)
            torch.cuda.synchronize()
            direct = out.float().cpu()
            assert not torch.isnan(direct).any()
            plan = C.c_void_p()
            L.check(lib.ppn_plan_create(C.byref(plan)), "ppn_plan_create")
            try:
                L.check(lib.ppn_plan_add_conv(plan, C.byref(d1)), "ppn_plan_add_conv")
                L.check(lib.ppn_plan_add_conv(plan, C.byref(d2)), "ppn_plan_add_conv")
                for _ in range(4):
                    mid.fill_(float("nan"))
                    out.fill_(float("nan"))
                    L.check(lib.ppn_plan_run(plan, st), "ppn_plan_run")
                    torch.cuda.synchronize()
                    assert torch.equal(out.float().cpu(), direct)
                assert lib.ppn_plan_graph_captures(plan) == 1
            finally:
                L.check(lib.ppn_plan_destroy(plan), "ppn_plan_destroy")
            results.append(direct)
    assert torch.equal(results[0], results[1])
