"""GPU: the split-K convolution (csrc/conv_splitk.hip, ppn_conv_desc.flags & PPN_CONV_SPLIT_K) through the C ABI -- parity with
the fp64 torch-CPU convolution at the tolerances of test_conv_gpu.py, determinism, batch independence, workspace hygiene,
the refusals, and that descriptors without the flag run exactly as before."""
import ctypes as C

import pytest
import torch

from test_conv_gpu import BF16_TOL, F16_TOL, F32_TOL, q, ref_conv, rnd

pytestmark = pytest.mark.gpu

F32, BF16, F16, X3 = 0, 1, 2, 3
TOL = {F32: F32_TOL, BF16: BF16_TOL, F16: F16_TOL}
DTYPES = [F32, BF16, F16]
INVALID, UNSUPPORTED = -1, -3


class Conv:
    """One convolution's device operands and descriptor; `launch()` runs it and returns (rc, kernel name)."""

    def __init__(self, x, w, dtype, stride=1, dil=1, pad=0, s1=None, b1=None, act1=0, residual=None, s2=None, b2=None,
                 act2=0, want_raw=True, want_act=False, flags=0, out_bf16=False):
        from pytorch_pose_proposal_network_amd import lib as L
        self.L, self.lib = L, L.load()
        dev = torch.device("cuda")
        pack_dt = F16 if dtype == X3 else dtype
        tdt = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}[pack_dt]
        B, Cin, H, W = x.shape
        Cout, _, k, _ = w.shape
        eff = dil * (k - 1) + 1
        Ho, Wo = (H + 2 * pad - eff) // stride + 1, (W + 2 * pad - eff) // stride + 1
        kstep, _, korder, ktot, cpad = L.conv_tiling(pack_dt, Cin, Cout, k)
        self.st = torch.cuda.current_stream().cuda_stream
        wd = w.contiguous().to(dev)
        packed = torch.empty(cpad, ktot, dtype=tdt, device=dev)
        L.check(self.lib.ppn_pack_weight(pack_dt, wd.data_ptr(), Cout, Cin, k, cpad, ktot, korder, kstep, packed.data_ptr(),
                                         self.st))
        xs = x.permute(0, 2, 3, 1).contiguous().to(dev, tdt)
        self.keep = [wd, packed, xs, torch.zeros(64, device=dev)]
        d = self.d = L.ConvDesc()
        d.dtype, d.batch, d.in_h, d.in_w, d.cin = dtype, B, H, W, Cin
        d.out_h, d.out_w, d.cout = Ho, Wo, Cout
        d.ksize, d.stride, d.dilation, d.pad = k, stride, dil, pad
        d.k_total, d.cout_pad, d.act1, d.act2 = ktot, cpad, act1, act2
        d.src, d.weight, d.zero_page = xs.data_ptr(), packed.data_ptr(), self.keep[3].data_ptr()
        d.flags = flags | (L.PPN_CONV_OUT_BF16 if out_bf16 else 0)

        def dv(t):
            if t is None:
                return None
            self.keep.append(t.float().contiguous().to(dev))
            return self.keep[-1].data_ptr()
        d.scale1, d.shift1, d.scale2, d.shift2 = dv(s1), dv(b1), dv(s2), dv(b2)
        if residual is not None:
            self.keep.append(residual.permute(0, 2, 3, 1).contiguous().to(dev, tdt))
            d.residual = self.keep[-1].data_ptr()
        odt = torch.bfloat16 if out_bf16 else tdt
        self.raw = self.act = None
        if want_raw:
            self.raw = torch.full((B, Ho, Wo, Cout), float("nan"), device=dev).to(odt)
            d.out_raw = self.raw.data_ptr()
        if want_act:
            self.act = torch.full((B, Ho, Wo, Cout), float("nan"), device=dev).to(odt)
            d.out_act = self.act.data_ptr()
        self.ws = None

    def workspace(self):
        """(bytes, slabs) the library asks for."""
        n, s = C.c_int64(), C.c_int32()
        self.L.check(self.lib.ppn_conv_splitk_workspace(C.byref(self.d), C.byref(n), C.byref(s)), "ppn_conv_splitk_workspace")
        return n.value, s.value

    def attach_workspace(self, nbytes=None):
        nbytes = self.workspace()[0] if nbytes is None else nbytes
        self.ws = torch.full((max(nbytes, 4) // 4,), float("nan"), device="cuda")          # NaN: a slab never written shows
        self.d.splitk_ws, self.d.splitk_ws_bytes = self.ws.data_ptr(), nbytes

    def launch(self):
        rc = self.lib.ppn_conv2d_fused(C.byref(self.d), self.st)
        torch.cuda.synchronize()
        return rc, self.lib.ppn_last_conv_kernel().decode()

    def outputs(self):
        return [None if t is None else t.float().cpu().permute(0, 3, 1, 2).contiguous() for t in (self.raw, self.act)]


def splitk(x, w, dtype, **kw):
    """Run as split-K with a NaN-filled workspace of exactly the requested size -> (raw, act, slabs)."""
    from pytorch_pose_proposal_network_amd import lib as L
    c = Conv(x, w, dtype, flags=L.PPN_CONV_SPLIT_K, **kw)
    slabs = c.workspace()[1]
    c.attach_workspace()
    rc, name = c.launch()
    assert rc == 0, c.lib.ppn_last_error()
    assert "conv_splitk" in name, name
    raw, act = c.outputs()
    return raw, act, slabs


def check(got, want, tol, what):
    assert got is not None and torch.isfinite(got).all(), f"{what}: NaN / inf in the output (a slab never written?)"
    err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-6)
    print(f"{what}: relative error {err:.3g} (tolerance {tol:g})")
    assert err <= tol, (what, err)


# name, B, Cin, Cout, H, W, k, stride, dil, pad, slabs in (f32, 16-bit)
SHAPES = [
    ("3x3_d2_ragged", 1, 128, 200, 9, 11, 3, 1, 2, 2, (3, 3)),     # 36 / 18 K steps: slabs 16+16+4 / 8+8+2; M = 99; Cout tile partial
    ("1x1_cin512", 2, 512, 64, 5, 7, 1, 1, 1, 0, (1, 1)),          # exactly one slab: S = 1
    ("1x1_cin576", 2, 576, 64, 5, 7, 1, 1, 1, 0, (2, 2)),          # last slab of one (16-bit) / two (f32) steps
    ("3x3_s2", 1, 64, 128, 13, 19, 3, 2, 1, 1, (2, 2)),            # the basicblock1 shape class; M = 70
    ("cout_below_64", 1, 64, 40, 6, 6, 3, 1, 1, 1, (2, 2)),        # tap-major packed rows (k_order 0)
    ("two_pixel_tiles", 3, 64, 64, 8, 9, 3, 1, 1, 1, (2, 2)),      # M = 216: two pixel tiles, the second partial
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", SHAPES, ids=[c[0] for c in SHAPES])
def test_parity(case, dtype):
    name, B, Cin, Cout, H, W, k, s, dl, p, want_slabs = case
    x, w = q(rnd(B, Cin, H, W, seed=1), dtype), q(rnd(Cout, Cin, k, k, seed=2, scale=(Cin * k * k) ** -0.5), dtype)
    raw, _, slabs = splitk(x, w, dtype, stride=s, dil=dl, pad=p)
    assert slabs == want_slabs[0 if dtype == F32 else 1]
    check(raw, ref_conv(x, w, s, dl, p)[0], TOL[dtype], name)


def _epi_inputs(dtype, Cin=128, Cout=72, H=7, W=9):
    x, w = q(rnd(2, Cin, H, W, seed=3), dtype), q(rnd(Cout, Cin, 3, 3, seed=4, scale=(Cin * 9) ** -0.5), dtype)
    vec = lambda seed, base: rnd(Cout, seed=seed, scale=0.25) + base                      # noqa: E731
    return x, w, vec(5, 1.0), vec(6, 0.0), vec(7, 1.0), vec(8, 0.0), q(rnd(2, Cout, H, W, seed=9), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_epilogue_bn_relu(dtype):
    x, w, s1, b1, *_ = _epi_inputs(dtype)
    raw, act, _ = splitk(x, w, dtype, pad=1, s1=s1, b1=b1, act1=1)
    assert act is None
    check(raw, ref_conv(x, w, 1, 1, 1, s1, b1, 1)[0], TOL[dtype], "conv+BN+ReLU")


@pytest.mark.parametrize("dtype", DTYPES)
def test_epilogue_residual_and_second_output(dtype):
    x, w, _, _, s2, b2, res = _epi_inputs(dtype)
    raw, act, _ = splitk(x, w, dtype, pad=1, residual=res, s2=s2, b2=b2, act2=1, want_act=True)
    y, u = ref_conv(x, w, 1, 1, 1, residual=res, s2=s2, b2=b2, act2=1)
    check(raw, y, TOL[dtype], "residual raw")
    check(act, u, TOL[dtype], "second pre-activation output")
    raw2, act2, _ = splitk(x, w, dtype, pad=1, residual=res, s2=s2, b2=b2, act2=1, want_raw=False, want_act=True)
    assert raw2 is None and torch.equal(act2, act)


@pytest.mark.parametrize("dtype", DTYPES)
def test_epilogue_bias_lrelu(dtype):
    x, w, _, b1, *_ = _epi_inputs(dtype)
    raw, _, _ = splitk(x, w, dtype, pad=1, b1=b1, act1=2)
    check(raw, ref_conv(x, w, 1, 1, 1, None, b1, 2)[0], TOL[dtype], "bias + LeakyReLU")


def test_out_bf16_store():
    """A PPN_F16 launch that stores bf16 (PPN_CONV_OUT_BF16): half accumulation error + one bf16 rounding of the result."""
    x, w, s1, b1, s2, b2, _ = _epi_inputs(F16)
    raw, act, _ = splitk(x, w, F16, pad=1, s1=s1, b1=b1, act1=1, s2=s2, b2=b2, act2=1, want_act=True, out_bf16=True)
    y, u = ref_conv(x, w, 1, 1, 1, s1, b1, 1, None, s2, b2, 1)
    tol = F16_TOL + 2.0 ** -8                                    # bf16 keeps 8 significant bits: relative rounding <= 2^-9
    check(raw, y, tol, "bf16 store, raw")
    check(act, u, tol, "bf16 store, act")
    assert torch.equal(raw, raw.to(torch.bfloat16).float())      # the stored values ARE bf16


def test_one_slab_equals_the_one_launch_kernel_on_exact_operands():
    """S = 1 on exactly representable operands (small integers: every product and partial sum is exact in f32): the split-K
    pair and the existing kernel give the same bits, epilogue included."""
    from pytorch_pose_proposal_network_amd import lib as L
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-4, 5, (2, 512, 5, 6), generator=g).float()
    w = torch.randint(-2, 3, (128, 512, 1, 1), generator=g).float()
    s1 = torch.randint(1, 4, (128,), generator=g).float() * 0.5
    b1 = torch.randint(-8, 9, (128,), generator=g).float()
    res = torch.randint(-8, 9, (2, 128, 5, 6), generator=g).float()
    kw = dict(s1=s1, b1=b1, act1=2, residual=res, s2=s1, b2=b1, act2=1, want_act=True)
    for dtype in DTYPES[1:]:                                     # 16-bit: 512 channels are one slab
        raw, act, slabs = splitk(x, w, dtype, **kw)
        assert slabs == 1
        c = Conv(x, w, dtype, **kw)
        rc, name = c.launch()
        assert rc == 0 and "splitk" not in name
        raw0, act0 = c.outputs()
        assert torch.equal(raw, raw0) and torch.equal(act, act0), L.PPN_CONV_SPLIT_K


@pytest.mark.parametrize("dtype", DTYPES)
def test_deterministic_and_batch_independent(dtype):
    x, w = q(rnd(3, 128, 9, 7, seed=21), dtype), q(rnd(72, 128, 3, 3, seed=22, scale=0.03), dtype)
    res = q(rnd(3, 72, 9, 7, seed=23), dtype)
    kw = dict(pad=2, dil=2, b1=rnd(72, seed=24), act1=1)
    a, _, slabs = splitk(x, w, dtype, residual=res, **kw)
    b, _, _ = splitk(x, w, dtype, residual=res, **kw)
    assert slabs == 3 and torch.equal(a, b)
    for i in range(3):
        one, _, _ = splitk(x[i:i + 1], w, dtype, residual=res[i:i + 1], **kw)
        assert torch.equal(one[0], a[i]), f"image {i} alone differs from image {i} in the batch"


def test_workspace_null_or_short_is_invalid():
    from pytorch_pose_proposal_network_amd import lib as L
    x, w = rnd(1, 128, 6, 6, seed=31), rnd(64, 128, 3, 3, seed=32)
    c = Conv(x, w, BF16, pad=1, flags=L.PPN_CONV_SPLIT_K)
    nbytes, slabs = c.workspace()
    assert (nbytes, slabs) == (3 * 36 * 64 * 4, 3)
    canary = c.raw.clone().fill_(7.0)
    c.raw.copy_(canary)
    rc, _ = c.launch()                                           # NULL workspace
    assert rc == INVALID and b"splitk_ws" in c.lib.ppn_last_error()
    c.attach_workspace(nbytes)
    c.d.splitk_ws_bytes = nbytes - 1                             # one byte short
    rc, _ = c.launch()
    assert rc == INVALID and torch.equal(c.raw, canary)
    c.d.splitk_ws_bytes = nbytes
    rc, name = c.launch()
    assert rc == 0 and "conv_splitk" in name and not torch.equal(c.raw, canary)


def test_unsupported_combinations_launch_nothing():
    from pytorch_pose_proposal_network_amd import lib as L
    x, w = rnd(1, 128, 6, 6, seed=41), rnd(64, 128, 3, 3, seed=42)

    def refused(mutate, dtype=BF16):
        c = Conv(x, w, dtype, pad=1, flags=L.PPN_CONV_SPLIT_K)
        c.attach_workspace(1 << 20)
        canary = c.raw.clone().fill_(7.0)
        c.raw.copy_(canary)
        keep = mutate(c)
        rc, _ = c.launch()
        assert rc == UNSUPPORTED, (rc, c.lib.ppn_last_error())
        assert torch.equal(c.raw, canary)
        return keep

    def src2(c):
        c.d.src2, c.d.in2_h, c.d.in2_w, c.d.cin2, c.d.stride2 = c.d.src, 6, 6, 128, 1
        c.d.k_total += 128

    def nchw(c):
        c.d.out_nchw_f32 = 1

    def stats(c):
        part, tiles = torch.zeros(4096, dtype=torch.float64, device="cuda"), C.c_int32(-5)
        c.d.stats_mode, c.d.stats_partial, c.d.stats_tiles = 1, part.data_ptr(), C.pointer(tiles)
        return part, tiles
    refused(src2)
    refused(nchw)
    refused(stats)
    refused(lambda c: None, dtype=X3)


def test_descriptors_without_the_flag_are_untouched():
    """The same descriptor without the flag names the same kernel and gives the same bits before and after split-K launches
    ran in the process (new fields zero, or set and ignored)."""
    from pytorch_pose_proposal_network_amd import lib as L
    x, w = q(rnd(2, 128, 9, 11, seed=51), BF16), q(rnd(200, 128, 3, 3, seed=52, scale=0.03), BF16)
    kw = dict(pad=2, dil=2, b1=rnd(200, seed=53), act1=1)
    c = Conv(x, w, BF16, **kw)
    rc, before_name = c.launch()
    assert rc == 0 and "splitk" not in before_name
    before = c.outputs()[0]
    splitk(x, w, BF16, **kw)
    c2 = Conv(x, w, BF16, **kw)
    c2.attach_workspace(c2.workspace()[0])                       # fields set, flag clear: ignored
    rc, after_name = c2.launch()
    assert rc == 0 and after_name == before_name
    assert torch.equal(c2.outputs()[0], before)
    assert torch.isnan(c2.ws).all()                              # and the workspace was not touched
    assert L.PPN_CONV_SPLIT_K == 16
