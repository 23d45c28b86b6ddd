"""GPU: the split-K convolution (csrc/conv_splitk.hip through ppn_conv2d_fused with PPN_CONV_SPLIT_K) on the cases of
tests/splitk_cases.py, against the f64 reference under forward_cases' derived per-element bound (a launch passes at
ratio = max(err / bound) <= 1), and bit for bit on operands whose sums are exact (tests/test_splitk_edges_cpu.py proves which
planted faults each of the two detectors sees).

Every launch is guarded: both outputs and the workspace each lie between two 4096-byte canary regions, the workspace is exactly
the ws_bytes the library asks for, and outputs and workspace are NaN-filled before the launch.  For every (case, dtype,
epilogue): return code 0, the routed kernel's name, no NaN in an output, ratio <= 1 per output, canaries intact, no NaN left in
the workspace (every element written, dead columns included), and a second launch into the re-filled buffers bit-identical.
Per (case, dtype) each workspace slab is held to the piece of the sum the partition assigns to it; on the exact operands both
outputs equal the once-rounded f64 result; image i alone equals image i in its batch.

`pytest tests/test_splitk_edges_gpu.py -m gpu -s` prints one SPLITK_EDGE line per launch: profiles/splitk_edge_errors.txt."""
import ctypes as C

import pytest
import torch

import forward_cases as FC
import splitk_cases as SK
from test_conv_gpu import GUARD_BYTES, GUARD_PATTERN

pytestmark = pytest.mark.gpu

NAN = float("nan")


class Guarded:
    """One split-K convolution: device operands, descriptor, guarded outputs and workspace.  c: Conv; op: f32 CPU tensors holding
    values of the storage type (NCHW); epi: Epi."""

    def __init__(self, c, op, epi, dtype, out_bf16=False):
        from pytorch_pose_proposal_network_amd import lib as L
        self.L, self.lib, self.c = L, L.load(), c
        dev = torch.device("cuda")
        code = {"f32": L.PPN_F32, "bf16": L.PPN_BF16, "f16": L.PPN_F16}[dtype]
        tdt = FC.DTYPES[dtype]
        Ho, Wo = FC.out_hw(c)
        kstep, _, korder, ktot, _ = L.conv_tiling(code, c.ci, c.co, c.k)
        cpad = SK.cout_pad(c)
        assert ktot == FC.depth(c) and korder == (0 if SK.tap_major(c) else 1)
        self.st = torch.cuda.current_stream().cuda_stream
        wd = op["w"].contiguous().to(dev)
        packed = torch.empty(cpad, ktot, dtype=tdt, device=dev)
        L.check(self.lib.ppn_pack_weight(code, wd.data_ptr(), c.co, c.ci, c.k, cpad, ktot, korder, kstep, packed.data_ptr(),
                                         self.st), "ppn_pack_weight")
        xs = op["x"].permute(0, 2, 3, 1).contiguous().to(dev, tdt)
        self.keep = [wd, packed, xs, torch.zeros(64, device=dev)]
        d = self.d = L.ConvDesc()
        d.dtype, d.batch, d.in_h, d.in_w, d.cin = code, c.B, c.H, c.W, c.ci
        d.out_h, d.out_w, d.cout = Ho, Wo, c.co
        d.ksize, d.stride, d.dilation, d.pad = c.k, c.s, c.dil, c.pad
        d.k_total, d.cout_pad, d.act1, d.act2 = ktot, cpad, epi.act1, epi.act2
        d.src, d.weight, d.zero_page = xs.data_ptr(), packed.data_ptr(), self.keep[3].data_ptr()
        d.flags = L.PPN_CONV_SPLIT_K | (L.PPN_CONV_OUT_BF16 if out_bf16 else 0)

        def dv(t, on):
            if not on:
                return None
            self.keep.append(t.float().contiguous().to(dev))
            return self.keep[-1].data_ptr()
        d.scale1, d.shift1 = dv(op["s1"], epi.s1), dv(op["b1"], epi.b1)
        d.scale2, d.shift2 = dv(op["s2"], epi.s2b2), dv(op["b2"], epi.s2b2)
        if epi.res:
            self.keep.append(op["res"].permute(0, 2, 3, 1).contiguous().to(dev, tdt))
            d.residual = self.keep[-1].data_ptr()
        self.fences = []
        odt = torch.bfloat16 if out_bf16 else tdt
        self.out = {}
        if epi.raw:
            self.out["raw"] = self._guarded((c.B, Ho, Wo, c.co), odt)
            d.out_raw = self.out["raw"].data_ptr()
        if epi.act:
            self.out["act"] = self._guarded((c.B, Ho, Wo, c.co), odt)
            d.out_act = self.out["act"].data_ptr()
        n, s = C.c_int64(), C.c_int32()
        L.check(self.lib.ppn_conv_splitk_workspace(C.byref(d), C.byref(n), C.byref(s)), "ppn_conv_splitk_workspace")
        self.ws_bytes, self.slabs = n.value, s.value
        assert self.ws_bytes == self.slabs * FC.pixels(c) * cpad * 4
        self.ws = self._guarded((self.slabs, FC.pixels(c), cpad), torch.float32)        # exactly ws_bytes long
        d.splitk_ws, d.splitk_ws_bytes = self.ws.data_ptr(), self.ws_bytes
        self.fill()

    def _guarded(self, shape, dt):
        n = torch.Size(shape).numel() * torch.empty(0, dtype=dt).element_size()
        buf = torch.full((n + 2 * GUARD_BYTES,), GUARD_PATTERN, dtype=torch.uint8, device="cuda")
        self.keep.append(buf)
        self.fences.extend([buf[:GUARD_BYTES], buf[GUARD_BYTES + n:]])
        return buf[GUARD_BYTES: GUARD_BYTES + n].view(dt).view(shape)

    def fill(self):
        for t in list(self.out.values()) + [self.ws]:
            t.fill_(NAN)

    def launch(self):
        """-> (return code, kernel name)"""
        rc = self.lib.ppn_conv2d_fused(C.byref(self.d), self.st)
        torch.cuda.synchronize()
        return rc, self.lib.ppn_last_conv_kernel().decode()

    def outputs(self):
        return {k: t.float().cpu().permute(0, 3, 1, 2).contiguous() for k, t in self.out.items()}

    def workspace(self):
        """[S, B, cout_pad, Ho, Wo] f32 CPU"""
        c = self.c
        return self.ws.cpu().view(self.slabs, c.B, *FC.out_hw(c), -1).permute(0, 1, 4, 2, 3).contiguous()

    def intact(self):
        return all(bool((f == GUARD_PATTERN).all()) for f in self.fences)


def run(c, op, epi, dtype, out_bf16=False):
    """Two guarded launches with everything asserted that needs no reference -> (outputs, workspace, slabs)."""
    g = Guarded(c, op, epi, dtype, out_bf16)
    rc, kernel = g.launch()
    assert rc == 0, g.lib.ppn_last_error()
    assert kernel == SK.kernel_name(dtype), kernel
    got, ws = g.outputs(), g.workspace()
    assert set(got) == {k for k, on in (("raw", epi.raw), ("act", epi.act)) if on}
    for k, t in got.items():
        assert t.shape == (c.B, c.co) + FC.out_hw(c)
        assert not torch.isnan(t).any(), "%s: %d elements keep the NaN fill" % (k, int(torch.isnan(t).sum()))
    assert g.intact(), "a canary region around an output or the workspace was written"
    assert ws.numel() * 4 == g.ws_bytes
    assert not torch.isnan(ws).any(), "%d workspace elements were never written" % int(torch.isnan(ws).sum())
    g.fill()
    rc, kernel2 = g.launch()
    assert rc == 0 and kernel2 == kernel
    again = g.outputs()
    for k in got:
        assert torch.equal(got[k], again[k]), "%s: the second launch differs" % k
    assert torch.equal(ws, g.workspace()), "the second launch leaves another workspace"
    assert g.intact()
    return got, ws, g.slabs


def report(name, dtype, en, slabs, got, ref, bound, note=""):
    """Asserts ratio <= 1 per output and returns the launch's SPLITK_EDGE line."""
    parts = []
    for k in sorted(ref):
        r, where = FC.worst(got[k], ref[k], bound[k])
        err = float((got[k].double() - ref[k]).abs().max())
        parts.append("%s max|ref| %.3f err %.3e ratio %.3f" % (k, float(ref[k].abs().max()), err, r))
        assert r <= 1.0, "%s: ratio %.3f at (image, channel, row, column) = %s, got %r, ref %r, bound %.3e" % (
            k, r, where, float(got[k][where]), float(ref[k][where]), float(bound[k][where]))
    return "SPLITK_EDGE %s %s %s%s: %d slabs, %s, workspace fully written, second run bitwise equal" % (
        name, dtype, en, note, slabs, ", ".join(parts))


RUNS = SK.runs()


@pytest.mark.parametrize("name,dtype,en,ob", RUNS, ids=["%s-%s-%s%s" % (n, d, e, "-bf16out" if ob else "") for n, d, e, ob in RUNS])
def test_splitk_edge(name, dtype, en, ob):
    c, want_slabs, _ = SK.CASES[name]
    ref, bound = SK.reference(name, dtype, en, ob)
    got, _, slabs = run(c, SK.operands(name, dtype), FC.EPILOGUES[en], dtype, ob)
    assert slabs == want_slabs[dtype]
    assert set(got) == set(ref)
    if ob:
        assert all(torch.equal(t, t.to(torch.bfloat16).float()) for t in got.values())       # the stored values ARE bf16
    print(report(name, dtype, en, slabs, got, ref, bound, " (bf16 store)" if ob else ""))


PAIRS = [(n, d) for n in SK.CASES for d in SK.DTYPE_NAMES]


@pytest.mark.parametrize("name,dtype", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_each_slab_holds_its_piece_of_the_sum(name, dtype):
    """Slab s of the workspace, columns < co, is within (n_s + 1) u S_s + tiny of the f64 sum over the n_s terms the partition
    assigns to slab s (S_s: the same sum of magnitudes; n_s - 1 additions in any order and, in f32, the products' roundings);
    columns >= co multiply zero weight rows and are exactly 0.  This pins the partition the kernel header's determinism
    claim rests on."""
    c = SK.CASES[name][0]
    op = SK.operands(name, dtype)
    _, ws, slabs = run(c, op, FC.EPILOGUES["plain"], dtype)
    P, Pmag = SK.partials_f64(c, op, dtype)
    terms = [int(m.sum()) for m in SK.slab_terms(c, dtype)]
    assert ws.shape == (slabs, c.B, SK.cout_pad(c)) + FC.out_hw(c) and P.shape[0] == slabs == len(terms)
    assert not ws[:, :, c.co:].any(), "a dead workspace column is not 0"
    worst = 0.0
    for s in range(slabs):
        bound = (terms[s] + 1) * FC.U * Pmag[s] + FC.TINY
        r, where = FC.worst(ws[s, :, : c.co], P[s], bound)
        assert r <= 1.0, "slab %d: ratio %.3f at (image, channel, row, column) = %s, got %r, ref %r, bound %.3e" % (
            s, r, where, float(ws[s, :, : c.co][where]), float(P[s][where]), float(bound[where]))
        worst = max(worst, r)
    print("SPLITK_EDGE %s %s per-slab: %d slabs of %d .. %d terms, worst ratio %.3f, dead columns 0" % (
        name, dtype, slabs, min(terms), max(terms), worst))


EXACT = [(n, d) for n in SK.EXACT_CASES for d in SK.DTYPE_NAMES]


@pytest.mark.parametrize("name,dtype", EXACT, ids=["%s-%s" % p for p in EXACT])
def test_exact_operands_give_the_once_rounded_sum(name, dtype):
    """Small-integer operands: every partial sum is exact in f32 in any order, so both outputs must EQUAL the f64 result
    rounded once to the storage type (as numbers: fmaxf(t, t * 0) may return -0 for +0).  A difference here where the bounded
    runs pass is a lost or doubled term."""
    c = SK.CASES[name][0]
    op, want = SK.exact_case(name)
    for en, epi in SK.EXACT_EPILOGUES.items():
        got, _, slabs = run(c, op, epi, dtype)
        for k in ("raw", "act"):
            w = want[en][dtype][k]
            diff = got[k] != w
            assert not diff.any(), "%s %s: %d of %d elements differ, first at (image, channel, row, column) = %s: got %r, want %r" % (
                en, k, int(diff.sum()), w.numel(), tuple(int(i) for i in diff.nonzero()[0]),
                float(got[k][diff][0]), float(w[diff][0]))
        print("SPLITK_EDGE %s %s exact/%s: %d slabs, max|raw| %.0f, max|act| %.1f, both outputs equal the once-rounded f64 result" % (
            name, dtype, en, slabs, float(want[en][dtype]["raw"].abs().max()), float(want[en][dtype]["act"].abs().max())))


BATCH = [(n, d) for n in SK.BATCH_CASES for d in SK.DTYPE_NAMES]


@pytest.mark.parametrize("name,dtype", BATCH, ids=["%s-%s" % p for p in BATCH])
def test_image_alone_equals_image_in_the_batch(name, dtype):
    c = SK.CASES[name][0]
    op, epi = SK.operands(name, dtype), FC.EPILOGUES["res_dual"]
    whole, _, _ = run(c, op, epi, dtype)
    for i in range(SK.BATCH_CASES[name]):
        one = dict(op, x=op["x"][i: i + 1], res=op["res"][i: i + 1])
        alone, _, _ = run(c._replace(B=1), one, epi, dtype)
        for k in whole:
            assert torch.equal(alone[k][0], whole[k][i]), "%s: image %d alone differs from image %d in the batch" % (k, i, i)
    print("SPLITK_EDGE %s %s batch independence: images 0 .. %d alone bitwise equal to the batch of %d" % (
        name, dtype, SK.BATCH_CASES[name] - 1, c.B))
