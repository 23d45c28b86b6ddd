"""GPU: the forward convolutions (csrc/conv.hip, conv_big.hip, conv64.hip through ppn_conv2d_fused) on the cases of
tests/forward_cases.py, against the f64 reference with the DERIVED per-element bound of that module (a case passes at
ratio = max(err / bound) <= 1; tests/test_forward_edges_cpu.py proves which planted faults the bound sees).

For every (case, dtype, epilogue): the kernel that ran is the recorded one, no NaN fill survives, the canary regions around
the output buffers are intact, ratio <= 1 on each output, and a second launch is bit-identical.  For `many_images` and the
conv64 epilogue sweep in the 16-bit types the launch is repeated with the filter bank kernel switched off: the two kernels
must agree bit for bit (conv64.hip promises it) and each stay within the bound.

`pytest tests/test_forward_edges_gpu.py -m gpu -s` prints one FWD_EDGE line per launch: profiles/forward_edge_errors.txt."""
import pytest
import torch

import forward_cases as FC
from test_conv_gpu import run_conv

pytestmark = pytest.mark.gpu


def _code(dtype):
    from pytorch_pose_proposal_network_amd import lib as L
    return {"f32": L.PPN_F32, "bf16": L.PPN_BF16, "f16": L.PPN_F16}[dtype]


@pytest.fixture
def conv64_switch():
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()

    def set_(on):
        L.check(lib.ppn_set_conv64_enabled(int(on)), "ppn_set_conv64_enabled")
    yield set_
    set_(1)
    L.check(lib.ppn_set_conv_tile_override(0, 0), "ppn_set_conv_tile_override")


def launch(name, dtype, en):
    """One guarded launch -> ({"raw": NCHW f32, "act": ...} of the wanted outputs, kernel name, canaries intact)."""
    c, force, _ = FC.ALL[name]
    op, epi = FC.operands(name, dtype), FC.EPILOGUES[en]
    info = {}
    raw, act, intact = run_conv(
        op["x"], op["w"], _code(dtype), c.s, c.dil, c.pad, s1=op["s1"] if epi.s1 else None, b1=op["b1"] if epi.b1 else None,
        act1=epi.act1, residual=op["res"] if epi.res else None, s2=op["s2"] if epi.s2b2 else None,
        b2=op["b2"] if epi.s2b2 else None, act2=epi.act2, want_raw=epi.raw, want_act=epi.act, info=info,
        ranges=[(0, 0, force)], guard=True)
    out = {k: t for k, t in (("raw", raw), ("act", act)) if t is not None}
    return out, info["kernel"], intact


def check(name, dtype, en, purpose, note=""):
    """Launch twice and assert everything but the conv64 comparison; returns the outputs and the report line's head."""
    c = FC.ALL[name][0]
    ref, bound = FC.reference(name, dtype, en)
    got, kernel, intact = launch(name, dtype, en)
    again, kernel2, intact2 = launch(name, dtype, en)
    assert kernel == kernel2 == FC.kernel_name(purpose, dtype), (kernel, kernel2)
    assert set(got) == set(ref)
    parts = []
    for k in sorted(ref):
        assert got[k].shape == ref[k].shape == (c.B, c.co) + FC.out_hw(c)
        assert not torch.isnan(got[k]).any(), "%s: %d elements keep the NaN fill" % (k, int(torch.isnan(got[k]).sum()))
        r, where = FC.worst(got[k], ref[k], bound[k])
        err = float((got[k].double() - ref[k]).abs().max())
        parts.append("%s max|ref| %.3f err %.3e ratio %.3f" % (k, float(ref[k].abs().max()), err, r))
        assert r <= 1.0, "%s: ratio %.3f at (image, channel, row, column) = %s, got %r, ref %r, bound %.3e" % (
            k, r, where, float(got[k][where]), float(ref[k][where]), float(bound[k][where]))
        assert torch.equal(got[k], again[k]), "%s: the second launch differs" % k
    assert intact and intact2, "a canary region around an output buffer was written"
    tile = "-" if purpose[0] == "conv64" else "%dx%d" % purpose[1:3]
    head = "FWD_EDGE %s %s %s%s: %s, tile %s, %s, second run bitwise equal" % (name, dtype, en, note, kernel, tile, ", ".join(parts))
    return got, head


RUNS = FC.runs()


@pytest.mark.parametrize("name,dtype,en", RUNS, ids=["%s-%s-%s" % r for r in RUNS])
def test_forward_edge(conv64_switch, name, dtype, en):
    _, head = check(name, dtype, en, FC.ALL[name][2][dtype])
    print(head)


OFF_RUNS = [(n, d, e) for n in FC.CONV64_OFF for d in ("bf16", "f16")
            for e in (FC.EPILOGUES if n in FC.SWEEP else FC.CASE_EPILOGUES)]


@pytest.mark.parametrize("name,dtype,en", OFF_RUNS, ids=["%s-%s-%s" % r for r in OFF_RUNS])
def test_conv64_equals_the_large_tile_kernel(conv64_switch, name, dtype, en):
    purpose_on = FC.ALL[name][2][dtype]
    assert purpose_on[0] == "conv64"
    on, _ = check(name, dtype, en, purpose_on)
    conv64_switch(0)
    off, head = check(name, dtype, en, FC.CONV64_OFF[name], note=" conv64 off")
    for k in on:
        assert torch.equal(on[k], off[k]), "%s: conv64 and the large-tile kernel differ, max |difference| %.3e" % (
            k, float((on[k] - off[k]).abs().max()))
    print(head + ", conv64 on/off bitwise equal")
