"""CPU: what `lowering.lower(..., latency=True)` changes -- the PPN_CONV_SPLIT_K flag of the eligible records and nothing
else -- the ABI of the split-K workspace query, and the slab / workspace arithmetic under the host sanitizers (a stand-alone
program, tools/splitk_partition_check.cpp).  Needs libppn.so for the host-only entry points (built on demand); no GPU."""
import copy
import ctypes as C
import os
import shutil
import subprocess

import pytest

from pytorch_pose_proposal_network_amd import arch as A, config as cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_UNARY, N_EDGES, WIN = 6 * len(cfg.KEYPOINT_NAMES), len(cfg.EDGES), 441


@pytest.fixture(scope="module")
def LW():
    from pytorch_pose_proposal_network_amd import build, lib, lowering
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lowering


def _lower(LW, dtype, batch, fused=False, size=384, **kw):
    mode = LW.resolve_mode(compute_dtype=dtype)
    ops = A.build_program("drn_d_22", N_UNARY + WIN * N_EDGES, fuse_stem=mode.fuse_stem, fuse_shortcut=mode.fuses_shortcut)
    return LW.lower(ops, mode, batch, size, size, True, fused, n_unary=N_UNARY, n_edges=N_EDGES, limb_window=WIN, **kw)


def _flagged(low, L):
    return [l for l in low.launches if l.kind == "conv" and l.scalars["flags"] & L.PPN_CONV_SPLIT_K]


@pytest.mark.parametrize("dtype", ["bfloat16", "float32", "float16"])
@pytest.mark.parametrize("fused", [False, True])
def test_latency_false_is_the_call_without_the_argument(LW, dtype, fused):
    for batch in (1, 32):
        a, b = _lower(LW, dtype, batch, fused), _lower(LW, dtype, batch, fused, latency=False)
        assert a.tensors == b.tensors and a.flops == b.flops and a.launches == b.launches


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("fused", [False, True])
def test_latency_true_only_flags_eligible_records(LW, dtype, fused):
    from pytorch_pose_proposal_network_amd import lib as L
    base, low = _lower(LW, dtype, 1, fused), _lower(LW, dtype, 1, fused, latency=True)
    assert low.tensors == base.tensors and low.flops == base.flops and low.entries == base.entries
    assert len(low.launches) == len(base.launches)                                  # launch counts unchanged
    flagged = _flagged(low, L)
    assert flagged and not _flagged(base, L)
    for a, b in zip(base.launches, low.launches):
        assert (a.kind, a.name, a.flops, a.tensors, a.params) == (b.kind, b.name, b.flops, b.tensors, b.params)
        assert a.params.get("prefetch") == b.params.get("prefetch")                 # the prefetch chain as it was
        if b in flagged:
            assert LW.splitk_eligible(a) and LW.splitk_eligible(b)
            undo = copy.deepcopy(b.scalars)
            undo["flags"] &= ~L.PPN_CONV_SPLIT_K
            assert undo == a.scalars                                                # only the flag differs
        else:
            assert a.scalars == b.scalars and not LW.splitk_eligible(a)
    for l in low.launches:                                                          # who never carries it
        if l.kind != "conv":
            assert "flags" not in l.scalars or not l.scalars["flags"] & L.PPN_CONV_SPLIT_K, l.name
    for l in flagged:
        s = l.scalars
        assert "src2" not in l.tensors and "argmax_keys" not in l.tensors and not s["out_nchw_f32"]
        assert not s.get("limb_edge_pad") and not s.get("m_count") and "downsample" not in l.name
        assert s["k_total"] >= 2 * LW.SPLITK_SLAB and s["cin"] % (32 if s["dtype"] == LW.F32 else 64) == 0
    names = {l.name for l in flagged}
    assert {"basicblock1.conv1", "basicblock2.conv2", "conv2"} <= names              # the 24 x 24 512-wide 3x3 layers
    assert not names & {"conv3", "conv3.unary", "conv3.limbs", "conv1x1_1", "conv1x1_2"}


@pytest.mark.parametrize("dtype", ["bfloat16", "float32", "float16"])
def test_batch_32_carries_no_flag_and_small_batches_split_the_same_layers(LW, dtype):
    from pytorch_pose_proposal_network_amd import lib as L
    assert not _flagged(_lower(LW, dtype, 32, latency=True), L)
    assert _lower(LW, dtype, 32, latency=True).launches == _lower(LW, dtype, 32).launches
    per_batch = {b: [l.name for l in _flagged(_lower(LW, dtype, b, latency=True), L)] for b in (1, 2, 4, 8)}
    # monotone: what is eligible at a batch is eligible at every smaller one ...
    assert set(per_batch[8]) <= set(per_batch[4]) <= set(per_batch[2]) <= set(per_batch[1])
    # ... and the latency batches split the SAME layers, which is what keeps image i's head bit-identical across them
    assert per_batch[1] == per_batch[2] == per_batch[4] and per_batch[1]


def test_eligibility_is_monotone_in_the_batch(LW):
    low = _lower(LW, "bfloat16", 2, latency=True)
    for l in low.launches:
        if l.kind != "conv":
            continue
        for b in (2, 3, 4, 16, 64):
            bigger = copy.deepcopy(l)
            bigger.scalars["batch"] = b
            if LW.splitk_eligible(bigger):
                smaller = copy.deepcopy(l)
                smaller.scalars["batch"] = 1
                assert LW.splitk_eligible(smaller), l.name


def test_workspace_query_matches_the_partition(LW):
    """ppn_conv_splitk_workspace on the flagged records: slabs = ceil(k_total / 512), bytes = slabs * M * cout_pad * 4; a
    record outside the scope is refused with PPN_E_UNSUPPORTED."""
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    low = _lower(LW, "bfloat16", 2, latency=True)
    for l in _flagged(low, L):
        s = l.scalars
        n, slabs = C.c_int64(), C.c_int32()
        assert lib.ppn_conv_splitk_workspace(C.byref(L.ConvDesc(**s)), C.byref(n), C.byref(slabs)) == 0, lib.ppn_last_error()
        assert slabs.value == -(-s["k_total"] // 512) >= 2
        assert n.value == slabs.value * s["batch"] * s["out_h"] * s["out_w"] * s["cout_pad"] * 4
    head = [l for l in low.launches if l.name == "conv3"][0]
    assert lib.ppn_conv_splitk_workspace(C.byref(L.ConvDesc(**head.scalars)), None, None) == -3
    assert lib.ppn_conv_splitk_workspace(None, None, None) == -1
    assert C.sizeof(L.ConvDesc) % 8 == 0 and L.ConvDesc._fields_[-2:] == [("splitk_ws", C.c_void_p), ("splitk_ws_bytes", C.c_int64)]


def test_latency_knob_is_off_by_default(LW):
    import inspect
    from pytorch_pose_proposal_network_amd import model, rt
    if "PPN_LATENCY" not in os.environ:
        assert LW.LATENCY is False
    assert inspect.signature(LW.lower).parameters["latency"].default is False
    assert inspect.signature(model.PoseProposalNet.__init__).parameters["latency"].default is None
    assert "latency" in inspect.signature(rt.network).parameters


def test_partition_arithmetic_under_host_sanitizers(tmp_path):
    """tools/splitk_partition_check.cpp walks every workspace index of the test shapes; built with ASan + UBSan and run as
    a program of its own."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "splitk_partition_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "pytorch_pose_proposal_network_amd", "csrc"),
                    os.path.join(ROOT, "tools", "splitk_partition_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "all ok" in out.stdout, out.stdout + out.stderr
