"""CPU-only checks of the action model: the exports, the skeleton graph, actions.py's folding against the restatement
tests/stgcn_ref.py in f64, the spec's refusals and the state-dict names, and the stage bounds of tests/stgcn_cases.py -- an f32
evaluation stays inside them, planted faults leave them -- plus the margins the whole-network GPU test relies on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import stgcn_cases as SC
import stgcn_ref as R
from pytorch_pose_proposal_network_amd import actions as AC
from pytorch_pose_proposal_network_amd import config as cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ppn_stgcn_input", "ppn_stgcn_gcn", "ppn_stgcn_tcn", "ppn_stgcn_head")


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


# ---- exports ------------------------------------------------------------------------------------------------------------------
def test_exports_are_declared_bound_and_built(tmp_path):
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "ppn.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    l = lib.load()
    for name in ENTRIES:
        assert f"int {name}(" in header
        assert f" T {name}" in out and name in lib.EXPORTS
        assert getattr(l, name).argtypes is not None and getattr(l, name).restype is C.c_int
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ppn.h"\nint main(){printf("%zu %zu %d %d %d %d %d %d %d\\n", '
           'sizeof(ppn_stgcn_desc), offsetof(ppn_stgcn_desc, residual), PPN_STGCN_MAX_P, PPN_STGCN_MAX_C, PPN_STGCN_MAX_CLASS, '
           'PPN_STGCN_MAX_STREAMS, PPN_STGCN_RES_NONE, PPN_STGCN_RES_IDENTITY, PPN_STGCN_RES_PROJ);return 0;}\n')
    exe = str(tmp_path / "ppn_stgcn_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    assert [int(v) for v in subprocess.check_output([exe]).split()] == [
        C.sizeof(lib.StgcnDesc), lib.StgcnDesc.residual.offset, lib.PPN_STGCN_MAX_P, lib.PPN_STGCN_MAX_C,
        lib.PPN_STGCN_MAX_CLASS, lib.PPN_STGCN_MAX_STREAMS, lib.PPN_STGCN_RES_NONE, lib.PPN_STGCN_RES_IDENTITY,
        lib.PPN_STGCN_RES_PROJ]
    from pytorch_pose_proposal_network_amd import build
    assert ("stgcn.hip", build.NOSLP) in build.SOURCES


def test_the_library_refuses_before_it_launches():
    lib = _lib()
    for what, rc, want in SC.refusals(lib):
        assert rc == want, what


# ---- the graph ----------------------------------------------------------------------------------------------------------------
def test_skeleton_graph_is_the_spatial_partition():
    A = AC.skeleton_graph()
    assert A.shape == (3, 18, 18) and A.dtype == np.float32
    adj = np.eye(18)
    for a, b in cfg.EDGES:
        adj[a, b] = adj[b, a] = 1
    norm = adj / adj.sum(0, keepdims=True)
    assert np.allclose(A.sum(0), norm, atol=1e-7) and np.allclose(A.sum(0).sum(0), 1.0, atol=1e-6)
    assert ((A > 0).sum(0) <= 1).all()                                # the parts do not overlap
    thorax = cfg.KEYPOINT_NAMES.index("thorax")
    assert not A[1][:, thorax].any() and A[2][:, thorax].any()       # nobody is closer to the centre than the centre
    assert (np.diagonal(A[0]) > 0).all() and not np.diagonal(A[1]).any() and not np.diagonal(A[2]).any()
    hop = AC.hop_to(cfg.EDGES, 18, thorax)
    for v, w in zip(*np.nonzero(A[1])):
        assert hop[v] == hop[w] - 1
    for v, w in zip(*np.nonzero(A[2])):
        assert hop[v] == hop[w] + 1
    H = AC.skeleton_graph(SC.HAND_EDGES, 5, 1)
    assert H.shape == (3, 5, 5) and H[1][1, 0] == 0.5 and H[2][0, 1] == 0.25 and H[2][4, 3] == np.float32(1 / 3)


# ---- specs and names ----------------------------------------------------------------------------------------------------------
def test_presets_and_refused_specs():
    paper, tiny = AC.stgcn_spec("paper", 60), AC.stgcn_spec("tiny", 10)
    assert len(paper.blocks) == 10 and paper.blocks[0] == (3, 64, 1, "none") and paper.blocks[4] == (64, 128, 2, "proj")
    assert paper.blocks[7] == (128, 256, 2, "proj") and paper.blocks[9] == (256, 256, 1, "identity")
    assert tiny.blocks == ((3, 16, 1, "none"), (16, 16, 1, "identity"), (16, 32, 2, "proj"), (32, 32, 1, "identity"))
    assert paper.lengths(32) == [32] * 5 + [16] * 3 + [8] * 3 and tiny.lengths(7) == [7, 7, 7, 4, 4]
    assert 1.2e9 < paper.flops(32) < 1.4e9
    bad = [dict(blocks=[(3, 24, 1, "none")]), dict(blocks=[(3, 272, 1, "none")]), dict(blocks=[(8, 16, 1, "none")]),
           dict(blocks=[(3, 16, 3, "none")]), dict(blocks=[(3, 16, 1, "skip")]), dict(blocks=[(3, 16, 1, "identity")]),
           dict(blocks=[(16, 16, 2, "identity")]), dict(blocks=[(3, 16, 1, "none"), (32, 32, 1, "none")]), dict(blocks=[]),
           dict(K=33), dict(K=0), dict(num_class=0), dict(num_class=1025), dict(P=4), dict(kt=3)]
    for kw in bad:
        args = dict(blocks=[(3, 16, 1, "none")], num_class=4, K=18)
        args.update(kw)
        with pytest.raises(ValueError):
            AC.STGCNSpec(**args)
    with pytest.raises(ValueError):
        AC.stgcn_spec("huge", 4)


def test_state_dict_names_and_statistics():
    spec = AC.stgcn_spec("tiny", 10)
    sd = AC.random_state_dict(spec, 3)
    bn = ("weight", "bias", "running_mean", "running_var")
    want = {f"data_bn.{k}": (54,) for k in bn}
    for i, (cin, cout, _, res) in enumerate(spec.blocks):
        b = f"st_gcn_networks.{i}"
        want.update({f"{b}.gcn.conv.weight": (3 * cout, cin, 1, 1), f"{b}.gcn.conv.bias": (3 * cout,),
                     f"{b}.tcn.2.weight": (cout, cout, 9, 1), f"{b}.tcn.2.bias": (cout,), f"edge_importance.{i}": (3, 18, 18)})
        want.update({f"{b}.tcn.{j}.{k}": (cout,) for j in (0, 3) for k in bn})
        if res == "proj":
            want.update({f"{b}.residual.0.weight": (cout, cin, 1, 1), f"{b}.residual.0.bias": (cout,)})
            want.update({f"{b}.residual.1.{k}": (cout,) for k in bn})
    want.update({"fcn.weight": (10, 32, 1, 1), "fcn.bias": (10,)})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    for k, v in sd.items():
        assert v.dtype == torch.float32
        if k.endswith("running_var"):
            assert 0.5 <= float(v.min()) and float(v.max()) <= 2.0
        if k.endswith(("running_mean", "bias")):
            assert float(v.abs().min()) > 0
        if k.startswith("edge_importance"):
            assert float((v - 1).abs().max()) > 0.1
    assert not torch.equal(sd["fcn.weight"], AC.random_state_dict(spec, 4)["fcn.weight"])
    with pytest.raises(KeyError):
        AC.fold(spec, {k: v for k, v in sd.items() if k != "st_gcn_networks.2.residual.1.running_var"})
    with pytest.raises(ValueError):
        AC.fold(spec, dict(sd, **{"fcn.bias": torch.zeros(11)}))


# ---- folding against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("tiny", "paper"))
def test_folded_f64_equals_the_restatement(name):
    net = SC.network(name)
    got = AC.forward_folded(AC.fold(net["spec"], net["sd"]), net["clips"].double().numpy())
    ref = net["ref64"].numpy()
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_packing_puts_every_weight_where_the_kernels_read_it():
    rng = np.random.default_rng(0)
    wg = rng.standard_normal((3, 32, 3))
    pk = AC.pack_gcn(wg).reshape(2, 1, 3, 4, 16, 4)                   # [ct][cc][p][g][col][j]
    for ct, p, g, col, j in ((0, 0, 0, 0, 0), (1, 2, 0, 15, 2), (1, 1, 0, 7, 3), (0, 2, 3, 3, 1)):
        ci = 4 * g + j
        assert pk[ct, 0, p, g, col, j] == np.float32(wg[p, ct * 16 + col, ci] if ci < 3 else 0.0)
    wt, wr = rng.standard_normal((32, 32, 9)), rng.standard_normal((32, 16))
    flat = AC.pack_tcn(wt, wr)
    pt, pr = flat[:2 * 2 * 9 * 256].reshape(2, 2, 9, 4, 16, 4), flat[2 * 2 * 9 * 256:].reshape(2, 1, 4, 16, 4)
    for ct, cc, k, g, col, j in ((0, 0, 0, 0, 0, 0), (1, 1, 8, 3, 15, 3), (1, 0, 4, 2, 5, 1)):
        assert pt[ct, cc, k, g, col, j] == np.float32(wt[ct * 16 + col, cc * 16 + 4 * g + j, k])
        assert pr[ct, 0, g, col, j] == np.float32(wr[ct * 16 + col, 4 * g + j])
    assert AC.pack_tcn(wt, None).size == 2 * 2 * 9 * 256


# ---- the stage bounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.GCN_CASES))
def test_an_f32_evaluation_stays_inside_the_gcn_bound(name):
    c = SC.gcn_case(name)
    got = R.gcn(c["sd"], 0, 3, c["sd"]["A"], c["x"])
    assert got.dtype == torch.float32 and SC.ratio(got, c["ref"], c["bound"]) <= 1.0


@pytest.mark.parametrize("name", sorted(SC.ALL_TCN))
def test_an_f32_evaluation_stays_inside_the_tcn_bound(name):
    c = SC.tcn_case(name)
    cin, cout, stride, residual = c["spec"].blocks[0]
    got = R.tcn(c["sd"], 0, stride, residual, c["u"], c["x"])
    assert got.dtype == torch.float32
    mid = slice(1, 2) if name in SC.WALL_CASES else slice(None)
    assert SC.ratio(got[mid], c["ref"][mid], c["bound"][mid]) <= 1.0


@pytest.mark.parametrize("fault,name", [("transpose", "256_256_t8"), ("importance", "256_256_t8"), ("bias", "256_256_t8"),
                                        ("transpose", "16_16_k5"), ("importance", "3_16_t8"), ("bias", "16_32_t7")])
def test_planted_gcn_faults_leave_the_bound(fault, name):
    c = SC.gcn_case(name)
    assert c["case"].K + 3 * c["case"].cin <= 2304
    got = R.gcn(c["sd"], 0, 3, c["sd"]["A"], c["x"].double(), fault)
    assert SC.ratio(got, c["ref"], c["bound"]) > 1.0


@pytest.mark.parametrize("fault,name", [("tap", "256_256_s1_identity_t8"), ("residual", "256_256_s1_identity_t8"),
                                        ("neighbour", "16_16_s1_identity_t8"), ("residual", "16_32_s2_proj_t9"),
                                        ("stride", "16_16_s2_none_t9"), ("stride", "16_32_s2_proj_t7"),
                                        ("tap", "16_32_s2_proj_t9"),
                                        ("neighbour", "wall_s1"), ("neighbour", "wall_s2"), ("neighbour", "wall_t1")])
def test_planted_tcn_faults_leave_the_bound(fault, name):
    c = SC.tcn_case(name)
    cin, cout, stride, residual = c["spec"].blocks[0]
    assert 9 * cout + (cin if residual == "proj" else 0) <= 2304
    got = R.tcn(c["sd"], 0, stride, residual, c["u"].double(), c["x"].double(), fault)
    mid = slice(1, 2) if name in SC.WALL_CASES else slice(None)
    r = SC.ratio(got[mid], c["ref"][mid], c["bound"][mid])
    assert r > 1.0
    if name in SC.WALL_CASES:
        assert r > 1e20                                               # thirty orders of magnitude, less the weights' size


# ---- what the whole-network GPU test relies on ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("tiny", "paper"))
def test_faults_move_the_logits_far_beyond_the_tolerance_and_the_labels_are_decided(name):
    net = SC.network(name)
    E = net["E"]
    assert 0 < E < 1e-4 * float(net["ref64"].abs().max())
    for fault in ("tap", "neighbour", "transpose", "importance", "bias", "residual", "stride"):
        got = R.forward(net["spec"], net["sd"], net["A"], net["clips"], torch.float64, fault)
        assert float((got - net["ref64"]).abs().max()) > 100 * E, fault
    undecided = int((SC.margins(net["ref64"]) <= 8 * E).sum())
    assert undecided <= 0.05 * SC.N_CLIPS                            # with three clips: none
    assert torch.equal(net["ref32"].argmax(1), net["ref64"].argmax(1))
