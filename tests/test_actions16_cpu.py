"""CPU-only checks of the action model's float16 mode: the exports and refusals of ppn_stgcn16_*, the half packers against
the formulas of include/ppn.h, the stage bounds of tests/stgcn16_cases.py -- an emulation in f32 arithmetic with half storage
(tests/stgcn16_ref.py) stays inside them, planted faults leave them -- and what the whole-network GPU test relies on."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import stgcn16_cases as SC16
import stgcn16_ref as R16
import stgcn_cases as SC
from pytorch_pose_proposal_network_amd import actions as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ppn_stgcn16_input", "ppn_stgcn16_gcn", "ppn_stgcn16_tcn", "ppn_stgcn16_head")


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


# ---- exports and refusals -----------------------------------------------------------------------------------------------------
def test_exports_are_declared_bound_and_built():
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "ppn.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH]).decode()
    l = lib.load()
    for name in ENTRIES:
        assert f"int {name}(" in header
        assert f" T {name}" in out and name in lib.EXPORTS
        assert getattr(l, name).argtypes is not None and getattr(l, name).restype is C.c_int
    from pytorch_pose_proposal_network_amd import build
    assert ("stgcn16.hip", build.NOSLP) in build.SOURCES


def test_the_library_refuses_before_it_launches():
    lib = _lib()
    got = SC16.refusals(lib)
    assert {w for w, _, _ in got} >= {"gcn f32", "gcn bf16", "tcn f32", "tcn bf16", "input f32", "input bf16", "head f32", "head bf16"}
    for what, rc, want in got:
        assert rc == want, what
    for what, rc, want in SC.refusals(lib):                           # the f32 entry points still refuse PPN_F16
        assert rc == want, what


def test_compute_dtypes():
    spec = AC.stgcn_spec("tiny", 10)
    sd = AC.random_state_dict(spec, 3)
    for bad in ("bfloat16", "float64", None):
        with pytest.raises(ValueError):
            AC.ActionModel(spec, sd, 1, 8, device="cpu", compute_dtype=bad)
    m = AC.ActionModel(spec, sd, 1, 8, device="cpu", compute_dtype="float16")
    assert m.x0.dtype == m.u.dtype == m.y[0].dtype == torch.float16 and m.x0.numel() == 64 * 8 * 18 * 4
    assert m.logits.dtype == m.scale.dtype == m.wf.dtype == m.blocks[0].s0.dtype == m.blocks[0].t3.dtype == torch.float32
    assert m.blocks[0].adj.dtype == m.blocks[0].wg.dtype == m.blocks[0].wt.dtype == torch.float16
    assert all(d.dtype == _lib().PPN_F16 for d in m.descs + [m.d_in, m.d_head])
    m32 = AC.ActionModel(spec, sd, 1, 8, device="cpu")
    assert m32.x0.dtype == torch.float32 and m32.x0.numel() == 64 * 8 * 18 * 3 and m32.descs[0].dtype == _lib().PPN_F32
    with pytest.raises(ValueError):                                   # weights of one mode under a descriptor of the other
        AC.launch_gcn(m.descs[0], m32.blocks[0], m.x0, m.n_active, 64, m.u)
    with pytest.raises(ValueError):
        AC.BlockWeights(AC.fold(spec, sd)["blocks"][0], "cpu", "bfloat16")


# ---- packing --------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


@pytest.mark.parametrize("cin,cout", ((3, 16), (16, 32), (48, 16), (64, 64)))
def test_pack_gcn16_by_formula(cin, cout):
    rng = np.random.default_rng(cin * 1000 + cout)
    P = 3
    wg = rng.standard_normal((P, cout, cin)) * 0.3
    pk = AC.pack_gcn16(wg)
    ncc = (cin + 31) // 32
    assert pk.dtype == np.float16 and pk.size == (cout // 16) * ncc * P * 64 * 8
    want = np.zeros(pk.size, np.float16)
    for ct in range(cout // 16):
        for cc in range(ncc):
            for p in range(P):
                for g in range(4):
                    for col in range(16):
                        for j in range(8):
                            ci = cc * 32 + 8 * g + j
                            if ci < cin:
                                want[((((ct * ncc + cc) * P + p) * 64) + g * 16 + col) * 8 + j] = np.float16(wg[p, ct * 16 + col, ci])
    assert _bits(pk).tobytes() == _bits(want).tobytes()
    assert np.count_nonzero(pk) == wg.size                           # zeros exactly in the padding


@pytest.mark.parametrize("cin,cout,proj", ((16, 16, False), (3, 16, True), (16, 32, True), (48, 48, True)))
def test_pack_tcn16_by_formula(cin, cout, proj):
    rng = np.random.default_rng(cin * 1000 + cout + 7)
    wt = rng.standard_normal((cout, cout, 9)) * 0.3
    wr = rng.standard_normal((cout, cin)) * 0.3 if proj else None
    pk = AC.pack_tcn16(wt, wr)
    ncc, nrc = (cout + 31) // 32, (cin + 31) // 32
    n_t = (cout // 16) * ncc * 9 * 64 * 8
    assert pk.dtype == np.float16 and pk.size == n_t + ((cout // 16) * nrc * 64 * 8 if proj else 0)
    want = np.zeros(pk.size, np.float16)
    for ct in range(cout // 16):
        for g in range(4):
            for col in range(16):
                for j in range(8):
                    for cc in range(ncc):
                        ci = cc * 32 + 8 * g + j
                        for k in range(9):
                            if ci < cout:
                                want[((((ct * ncc + cc) * 9 + k) * 64) + g * 16 + col) * 8 + j] = np.float16(wt[ct * 16 + col, ci, k])
                    for rc in range(nrc if proj else 0):
                        ci = rc * 32 + 8 * g + j
                        if ci < cin:
                            want[n_t + (((ct * nrc + rc) * 64) + g * 16 + col) * 8 + j] = np.float16(wr[ct * 16 + col, ci])
    assert _bits(pk).tobytes() == _bits(want).tobytes()
    assert np.count_nonzero(pk) == wt.size + (wr.size if proj else 0)


def test_block_weights_hold_one_rounding_of_the_f64_fold():
    c = SC.gcn_case("16_32_t7")
    b = AC.fold(c["spec"], c["sd"])["blocks"][0]
    w = AC.BlockWeights(b, "cpu", "float16")
    assert _bits(w.adj.numpy()).tobytes() == _bits(b["adj"].astype(np.float16)).tobytes()
    assert _bits(w.wg.numpy()).tobytes() == _bits(AC.pack_gcn16(b["wg"])).tobytes()
    mine = R16.fold_block(c["sd"], 0, 3, c["sd"]["A"].double().numpy(), c["spec"].blocks[0])     # the two folds agree
    for k in ("adj", "wg", "s0", "t0", "wt", "s3", "t3"):
        assert np.abs(mine[k] - b[k]).max() <= 1e-12 * max(1.0, np.abs(b[k]).max()), k
    # a value that rounds differently through f32: 1 + 2^-11 + 2^-30 is above the tie in f64, on it in f32
    v = np.full((1, 16, 16), 1 + 2.0 ** -11 + 2.0 ** -30)
    assert AC.pack_gcn16(v)[0] == np.float16(1 + 2.0 ** -10) and np.float16(np.float32(v[0, 0, 0])) == np.float16(1.0)


# ---- the stage bounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SC.GCN_CASES))
def test_an_emulation_in_f32_stays_inside_the_gcn_bound(name):
    c = SC16.gcn_case(name)
    got = R16.gcn16(c["b"], c["x"], torch.float32)
    r = SC.ratio(got, c["ref"], c["bound"])
    print(f"gcn16 {name}: emulated err / bound = {r:.3f}")
    assert got.dtype == torch.float32 and r <= 1.0


@pytest.mark.parametrize("name", sorted(SC.ALL_TCN))
def test_an_emulation_in_f32_stays_inside_the_tcn_bound(name):
    c = SC16.tcn_case(name)
    got = R16.tcn16(c["b"], c["u"], c["x"], torch.float32)
    m = SC16.mid(name)
    r = SC.ratio(got[m], c["ref"][m], c["bound"][m])
    print(f"tcn16 {name}: emulated err / bound = {r:.3f}")
    assert got.dtype == torch.float32 and r <= 1.0


@pytest.mark.parametrize("fault,name", [("transpose", "256_256_t8"), ("importance", "256_256_t8"), ("bias", "256_256_t8"),
                                        ("transpose", "16_16_k5"), ("importance", "3_16_t8"), ("bias", "16_32_t7")])
def test_planted_gcn_faults_leave_the_bound(fault, name):
    c = SC16.gcn_case(name)
    b = R16.fold_block(c["sd"], 0, 3, c["sd"]["A"].double().numpy(), c["spec"].blocks[0], fault)
    assert SC.ratio(R16.gcn16(b, c["x"], torch.float64, exact=True), c["ref"], c["bound"]) > 1.0


@pytest.mark.parametrize("fault,name", [("tap", "256_256_s1_identity_t8"), ("residual", "256_256_s1_identity_t8"),
                                        ("neighbour", "16_16_s1_identity_t8"), ("residual", "16_32_s2_proj_t9"),
                                        ("stride", "16_16_s2_none_t9"), ("stride", "16_32_s2_proj_t7"),
                                        ("tap", "16_32_s2_proj_t9"),
                                        ("neighbour", "wall_s1"), ("neighbour", "wall_s2"), ("neighbour", "wall_t1")])
def test_planted_tcn_faults_leave_the_bound(fault, name):
    c = SC16.tcn_case(name)
    b = R16.fold_block(c["sd"], 0, 3, c["sd"]["A"].double().numpy(), c["spec"].blocks[0], fault)
    got = R16.tcn16(b, c["u"], c["x"], torch.float64, exact=True, fault=fault)
    m = SC16.mid(name)
    r = SC.ratio(got[m], c["ref"][m], c["bound"][m])
    assert r > 1.0
    if name in SC.WALL_CASES:
        assert r > 1e3                                                # 6.0e4 against a bound of a few 1e-3


def test_the_exact_cases_are_small_integers():
    g, t = SC16.exact_gcn(), SC16.exact_tcn()
    assert SC16.small_integers(g["x"], g["y"], g["ref"]) and SC16.small_integers(t["u"], t["x"], t["ref"])
    assert float(g["ref"].max()) > 8 and float(t["ref"].max()) > 8 and float(g["y"].abs().max()) > 4
    adj = g["b"]["adj"]
    assert set(np.unique(adj)) == {0.0, 0.5, 1.0} and not np.array_equal(adj, adj.transpose(0, 2, 1))
    # the emulation with its roundings is the reference itself: nothing is rounded away
    assert torch.equal(R16.gcn16(g["b"], g["x"], torch.float32).double(), g["ref"])
    assert torch.equal(R16.tcn16(t["b"], t["u"], t["x"], torch.float32).double(), t["ref"])
    assert not torch.equal(R16.tcn16(t["b"], t["u"], t["x"], fault="stride"), t["ref"])
    assert not torch.equal(R16.gcn16(dict(g["b"], adj=adj.transpose(0, 2, 1)), g["x"]), g["ref"])


# ---- what the whole-network GPU test relies on ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("tiny", "paper"))
def test_faults_move_the_logits_far_beyond_the_tolerance_and_the_labels_are_decided(name):
    net = SC16.network(name)
    E16, emu = net["E16"], net["emu64"]
    print(f"{name}: E16 = {E16:.3e}, |emu64 - restatement f64| = {float((emu - net['ref64']).abs().max()):.3e}, "
          f"margins {SC.margins(emu).tolist()}")
    assert 0 < E16 < 1e-3 * float(emu.abs().max())
    for fault in ("tap", "neighbour", "transpose", "importance", "bias", "residual", "stride"):
        got = R16.forward16(net["spec"], net["sd"], net["A"], net["clips"], torch.float64, fault)
        assert float((got - emu).abs().max()) > 100 * E16, fault
    undecided = int((SC.margins(emu) <= 8 * E16).sum())
    assert undecided <= 0.05 * SC.N_CLIPS                            # with three clips: none
    assert torch.equal(emu.argmax(1), net["ref64"].argmax(1)) and torch.equal(net["emu32"].argmax(1), emu.argmax(1))
