"""CPU-only checks of flip-averaged inference: the mirror tables, the NumPy oracle (tests/tta_ref.py) against the target
encoder and the decode oracle, the library's argument validation without a GPU, and the defaults of the entry points."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import tta_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def test_mirror_tables():
    from pytorch_pose_proposal_network_amd import config as cfg, tta
    kp, ed = tta.mirror_tables()
    assert kp == [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 13, 14, 15, 16, 17] == R.KP_MIRROR
    assert ed == [0, 1, 5, 6, 7, 2, 3, 4, 8, 9, 11, 10, 13, 12, 15, 14, 16] == R.EDGE_MIRROR
    assert all(kp[kp[k]] == k for k in range(cfg.K)) and all(ed[ed[e]] == e for e in range(cfg.E))
    for e, (s, d) in enumerate(cfg.EDGES):                       # the edge table is what its definition says
        assert cfg.EDGES[ed[e]] == [kp[s], kp[d]]
    edges = [e for e in cfg.EDGES_BY_NAME if e != ("pelvis", "right_hip")]
    with pytest.raises(ValueError):
        tta.mirror_tables(cfg.KEYPOINT_NAMES, edges)
    with pytest.raises(ValueError):                              # a keypoint without its partner
        tta.mirror_tables([n for n in cfg.KEYPOINT_NAMES if n != "left_ankle"], [])
    assert tta.mirror_tables(["a", "left_b", "right_b"], [("a", "right_b"), ("a", "left_b")]) == ([0, 2, 1], [1, 0])


def test_oracle_against_the_target_encoder():
    """mirror_head(planted(mirror P)) == planted(P), and the merged pair decodes to the planted people: pins the four
    permutations and the 1 - x independently of merge_ref's use as the kernel's oracle."""
    from oracle import decode_ref as D
    people = R.people_in_distinct_cells()
    a = R.planted(people)
    bm = R.planted([R.mirror_person(p) for p in people])
    delta = a[:R.K]
    assert int(delta.sum()) == 3 * R.K and int(a[6 * R.K:].sum()) == 3 * R.E     # distinct cells, 51 limb ones
    m = R.mirror_head(bm)
    for g in (0, 1, 3, 4, 5):
        assert np.array_equal(m[g * R.K:(g + 1) * R.K], a[g * R.K:(g + 1) * R.K]), g
    assert np.array_equal(m[6 * R.K:], a[6 * R.K:])
    on = delta != 0
    assert np.array_equal(m[2 * R.K:3 * R.K][on], a[2 * R.K:3 * R.K][on])
    assert not np.array_equal(bm, a)                             # the mirrored frame's head is a different head
    unary, keys, head = R.merge_ref(a[None], bm[None])
    exp, got = D.decode_ref(a), D.decode_ref(head[0])
    assert exp["n"] == 3
    assert set(exp) == set(got)
    for k in exp:
        assert np.array_equal(np.asarray(exp[k]), np.asarray(got[k])), k
    # the keys hold the window maximum and its first index
    arg = D.limb_argmax_dense(head[0])
    assert np.array_equal((~keys[0]).astype(np.uint32).astype(np.int32), arg)
    assert np.array_equal((keys[0] >> np.uint64(32)).astype(np.uint32).view(np.float32),
                          head[0, 6 * R.K:].reshape(R.E, 441, 24, 24).max(1))


def test_generators_hold_ties_that_reverse():
    for shape in (R.ODD, R.EVEN, R.VECTOR):
        B, H, W, sH, sW = shape
        a, b = R.dyadic_pair(11, shape)
        _, keys, head = R.merge_ref(a, b, sH, sW)
        win = head[:, 6 * R.K:].reshape(B, R.E, sH * sW, H, W)
        ties = (win == win.max(2, keepdims=True)).sum(2)
        assert (ties > 1).sum() > 50                             # window maxima attained at several s
        first = (~keys).astype(np.uint32).astype(np.int64)
        assert (R.backwards_argmax(a, b, sH, sW) != first).sum() > 20
        assert np.array_equal((a + R.mirror_head(b, sH=sH, sW=sW)) / 2, head)          # exact averages


def test_library_without_a_gpu():
    lib = _lib()
    l = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    assert " T ppn_tta_merge" in out and " T ppn_tta_stage" in out
    assert "ppn_tta_merge" in lib.EXPORTS and "ppn_tta_stage" in lib.EXPORTS
    src = '#include <stdio.h>\n#include "ppn.h"\nint main(){printf("%zu\\n", sizeof(ppn_tta_cfg));return 0;}\n'
    exe = os.path.join("/tmp", "ppn_tta_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    assert int(subprocess.check_output([exe])) == C.sizeof(lib.TtaCfg)

    from pytorch_pose_proposal_network_amd import tta
    cfg = tta.make_cfg((5, 7), (3, 5))
    assert (cfg.K, cfg.E, cfg.sH, cfg.sW, cfg.H, cfg.W) == (18, 17, 5, 3, 5, 7)
    # addresses that are never dereferenced: every rejection happens before anything is launched
    A, Bm, U, KY = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    bad = -1                                                      # PPN_E_INVALID
    assert l.ppn_tta_merge(None, A, Bm, 1, U, KY, None, None) == bad and b"NULL" in l.ppn_last_error()
    for args in ((None, Bm, U, KY), (A, None, U, KY), (A, Bm, None, KY), (A, Bm, U, None)):
        assert l.ppn_tta_merge(C.byref(cfg), args[0], args[1], 1, args[2], args[3], None, None) == bad
        assert b"NULL" in l.ppn_last_error()
    c = tta.make_cfg((5, 7), (3, 5))
    c.kp_mirror[1], c.kp_mirror[2] = 2, 3                         # 1 -> 2 -> 3: not an involution
    assert l.ppn_tta_merge(C.byref(c), A, Bm, 1, U, KY, None, None) == bad and b"involution" in l.ppn_last_error()
    c = tta.make_cfg((5, 7), (3, 5))
    c.edge_mirror[3] = 17                                         # out of range
    assert l.ppn_tta_merge(C.byref(c), A, Bm, 1, U, KY, None, None) == bad and b"edge_mirror" in l.ppn_last_error()
    c.edge_mirror[3] = -1
    assert l.ppn_tta_merge(C.byref(c), A, Bm, 1, U, KY, None, None) == bad
    c = tta.make_cfg((5, 7), (3, 5))
    c.K = lib.PPN_MAX_KP + 1
    assert l.ppn_tta_merge(C.byref(c), A, Bm, 1, U, KY, None, None) == bad
    c.K, c.E = 18, lib.PPN_MAX_EDGES + 1
    assert l.ppn_tta_merge(C.byref(c), A, Bm, 1, U, KY, None, None) == bad
    assert l.ppn_tta_merge(C.byref(cfg), A, Bm, 0, U, KY, None, None) == bad
    # out_head on an input, and overlapping its tail
    assert l.ppn_tta_merge(C.byref(cfg), A, Bm, 1, U, KY, A, None) == bad and b"alias" in l.ppn_last_error()
    assert l.ppn_tta_merge(C.byref(cfg), A, Bm, 1, U, KY, Bm + 64, None) == bad and b"alias" in l.ppn_last_error()

    assert l.ppn_tta_stage(None, U, 4, 7, 3, None) == bad and b"NULL" in l.ppn_last_error()
    assert l.ppn_tta_stage(A, None, 4, 7, 3, None) == bad
    assert l.ppn_tta_stage(A, U, 4, 7, 5, None) == bad and b"elem_bytes" in l.ppn_last_error()
    assert l.ppn_tta_stage(A, U, -1, 7, 4, None) == bad
    assert l.ppn_tta_stage(A, U, 4, 0, 4, None) == bad
    assert l.ppn_tta_stage(A, A + 4 * 7 * 3 - 1, 4, 7, 3, None) == bad and b"overlap" in l.ppn_last_error()
    assert l.ppn_tta_stage(A, A - 2 * 4 * 7 * 3 + 1, 4, 7, 3, None) == bad and b"overlap" in l.ppn_last_error()
    assert l.ppn_tta_stage(A, U, 0, 7, 3, None) == 0             # nothing to do, nothing launched


def test_flip_tta_defaults_to_off():
    from pytorch_pose_proposal_network_amd import rt, validate
    from pytorch_pose_proposal_network_amd.trainer import PPNTrainer
    for fn in (rt.inference, rt.inference_batch, rt.inference_drawn, rt.inference_batch_drawn, validate.Validator.__init__,
               PPNTrainer.validate):
        p = inspect.signature(fn).parameters
        assert "flip_tta" in p and p["flip_tta"].default is False, fn
