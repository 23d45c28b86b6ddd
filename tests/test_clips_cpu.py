"""CPU-only checks of the skeleton clips: the rules of ppn_clip_push / ppn_clip_gather (include/ppn.h) as tests/clips_ref.py
restates them, on hand-checked cases; the tracker's restatement chained into the clips'; and the library's argument
validation and struct layout without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import clips_cases as CC
import clips_ref as R
import track_cases as TC
import track_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
M = 4


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def _frame(people, K=2, present=None):
    """One image: people = [(id, x0)]; keypoint k of a person sits at (x0 + k, 2 * x0 + k)."""
    img = CC.blank(M, K)
    img["count"] = len(people)
    for p, (pid, x0) in enumerate(people):
        CC.put(img, p, pid, coords=[(x0 + k, 2 * x0 + k) for k in range(K)], present=present)
    return img


def _play(frames, K=2, T=4, max_gap=2, norm=R.NORM_NONE, with_xy=True):
    """One call of one frame each; returns the steps of clips_cases.run_case."""
    case = dict(cfg=R.make_cfg(K, T, max_gap, norm), streams=1, frames=1, M=M,
                calls=[CC.pack([f], M, K, with_xy=with_xy) for f in frames])
    return CC.ref_steps(case)


def test_an_id_is_held_through_max_gap_and_dropped_beyond():
    seq = [[(5, 10)], [], [], [(5, 40)], [], [], []]
    steps = _play([_frame(p) for p in seq], T=8, max_gap=2)
    ids = [int(st["id"][0, 0]) for _, _, st in steps]
    gaps = [int(st["gap"][0, 0]) for _, _, st in steps]
    lens = [int(st["len"][0, 0]) for _, _, st in steps]
    assert ids == [5, 5, 5, 5, 5, 5, 0]                             # a gap of 2 is survived, twice; the third miss frees
    assert gaps == [0, 1, 2, 0, 1, 2, 0] and lens == [1, 2, 3, 4, 5, 6, 0]
    assert [int(row[0, 0]) for row, _, _ in steps] == [0, -1, -1, 0, -1, -1, -1]
    _, (x, out_id, out_len), st = steps[5]
    assert out_id[0, 0] == 5 and out_len[0, 0] == 6 and st["pos"][0] == 6
    assert x[0, 0, 0, :, 0].tolist() == [0, 0, 10, 0, 0, 40, 0, 0]                 # padding, frame, two unseen rows, frame, ...
    assert st["mask"][0, 0].tolist() == [3, 0, 0, 3, 0, 0, 0, 0]
    assert st["ref"][0, 0].tolist() == [77, 37, 83, 43]                            # the newest SEEN root box: (y - 3, x - 3, ..)
    _, (x, out_id, out_len), st = steps[6]
    assert not x.any() and not out_id.any() and not out_len.any()
    assert st["ring"][0, 0, 3, 0, 0] == 40 and st["ref"][0, 0, 0] == 77             # a freed slot keeps its bytes


def test_a_slot_freed_in_a_frame_is_retaken_in_the_same_frame():
    steps = _play([_frame([(5, 10), (6, 20)]), _frame([(6, 21), (9, 30)]), _frame([(9, 31), (6, 22), (4, 50)])], max_gap=0)
    row, _, st = steps[0]
    assert row[0].tolist() == [0, 1, -1, -1] and st["id"][0, :3].tolist() == [5, 6, 0]
    row, (x, out_id, out_len), st = steps[1]
    assert row[0].tolist() == [1, 0, -1, -1]                        # 6 is seen in slot 1; 9 takes slot 0, freed by 5 just now
    assert st["id"][0, :3].tolist() == [9, 6, 0] and st["len"][0, :3].tolist() == [1, 2, 0] and st["gap"][0, :3].tolist() == [0] * 3
    assert x[0, 0, 0, :, 0].tolist() == [0, 0, 0, 30]               # 5's frame lies before the clip's first: it is padding
    assert x[0, 1, 0, :, 0].tolist() == [0, 0, 20, 21]
    assert st["ring"][0, 0, 0, 0, 0] == 10 and st["ring"][0, 0, 1, 0, 0] == 30      # 5's bytes stay; len guards them
    row, _, st = steps[2]
    assert row[0].tolist() == [0, 1, 2, -1] and st["id"][0, :4].tolist() == [9, 6, 4, 0] and st["flags"][0] == 0


def test_left_padding_order_and_ring_wrap():
    steps = _play([_frame([(5, 10 * (t + 1))], K=3, present={0, 2}) for t in range(6)], K=3, T=4)
    for t, (row, (x, out_id, out_len), st) in enumerate(steps):
        n = min(t + 1, 4)
        assert st["pos"][0] == (t + 1) % 4 and out_len[0, 0] == n
        want = [0] * (4 - n) + [10 * (u + 1) for u in range(t + 1 - n, t + 1)]
        assert x[0, 0, 0, :, 0].tolist() == want, t                                 # chronological, newest last, zeros first
        assert x[0, 0, 1, :, 2].tolist() == [2 * v + 2 if v else 0 for v in want]
        assert x[0, 0, 2, :, 2].tolist() == [F(0.52) if v else 0 for v in want]
        assert not x[0, 0, :, :, 1].any() and not x[0, 1:].any()                    # the absent keypoint; the free slots
    assert steps[-1][2]["ring"][0, 0, :, 0, 0].tolist() == [50, 60, 30, 40]         # the ring itself has wrapped


def test_root_normalisation_and_absent_keypoints():
    img = _frame([(5, 50)], K=3, present={0, 1})
    img["bbox"][0, 0] = (10, 20, 50, 40)                            # cx = 30, cy = 30, s = max(40, 20)
    img["xy"][0, 2], img["score"][0, 2], img["bbox"][0, 2] = np.nan, 7.0, 1e9      # garbage at the absent keypoint
    for with_xy in (True, False):
        (_, (x, _, _), st), = _play([img], K=3, T=2, norm=R.NORM_ROOT, with_xy=with_xy)
        # keypoint 0: its smoothed centre (50, 100), or the centre of its box (30, 30); keypoint 1: (51, 101) either way
        assert x[0, 0, :, 1, 0].tolist() == ([0.5, 1.75, 0.5] if with_xy else [0, 0, 0.5])
        assert x[0, 0, :, 1, 1].tolist() == [F(21) / F(40), F(71) / F(40), F(0.51)]
        assert not x[0, 0, :, :, 2].any() and not x[0, 0, :, 0].any() and not st["ring"][0, 0, 0, :, 2].any()
    # the degenerate and inverted boxes fall back to s = 1
    (_, (x, _, _), st), = CC.ref_steps(CC.ref_edges())
    for s, scale in enumerate((1.0, 1.0, F(77.7) - F(30), F(33.3) - F(10), F(70.7) - F(10.1))):
        ref, raw = st["ref"][s, 0], st["ring"][s, 0, 1, 0, 1]
        assert raw == F(101.3) and x[s, 0, 0, 1, 1] == F(F(raw - F(F(ref[1] + ref[3]) * F(0.5))) / F(scale)), s


def test_overflow_rows_and_flag():
    steps = CC.ref_steps(CC.crowd70())
    row, _, st = steps[0]
    assert (row[0] >= 0).sum() == 64 and sorted(row[0][row[0] >= 0].tolist()) == list(range(64)) and st["flags"][0] == 1
    ids = CC.crowd70()["calls"][0]["ids"][0]
    assert (row[0][ids >= 565] == -1).all() and (ids >= 565).sum() == 6             # the last six of the 70 found no slot
    row, _, st = steps[1]
    assert (row[0] >= 0).sum() == 64 and st["len"][0].tolist() == [2] * 64
    assert not steps[2][2]["id"].any()
    row, _, st = steps[3]
    assert st["id"][0, :6].tolist() == [566, 567, 568, 569, 570, 0] and row[0, :5].tolist() == [0, 1, 2, 3, 4]


def test_chunking_invariance():
    CC.assert_chunking_invariant(CC.chunking_views(7, CC.run_ref))


def _per_frame(case):
    """The calls of a tracker case cut into calls of one frame per stream (the same video, by chunking invariance)."""
    S, Fr = case["streams"], case["frames"]
    for c in case["calls"]:
        nf = np.full(S, Fr) if c["n_frames"] is None else c["n_frames"]
        for t in range(Fr):
            rows = [s * Fr + t for s in range(S)]
            yield {k: c[k][rows] for k in ("count", "kp_cell", "bbox", "score")}, (nf > t).astype(np.int32)


def test_clips_follow_the_tracker():
    """track_ref chained into clips_ref on the tracker's own cases, max_gap == max_age: after every frame the live ids of
    the clips are the tracker's and the overflow flag is never set.  Outcome of the stronger check: state.id is equal to
    the tracker's state.id BYTE FOR BYTE after every frame of every case below -- the clips age as the tracks do, and
    births take the free slots in the same order (ascending p into ascending slot), so the slot of a clip is the slot of
    its track.  The cases include 70 people in a frame (the tracker overflows, the clips then do not: they see 64 ids),
    more than 256 people, a freed slot reused within a frame, and idle streams."""
    cases = [TC.drift(7), TC.absence(7, 1), TC.absence(7, 3), TC.freed_slot_reused(7), TC.two_want_one(7),
             TC.birth_threshold(7), TC.small_k(7, 0), TC.small_k(7, 2), TC.smoothing(7, 0.5), TC.edge_batch(300),
             TC.chunking(7, "streams")[0]]
    frames = 0
    for n, case in enumerate(cases):
        tcfg, S, K = case["cfg"], case["streams"], case["cfg"]["K"]
        ccfg = R.make_cfg(K, 3, tcfg["max_age"])
        tst, cst = TR.fresh_state(S, K), R.fresh_state(S, K, 3)
        for c, nf in _per_frame(case):
            out = TR.track_update(tcfg, tst, c["count"], c["kp_cell"], c["bbox"], c["score"], S, 1, nf)
            row = R.clip_push(ccfg, cst, c["count"], c["kp_cell"], c["bbox"], c["score"], out["ids"], out["xy"], S, 1, nf)
            for s in range(S):
                assert set(cst["id"][s][cst["id"][s] != 0]) == set(tst["id"][s][tst["id"][s] != 0]), (n, s)
            assert cst["id"].tobytes() == tst["id"].tobytes() and cst["gap"].tobytes() == tst["miss"].tobytes(), n
            assert not cst["flags"].any(), n
            assert ((row >= 0) == (out["ids"] > 0)).all()                           # every tracked person has a row
            frames += 1
    assert frames > 60


def test_library_without_a_gpu(tmp_path):
    lib = _lib()
    l = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    for name in ("ppn_clip_push", "ppn_clip_gather"):
        assert f" T {name}" in out and name in lib.EXPORTS
        assert getattr(l, name).argtypes is not None and getattr(l, name).restype is C.c_int
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ppn.h"\nint main(){printf("%zu %zu %zu %zu %d %d %d %d %d\\n", '
           'sizeof(ppn_clip_cfg), sizeof(ppn_clip_state), offsetof(ppn_clip_cfg, norm), offsetof(ppn_clip_state, flags), '
           'PPN_CLIP_SLOTS, PPN_CLIP_MAX_LEN, PPN_CLIP_NORM_NONE, PPN_CLIP_NORM_ROOT, PPN_CLIP_FLAG_SLOT_OVERFLOW);'
           'return 0;}\n')
    exe = str(tmp_path / "ppn_clip_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    assert [int(v) for v in subprocess.check_output([exe]).split()] == [
        C.sizeof(lib.ClipCfg), C.sizeof(lib.ClipState), lib.ClipCfg.norm.offset, lib.ClipState.flags.offset,
        lib.PPN_CLIP_SLOTS, lib.PPN_CLIP_MAX_LEN, lib.PPN_CLIP_NORM_NONE, lib.PPN_CLIP_NORM_ROOT,
        lib.PPN_CLIP_FLAG_SLOT_OVERFLOW]
    assert (lib.PPN_CLIP_SLOTS, lib.PPN_CLIP_MAX_LEN) == (R.SLOTS, R.MAX_LEN) == (64, 256)
    assert [n for n, _ in lib.ClipState._fields_] == list(R.fresh_state(1, 1, 1))

    # addresses that are never dereferenced: every rejection happens before anything is launched
    good_cfg = dict(K=18, length=32, max_gap=15, norm=lib.PPN_CLIP_NORM_ROOT)
    names = [n for n, _ in lib.ClipState._fields_]
    ptrs = {n: 0x10000000 * (i + 1) for i, n in enumerate(names)}
    ins = dict(count=0x100000000, kp_cell=0x110000000, bbox=0x120000000, score=0x130000000, ids=0x140000000,
               xy=0x150000000, n_frames=0x160000000)
    outs = dict(out_row=0x170000000, out=0x180000000, out_id=0x190000000, out_len=0x1a0000000)

    def push(cfg=None, st=None, streams=1, frames=1, max_humans=7, null_cfg=False, null_st=False, **over):
        c = lib.ClipCfg(**{**good_cfg, **(cfg or {})})
        s = lib.ClipState(**{**ptrs, **(st or {})})
        a = {**ins, **outs, **over}
        return l.ppn_clip_push(None if null_cfg else C.byref(c), None if null_st else C.byref(s), a["count"], a["kp_cell"],
                               a["bbox"], a["score"], a["ids"], a["xy"], streams, frames, max_humans, a["n_frames"],
                               a["out_row"], None)

    def gather(cfg=None, st=None, streams=1, null_cfg=False, null_st=False, **over):
        c = lib.ClipCfg(**{**good_cfg, **(cfg or {})})
        s = lib.ClipState(**{**ptrs, **(st or {})})
        a = {**outs, **over}
        return l.ppn_clip_gather(None if null_cfg else C.byref(c), None if null_st else C.byref(s), streams, a["out"],
                                 a["out_id"], a["out_len"], None)

    bad, unsupported = -1, -3
    for call in (push, gather):
        assert call(null_cfg=True) == bad and b"NULL" in l.ppn_last_error()
        assert call(null_st=True) == bad and b"NULL" in l.ppn_last_error()
        for n in names:
            assert call(st={n: None}) == bad and b"state" in l.ppn_last_error(), n
        for cfg in (dict(K=0), dict(K=lib.PPN_MAX_KP + 1), dict(length=0), dict(length=lib.PPN_CLIP_MAX_LEN + 1),
                    dict(max_gap=-1), dict(norm=2), dict(norm=-1)):
            assert call(cfg=cfg) == bad, cfg
        assert call(streams=0) == bad
    for n in ("count", "kp_cell", "bbox", "score", "ids", "out_row"):
        assert push(**{n: None}) == bad and b"NULL" in l.ppn_last_error(), n
    for n in ("out", "out_id", "out_len"):
        assert gather(**{n: None}) == bad and b"NULL" in l.ppn_last_error(), n
    assert push(frames=0) == bad and push(max_humans=0) == bad
    assert push(max_humans=lib.PPN_MATCH_MAX_PEOPLE + 1) == unsupported and b"max_humans" in l.ppn_last_error()


def test_pose_clips_rejects_bad_arguments_on_the_host():
    from pytorch_pose_proposal_network_amd import clips
    for kw in (dict(streams=0), dict(frames=0), dict(max_humans=0), dict(max_humans=1025), dict(K=33), dict(length=0),
               dict(length=257), dict(max_gap=-1), dict(norm="box")):
        with pytest.raises(ValueError):
            clips.PoseClips(device="cpu", **kw)
    c = clips.PoseClips(streams=2, frames=3, max_humans=5, K=4, length=6, device="cpu")
    assert c.state["ring"].shape == (2, 64, 6, 3, 4) and c.state["mask"].shape == (2, 64, 6) and c.row.shape == (6, 5)
    assert c.x.shape == (2, 64, 3, 6, 4) and c.ids.shape == c.len.shape == (2, 64)
    assert all(int(v.abs().sum()) == 0 for v in c.state.values())           # all zero bytes: fresh
    with pytest.raises(ValueError):
        c.push(None, None)                                                   # the kernels are the only implementation
    with pytest.raises(ValueError):
        c.gather()
    batch = clips.ClipBatch(c.x, c.ids.clone(), c.len.clone())
    batch.ids[1, 3], batch.length[1, 3], batch.ids[1, 4], batch.length[1, 4] = 9, 2, 11, 6
    host = batch.to_host(min_len=3)
    assert host[0] == {} and list(host[1]) == [11] and host[1][11][0].shape == (3, 6, 4) and host[1][11][1] == 6
    assert sorted(batch.to_host()[1]) == [9, 11]
