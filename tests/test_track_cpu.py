"""CPU-only checks of the tracker: the rules of ppn_track_update (include/ppn.h) as tests/track_ref.py restates them, on the
cases of tests/track_cases.py that the GPU tests run through the kernel, and the library's argument validation without a
GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import track_cases as TC
import track_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def _ids(steps, b=None):
    """The ids of every image of every call, in order."""
    rows = [out["ids"][i] for out, _ in steps for i in range(out["ids"].shape[0])]
    return rows if b is None else rows[b]


def test_drifting_people_keep_their_ids():
    steps = TC.run_ref("drift/7", TC.drift(7))
    assert len(steps) == 12
    for out, st in steps:
        assert out["ids"][0, :3].tolist() == [1, 2, 3] and (out["ids"][0, 3:] == -1).all()
        assert out["live"][0] == 3
    assert steps[-1][0]["hits"][0, :3].tolist() == [12, 12, 12]
    assert steps[-1][1]["last_id"][0] == 3 and steps[-1][1]["flags"][0] == 0


def test_absence_up_to_max_age_keeps_the_id():
    for gap in (1, 2):
        (out, st), = TC.run_ref(f"absence{gap}/7", TC.absence(7, gap))
        assert out["ids"][-1, :2].tolist() == [1, 2], gap
        assert out["hits"][-1, :2].tolist() == [3 + gap, 3] and st["last_id"][0] == 2
        assert out["live"].tolist() == [2] * (3 + gap)


def test_absence_beyond_max_age_gives_a_new_id():
    (out, st), = TC.run_ref("absence3/7", TC.absence(7, 3))
    assert out["ids"][-1, :2].tolist() == [1, 3] and out["hits"][-1, :2].tolist() == [6, 1]
    assert out["live"].tolist() == [2, 2, 2, 2, 1, 2] and st["last_id"][0] == 3
    assert st["id"][0, :3].tolist() == [1, 3, 0]                   # the freed slot 1 is taken again, by a new id


def test_tie_and_order_rules():
    (out, st), = TC.run_ref("close_beats_iou/7", TC.close_beats_iou(7))
    assert out["ids"][0, :2].tolist() == [1, 2] and out["ids"][1, 0] == 2           # B's keypoints beat A's box
    assert st["miss"][0, :2].tolist() == [1, 0]
    (out, st), = TC.run_ref("equal_keys/7", TC.equal_keys(7))
    assert out["ids"][0, :2].tolist() == [1, 2] and out["ids"][1, 0] == 1           # equal keys: the lowest slot
    assert st["hits"][0, :2].tolist() == [2, 1]
    (out, st), = TC.run_ref("iou_breaks_ties/7", TC.iou_breaks_ties(7))
    assert out["ids"][0, :2].tolist() == [1, 2] and out["ids"][1, 0] == 2           # equal n_close: the larger iou
    assert st["hits"][0, :2].tolist() == [1, 2]
    (out, st), = TC.run_ref("two_want_one/7", TC.two_want_one(7))
    assert out["ids"][1, :2].tolist() == [1, 2] and out["hits"][1, :2].tolist() == [2, 1]     # the lower p wins
    (out, st), = TC.run_ref("freed_slot_reused/7", TC.freed_slot_reused(7))
    assert out["ids"][0, :2].tolist() == [1, 2] and out["ids"][1, :2].tolist() == [2, 3]
    assert out["ids"][2, :3].tolist() == [2, 3, 4]
    assert st["id"][0, :4].tolist() == [3, 2, 4, 0]                # slot 0, freed in frame 1, was reused in frame 1
    assert st["last_id"][0] == 4                                   # ids are never reused
    ids = np.concatenate(_ids(TC.run_ref("freed_slot_reused/7", None)))
    assert sorted(set(ids[ids > 0])) == [1, 2, 3, 4]


def _centres(call, b, p, K):
    bb = call["bbox"][b, p]
    return np.stack([(bb[:, 1] + bb[:, 3]) * F(0.5), (bb[:, 0] + bb[:, 2]) * F(0.5)], 1).astype(F)


def test_alpha_one_stores_the_new_centre():
    case = TC.smoothing(7, 1.0)
    (out, st), = TC.run_ref("smoothing1/7", case)
    new = _centres(case["calls"][0], 3, 0, 18)
    assert st["xy"][0, 0].tobytes() == new.tobytes()
    assert out["xy"][3, 0].tobytes() == new.tobytes()
    assert out["ids"][:, 0].tolist() == [1] * 4 and out["hits"][:, 0].tolist() == [1, 2, 3, 4]


def test_alpha_half_follows_the_formula():
    case = TC.smoothing(7, 0.5)
    (out, st), = TC.run_ref("smoothing.5/7", case)
    c = [_centres(case["calls"][0], t, 0, 18) for t in range(4)]
    xy = c[0].copy()
    for t in (1, 2, 3):
        had = np.ones(18, bool) if t != 2 else np.arange(18) != 5            # keypoint 5 was absent in frame 1
        present = np.ones(18, bool) if t != 1 else np.arange(18) != 5
        smooth = (xy + F(0.5) * (c[t] - xy)).astype(F)
        xy = np.where((present & had)[:, None], smooth, np.where(present[:, None], c[t], xy))
        assert out["xy"][t, 0][present].tobytes() == xy[present].tobytes(), t
        assert (out["xy"][t, 0][~present] == 0).all()
    assert st["xy"][0, 0].tobytes() == xy.tobytes()
    assert not np.array_equal(xy, c[3])                                      # the smoothing did something


def test_chunking_invariance():
    TC.assert_chunking_invariant(TC.chunking_views(7, TC.run_ref))


def test_knife_edges_tell_contraction_from_none():
    case, pts, r2 = TC.gate_sweep()
    (out, st), = TC.run_ref("gate_sweep", case)
    plain = np.array([R.gate_distance(x, y, F(0), F(0)) <= r2 for x, y in pts])
    fused = np.array([R.gate_distance(x, y, F(0), F(0), fused=True) <= r2 for x, y in pts])
    ulps = np.array([(int(R.gate_distance(x, y, F(0), F(0)).view(np.int32)) - int(r2.view(np.int32))) for x, y in pts])
    assert np.abs(ulps).max() <= 4 and (ulps == 0).any() and (ulps > 0).any() and (ulps < 0).any()
    assert np.array_equal(out["ids"][1::2, 0], np.where(plain, 1, 2))       # matched iff the uncontracted gate holds
    flips = int((plain != fused).sum())
    print(f"gate sweep: {len(pts)} points within {np.abs(ulps).max()} ulps of r2, {int(plain.sum())} inside, "
          f"{flips} would flip under a fused dx*dx + dy*dy")
    assert flips > 0
    fused_out = R.track_update(case["cfg"], R.fresh_state(case["streams"], 3), **{k: case["calls"][0][k] for k in
                               ("count", "kp_cell", "bbox", "score")}, streams=case["streams"], frames=2, fused=True)
    assert int((fused_out["ids"] != out["ids"]).any(1).sum()) == flips               # each flip changes one image's ids

    case, boxes = TC.iou_sweep()
    (out, st), = TC.run_ref("iou_sweep", case)
    thr = F(TC.IOU_THR)
    exact = np.array([R.iou(a, R.area(a), b, R.area(b)) >= thr for a, b in boxes])
    recip = []
    for a, b in boxes:                                              # a divide done as a multiplication by the reciprocal
        inter = R.area(a)
        recip.append(F(inter * F(F(1) / F(F(R.area(a) + R.area(b)) - inter))) >= thr)
    assert np.array_equal(out["ids"][1::2, 0], np.where(exact, 1, 2))
    assert exact.any() and not exact.all()
    print(f"iou sweep: {len(boxes)} boxes, {int(exact.sum())} at or above the threshold, "
          f"{int((exact != np.array(recip)).sum())} would flip under a reciprocal divide")


def test_birth_threshold_keeps_low_scores_out():
    (out, st), = TC.run_ref("birth_threshold/7", TC.birth_threshold(7))
    assert out["ids"][:, :3].tolist() == [[1, -1, 2]] * 3 and st["last_id"][0] == 2


def test_edge_batch_flags_and_limits():
    """What the edge batch is there for, read off the restatement the GPU tests hold the kernel to."""
    (out, st), = TC.run_ref("edge_batch/300", TC.edge_batch(300))
    assert st["flags"].tolist() == [R.SLOT_OVERFLOW, R.DET_OVERFLOW | R.SLOT_OVERFLOW, 0, 0, 0]
    assert out["live"].tolist() == [0, 64, 64, 64, 64, -1, -1, -1, -1, 4, 4, 4, 3, -1, -1]
    assert (out["ids"][1] > 0).sum() == 64 and (out["ids"][1, :64] > 0).all()       # exactly 64 of the 70 are tracked
    assert (out["ids"][3, 256:] == -1).all() and (out["ids"][4, 256:] == -1).all()  # people past 256 take no part
    assert (out["ids"][4, :256] > 0).sum() == 64                                    # the 64 tracks are found again
    assert out["ids"][9, :5].tolist() == [1, -1, 2, 3, 4]                           # the person without a root
    assert (out["ids"][[5, 6, 7, 8, 13, 14]] == -1).all() and (out["hits"][[5, 6, 7, 8, 13, 14]] == 0).all()
    (out, st), = TC.run_ref("edge_batch/7", TC.edge_batch(7))
    assert st["flags"].tolist() == [0] * 5 and out["live"][:5].tolist() == [0, 7, 7, 7, 7]


def test_library_without_a_gpu():
    lib = _lib()
    l = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    assert " T ppn_track_update" in out and "ppn_track_update" in lib.EXPORTS
    src = ('#include <stdio.h>\n#include "ppn.h"\nint main(){printf("%zu %zu\\n", sizeof(ppn_track_cfg), '
           'sizeof(ppn_track_state));return 0;}\n')
    exe = os.path.join("/tmp", "ppn_track_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    assert [int(v) for v in subprocess.check_output([exe]).split()] == [C.sizeof(lib.TrackCfg), C.sizeof(lib.TrackState)]
    assert (lib.PPN_TRACK_SLOTS, lib.PPN_TRACK_MAX_DET) == (R.SLOTS, R.MAX_DET) == (64, 256)

    # addresses that are never dereferenced: every rejection happens before anything is launched
    good_cfg = dict(K=18, min_close=3, max_age=15, iou_thr=0.3, kp_gate=0.1, birth_thr=0.0, alpha=1.0)
    names = [n for n, _ in lib.TrackState._fields_]
    ptrs = {n: 0x10000000 * (i + 1) for i, n in enumerate(names)}
    ins = dict(count=0x100000000, kp_cell=0x110000000, bbox=0x120000000, score=0x130000000)
    outs = dict(out_id=0x140000000, out_hits=0x150000000, out_xy=0x160000000, out_live=0x170000000)

    def call(cfg=None, st=None, streams=1, frames=1, max_humans=7, null_cfg=False, null_st=False, **over):
        c = lib.TrackCfg(**{**good_cfg, **(cfg or {})})
        s = lib.TrackState(**{**ptrs, **(st or {})})
        a = {**ins, **outs, "n_frames": None, **over}
        return l.ppn_track_update(None if null_cfg else C.byref(c), None if null_st else C.byref(s), a["count"],
                                  a["kp_cell"], a["bbox"], a["score"], streams, frames, max_humans, a["n_frames"],
                                  a["out_id"], a["out_hits"], a["out_xy"], a["out_live"], None)

    bad, unsupported = -1, -3
    assert call(null_cfg=True) == bad and b"NULL" in l.ppn_last_error()
    assert call(null_st=True) == bad and b"NULL" in l.ppn_last_error()
    for n in names:
        assert call(st={n: None}) == bad and b"state" in l.ppn_last_error(), n
    for n in ("count", "kp_cell", "bbox", "score", "out_id", "out_hits", "out_live"):
        assert call(**{n: None}) == bad and b"NULL" in l.ppn_last_error(), n
    for cfg in (dict(K=0), dict(K=lib.PPN_MAX_KP + 1), dict(min_close=0), dict(max_age=-1),
                dict(iou_thr=-0.01), dict(iou_thr=1.01), dict(iou_thr=float("nan")), dict(kp_gate=-0.5),
                dict(kp_gate=float("inf")), dict(birth_thr=float("nan")), dict(birth_thr=float("-inf")),
                dict(alpha=0.0), dict(alpha=1.5), dict(alpha=float("nan"))):
        assert call(cfg=cfg) == bad, cfg
    assert call(streams=0) == bad and call(frames=0) == bad and call(max_humans=0) == bad
    assert call(bbox=ins["bbox"] + 8) == bad and b"aligned" in l.ppn_last_error()
    assert call(max_humans=lib.PPN_MATCH_MAX_PEOPLE + 1) == unsupported and b"max_humans" in l.ppn_last_error()


def test_tracker_rejects_bad_arguments_on_the_host():
    from pytorch_pose_proposal_network_amd import track
    for kw in (dict(streams=0), dict(frames=0), dict(max_humans=0), dict(max_humans=1025), dict(K=33), dict(alpha=0.0),
               dict(iou_thr=2.0), dict(kp_gate=-1.0), dict(min_close=0), dict(max_age=-1), dict(birth_thr=float("nan"))):
        with pytest.raises(ValueError):
            track.Tracker(device="cpu", **kw)
    t = track.Tracker(streams=2, frames=3, max_humans=5, K=4, device="cpu")
    assert t.state["xy"].shape == (2, 64, 4, 2) and t.ids.shape == (6, 5) and t.xy.shape == (6, 5, 4, 2)
    assert all(int(v.abs().sum()) == 0 for v in t.state.values())           # all zero bytes: a fresh tracker
    with pytest.raises(ValueError):
        t.update(None)                                                       # the kernel is the only implementation
