"""CPU-only checks of the re-identification: the rules of ppn_people_descr and ppn_reid_update (include/ppn.h) as
tests/reid_ref.py restates them, on hand-checked cases; the tracker's and the cropper's restatements chained into it; and the
library's argument validation and struct layout without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reid_cases as RC
import reid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC = RC.scenarios()
A, B_, C_ = RC.A, RC.B_, RC.C_


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def _steps(name, M=7):
    return RC.run_ref(RC.single(SC[name], M))


def _pids(steps):
    return [out["pid"][0].tolist() for out, _ in steps]


# ---- the descriptor -------------------------------------------------------------------------------------------------------
def _flat_frame(fmt, h, w, c, pitch=None):
    """One frame of one colour c = (c0, c1, c2) as `pixel` names them."""
    nbytes, pitch, pc, uo, vo = R.layout(fmt, h, w, pitch)
    f = np.zeros(nbytes, np.uint8)
    if fmt == "bgr":
        rows = f.reshape(h, pitch)
        rows[:, 0:3 * w:3], rows[:, 1:3 * w:3], rows[:, 2:3 * w:3] = c[1], c[0], c[2]
    elif fmt == "yuyv":
        rows = f.reshape(h, pitch)
        rows[:, 0:2 * w:2], rows[:, 1:2 * w:4], rows[:, 3:2 * w:4] = c[0], c[1], c[2]
    else:
        f[:h * pitch] = c[0]
        if fmt == "nv12":
            f[uo::2], f[uo + 1::2] = c[1], c[2]
        else:
            f[uo:vo], f[vo:] = c[1], c[2]
    return f


@pytest.mark.parametrize("fmt", ("nv12", "i420", "yuyv", "bgr"))
def test_a_flat_colour_fills_one_bin_per_channel(fmt):
    h, w = 16, 24
    pitch = {"nv12": 32, "i420": 28, "yuyv": 52, "bgr": 75}[fmt]
    c = (200, 100, 190)
    d = R.describe(_flat_frame(fmt, h, w, c, pitch), fmt, h, w, (2, 4, 10, 14), pitch).reshape(3, 3, 8)
    want = (6, 3, 5) if fmt == "bgr" else (6, 2, 7)                  # 200 >> 5, (100 - 64) >> 4 resp. 100 >> 5, ...
    for band in range(3):
        for ch in range(3):
            assert d[band, ch, want[ch]] == 1024 and d[band, ch].sum() == 1024
    assert R.bins("nv12", (0, 0, 255)) == (0, 0, 7) and R.bins("nv12", (255, 63, 192)) == (7, 0, 7)
    assert R.bins("nv12", (31, 64, 79)) == (0, 0, 0) and R.bins("nv12", (32, 80, 191)) == (1, 1, 7)
    assert R.bins("bgr", (31, 32, 255)) == (0, 1, 7)


def test_histograms_sum_to_1024_and_the_samples_stay_inside():
    rng = np.random.default_rng(0)
    h, w = 20, 30
    for fmt in ("nv12", "bgr"):
        nbytes = R.layout(fmt, h, w)[0]
        frame = rng.integers(0, 256, nbytes).astype(np.uint8)
        for rect in ((0, 0, 20, 30), (18, 28, 2, 2), (4, 6, 8, 8)) + (((19, 29, 1, 1),) if fmt == "bgr" else ()):
            assert R.good(rect, 0, fmt, h, w)
            d = R.describe(frame, fmt, h, w, rect).reshape(9, 8)
            assert (d.sum(axis=1) == 1024).all()
    assert (191 * 7) // 192 < 7 and (63 * 5) // 64 < 5               # the largest sample index is inside the rectangle
    for rect, status in (((0, 0, 0, 0), 1), ((0, 0, 4, 4), 2), ((-2, 0, 4, 4), 0), ((0, 0, 22, 4), 0), ((0, 28, 4, 4), 0),
                         ((0, 1, 4, 4), 0), ((1, 0, 4, 4), 0), ((0, 0, 4, 3), 0), ((0, 0, 0, 4), 0)):
        assert not R.good(rect, status, "nv12", h, w), (rect, status)
    assert R.good((1, 0, 3, 4), 0, "yuyv", h, w) and R.good((1, 1, 3, 3), 0, "bgr", h, w)
    d, v = R.people_descr(np.zeros((1, R.layout("nv12", h, w)[0]), np.uint8), "nv12", h, w, [[(0, 1, 4, 4), (0, 0, 4, 4)]],
                          [[0, 0]])
    assert v.tolist() == [[0, 1]] and not d[0, 0].any() and d[0, 1].sum() == R.SIM_MAX


def test_intersection_of_flat_colours():
    assert R.similarity(A, A) == R.SIM_MAX == 9216 and R.similarity(A, B_) == 0 and R.similarity(B_, C_) == 0
    assert R.similarity(A, RC.moved(A, 2764)) == 6452 and RC.moved(A, 2764).reshape(9, 8).sum(axis=1).tolist() == [1024] * 9


# ---- the gallery ----------------------------------------------------------------------------------------------------------
def test_relink_at_the_threshold_and_birth_below_it():
    steps = _steps("relink_at_thr")
    assert _pids(steps) == [[1] + [-1] * 6, [-1] * 7, [1] + [-1] * 6]
    assert [out["sim"][0, 0] for out, _ in steps] == [-1, -1, RC.THR]
    st = steps[-1][1]
    assert st["tid"][0, 0] == 9 and st["lost"][0, 0] == 0 and st["n"][0, 0] == 2 and st["last_pid"][0] == 1
    assert [int(out["live"][0]) for out, _ in steps] == [1, 1, 1]
    steps = _steps("born_below_thr")
    assert _pids(steps)[-1] == [2] + [-1] * 6 and steps[-1][0]["sim"][0, 0] == -1
    st = steps[-1][1]
    assert st["pid"][0, :3].tolist() == [1, 2, 0] and st["tid"][0, :2].tolist() == [5, 9] and st["lost"][0, :2].tolist() == [2, 0]


def test_the_three_tie_breaks():
    steps = _steps("tie_similarity")                                 # entry 1 is more similar
    assert _pids(steps)[-1][0] == 2 and steps[-1][0]["sim"][0, 0] == 9000
    steps = _steps("tie_lost")                                       # equal similarity: entry 1 has been lost for less
    assert _pids(steps)[-1][0] == 2 and steps[-1][1]["lost"][0, :2].tolist() == [3, 0]
    steps = _steps("tie_index")                                      # equal similarity and lost: the lower index
    assert _pids(steps)[-1][0] == 1 and steps[-1][1]["tid"][0, :2].tolist() == [7, 2]


def test_two_newcomers_compete_for_one_entry():
    steps = _steps("two_want_one")
    out, st = steps[-1]
    assert out["pid"][0, :2].tolist() == [1, 2] and out["sim"][0, :2].tolist() == [5000, -1]
    assert st["tid"][0, :2].tolist() == [7, 8] and st["n"][0, :2].tolist() == [2, 1]


def test_min_lost_and_memory():
    assert _pids(_steps("min_lost_short"))[-1][0] == 2               # lost = min_lost - 1: no candidate
    assert _pids(_steps("min_lost_met"))[-1][0] == 1
    steps = _steps("memory_last")                                    # lost == memory relinks
    assert _pids(steps)[-1][0] == 1 and steps[-2][1]["lost"][0, 0] == 2
    steps = _steps("memory_gone")                                    # freed the frame before
    assert steps[-2][1]["pid"][0, 0] == 0 and int(steps[-2][0]["live"][0]) == 0
    assert _pids(steps)[-1][0] == 2 and steps[-1][1]["pid"][0, :2].tolist() == [2, 0]       # the freed entry is taken again
    steps = _steps("memory_zero")
    assert [int(st["pid"][0, 0]) for _, st in steps] == [1, 0, 2]    # pids are never reused


def test_entries_and_newcomers_without_a_descriptor():
    steps = _steps("no_descr_no_candidate")
    assert steps[0][1]["n"][0, 0] == 0 and _pids(steps)[-1][0] == 2
    steps = _steps("newcomer_without_descr")
    assert _pids(steps)[-1][0] == 2 and steps[-1][1]["n"][0, :2].tolist() == [1, 0]


def test_blend_and_its_rounding():
    d1 = RC.moved(A, 1003)
    steps = _steps("blend_shift0")
    assert [st["descr"][0, 0].tolist() for _, st in steps] == [A.tolist(), d1.tolist(), B_.tolist()]
    steps = _steps("blend_shift2")
    a, b = A.astype(np.int64), d1.astype(np.int64)
    want1 = (a * 3 + b + 2) >> 2
    want2 = (want1 * 3 + B_ + 2) >> 2
    want3 = (want2 * 3 + B_ + 2) >> 2
    assert [st["descr"][0, 0].tolist() for _, st in steps] == [A.tolist(), want1.tolist(), want2.tolist(), want3.tolist()]
    assert want1[0] == 1024 - 28 and want1[1] == 28                  # 112 moved: (3 * 1024 + 912 + 2) >> 2, (112 + 2) >> 2
    assert want1[8 * 4] == 996 and want1[8 * 4 + 1] == 28            # 111 moved: (3 * 1024 + 913 + 2) >> 2, (111 + 2) >> 2
    assert [int(st["n"][0, 0]) for _, st in steps] == [1, 2, 3, 4]
    st = steps[-1][1]
    st["n"][0, 0] = 65535
    case = RC.single(dict(cfg=SC["blend_shift2"]["cfg"], seq=[[(1, A)]]))
    assert RC.run_ref(case, state=st)[-1][1]["n"][0, 0] == 65535     # saturating


def test_a_bound_person_without_a_descriptor_keeps_the_entrys():
    steps = _steps("bound_without_descr")
    assert steps[1][1]["descr"][0, 0].tolist() == A.tolist() and steps[1][1]["n"][0, 0] == 1 and steps[1][1]["lost"][0, 0] == 0
    assert steps[2][1]["n"][0, 0] == 2
    steps = _steps("first_descr_later")
    assert [int(st["n"][0, 0]) for _, st in steps] == [0, 1, 2] and steps[1][1]["descr"][0, 0].tolist() == B_.tolist()


def test_old_track_id_is_forgotten_and_non_participants():
    steps = _steps("old_tid_forgotten")
    assert _pids(steps)[-1][:2] == [1, 2] and steps[-1][1]["tid"][0, :2].tolist() == [7, 1]
    steps = _steps("non_participants")
    assert _pids(steps) == [[-1, -1, 1] + [-1] * 4, [1] + [-1] * 6]
    steps = _steps("three_return")
    assert _pids(steps)[-1][:3] == [3, 1, 2] and steps[-1][0]["sim"][0, :3].tolist() == [9216] * 3


def test_slot_overflow_at_128():
    steps = RC.run_ref(RC.crowd())
    out, st = steps[0]
    assert out["pid"][0, :128].tolist() == list(range(1, 129)) and out["pid"][0, 128:].tolist() == [-1] * 8
    assert st["flags"][0] == R.SLOT_OVERFLOW and out["live"][0] == 128 and st["last_pid"][0] == 128
    assert st["n"][0, :6].tolist() == [0, 1, 0, 1, 0, 0]             # max_rois 4: person 5 has no descriptor
    out, st = steps[2]                                               # the odd entries are freed, 1128 is born into the first
    assert out["pid"][0, 64] == 129 and st["pid"][0, 1] == 129 and out["live"][0] == 65
    out, st = steps[3]                                               # 65 newcomers, 63 free entries
    assert (out["pid"][0, :130] == -1).sum() == 2 and out["pid"][0, 127] == -1 and out["pid"][0, 129] == -1
    assert out["live"][0] == 128 and st["last_pid"][0] == 129 + 63


def test_n_frames_and_untouched_streams():
    seqs = [SC["three_return"]["seq"], RC.video(3, 5)]
    case = RC.as_case(seqs, R.make_cfg(thr=RC.THR), 3, 7)
    assert [None if c["n_frames"] is None else c["n_frames"].tolist() for c in case["calls"]] == [None, [1, 2]]
    st = R.fresh_state(2)
    call = case["calls"][0]
    sentinel = dict(pid=np.full((6, 7), 55, np.int32), sim=np.full((6, 7), 55, np.int32), live=np.full(6, 55, np.int32))
    out = R.reid_update(case["cfg"], st, call["count"], call["ids"], call["descr"], call["valid"], 2, 3, [0, 2], sentinel)
    assert not any(v[0].any() for v in st.values()) and st["pid"][1].any()           # stream 0 keeps every byte
    assert (out["pid"][:3] == -1).all() and (out["sim"][:3] == -1).all() and out["live"].tolist()[:3] == [-1] * 3
    assert out["live"][5] == -1 and (out["pid"][5] == -1).all() and out["live"][4] >= 0 and 55 not in out["pid"]
    out = R.reid_update(case["cfg"], st, call["count"], call["ids"], call["descr"], call["valid"], 2, 3, [-4, 9], None)
    assert not st["pid"][0].any() and out["live"][5] >= 0            # negative: 0; beyond frames: frames


@pytest.mark.parametrize("seed", (1, 2))
def test_cut_invariance(seed):
    """6 frames as one call = 6 calls of one frame = 2 + 4."""
    seqs = [RC.video(seed, 6), RC.video(seed + 10, 6, p_rename=0.4)]
    cfg = R.make_cfg(thr=5000, memory=2, max_rois=4)
    whole = RC.run_ref(RC.as_case(seqs, cfg, 6, 7))
    ones = RC.run_ref(RC.as_case(seqs, cfg, 1, 7))
    split = RC.run_ref(RC.as_case(seqs, cfg, 4, 7, cuts=[(2, 2), (4, 4)]))
    assert len(whole) == 1 and len(ones) == 6 and len(split) == 2
    for k, v in whole[-1][1].items():
        assert v.tobytes() == ones[-1][1][k].tobytes() == split[-1][1][k].tobytes(), k
    for s in range(2):
        for t in range(6):
            for k in ("pid", "sim"):
                w = whole[0][0][k][s * 6 + t]
                assert w.tolist() == ones[t][0][k][s].tolist(), (k, s, t)
                c, tt = (0, t) if t < 2 else (1, t - 2)
                assert w.tolist() == split[c][0][k][s * 4 + tt].tolist(), (k, s, t)
    assert any(out["sim"].max() >= 0 for out, _ in ones) and whole[-1][1]["last_pid"].min() > 5      # relinks and births happen


# ---- tracker -> rectangles -> descriptors -> gallery on the restatements ------------------------------------------------------
def test_a_person_who_returns_keeps_its_pid_but_not_its_track_id():
    ref = RC.walk_ref()
    w, steps = ref["walk"], ref["steps"]
    first, last = w["away"]
    assert last - first + 1 == RC.WALK_MAX_AGE + 3
    tid = {i: [] for i in range(3)}
    pid = {i: [] for i in range(3)}
    for t, step in enumerate(steps):
        for p, i in enumerate(w["who"][t]):
            tid[i].append(int(step["ids"][0, p]))
            pid[i].append(int(step["out"]["pid"][0, p]))
            assert step["valid"][0, p] == 1
        assert step["valid"][0, len(w["who"][t]):].tolist() == [0] * (RC.WALK_R - len(w["who"][t]))
    for i in (0, 1):
        assert len(set(tid[i])) == 1 and len(set(pid[i])) == 1 and len(pid[i]) == w["T"]
    assert len(set(tid[2][:3])) == 1 and len(set(tid[2][3:])) == 1 and tid[2][3] != tid[2][0]       # a NEW track id
    assert tid[2][3] > max(tid[0][0], tid[1][0], tid[2][0])
    assert len(set(pid[2])) == 1 and pid[2][0] > 0                                                  # its OLD pid
    assert sorted((pid[0][0], pid[1][0], pid[2][0])) == [1, 2, 3]
    back = steps[last + 1]
    assert back["out"]["sim"][0, 2] == R.SIM_MAX and back["state"]["last_pid"][0] == 3
    assert steps[last]["state"]["lost"][0].max() == last - first + 1


# ---- the library and the Python object without a GPU --------------------------------------------------------------------
def test_library_without_a_gpu(tmp_path):
    lib = _lib()
    l = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    for name in ("ppn_people_descr", "ppn_reid_update"):
        assert f" T {name}" in out and name in lib.EXPORTS
        assert getattr(l, name).argtypes is not None and getattr(l, name).restype is C.c_int
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ppn.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d\\n", '
           'sizeof(ppn_reid_cfg), sizeof(ppn_reid_state), sizeof(ppn_yuv_surface), offsetof(ppn_reid_cfg, max_rois), '
           'offsetof(ppn_reid_state, descr), offsetof(ppn_reid_state, flags), PPN_DESCR_ROWS, PPN_DESCR_COLS, PPN_DESCR_BANDS, '
           'PPN_DESCR_BINS, PPN_DESCR_LEN, PPN_REID_SLOTS, PPN_REID_SIM_MAX, PPN_REID_FLAG_SLOT_OVERFLOW);return 0;}\n')
    exe = str(tmp_path / "ppn_reid_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    assert [int(v) for v in subprocess.check_output([exe]).split()] == [
        C.sizeof(lib.ReIdCfg), C.sizeof(lib.ReIdState), C.sizeof(lib.YuvSurface), lib.ReIdCfg.max_rois.offset,
        lib.ReIdState.descr.offset, lib.ReIdState.flags.offset, lib.PPN_DESCR_ROWS, lib.PPN_DESCR_COLS, lib.PPN_DESCR_BANDS,
        lib.PPN_DESCR_BINS, lib.PPN_DESCR_LEN, lib.PPN_REID_SLOTS, lib.PPN_REID_SIM_MAX, lib.PPN_REID_FLAG_SLOT_OVERFLOW]
    assert (lib.PPN_DESCR_ROWS, lib.PPN_DESCR_COLS, lib.PPN_DESCR_BANDS, lib.PPN_DESCR_BINS, lib.PPN_DESCR_LEN) == (
        R.ROWS, R.COLS, R.BANDS, R.BINS, R.LEN) == (96, 32, 3, 8, 72)
    assert (lib.PPN_REID_SLOTS, lib.PPN_REID_SIM_MAX, lib.PPN_REID_FLAG_SLOT_OVERFLOW) == (R.SLOTS, R.SIM_MAX, R.SLOT_OVERFLOW)
    assert [n for n, _ in lib.ReIdState._fields_] == list(R.fresh_state(1))
    assert [n for n, _ in lib.ReIdCfg._fields_] == list(R.make_cfg())

    bad, unsupported = -1, -3
    # ---- ppn_people_descr: addresses that are never dereferenced
    good_surf = dict(format=lib.PPN_PIX_NV12, height=16, width=16, pitch=16, pitch_c=16, frame_stride=384, y=0x10000000,
                     u=0x10000100, v=None, matrix=0, full_range=0)
    dargs = dict(roi=0x20000000, status=0x30000000, descr=0x40000000, valid=0x50000000)

    def descr(surf=None, frames=1, max_rois=4, null_surface=False, **over):
        s = lib.YuvSurface(**{**good_surf, **(surf or {})})
        a = {**dargs, **over}
        return l.ppn_people_descr(None if null_surface else C.byref(s), frames, a["roi"], a["status"], max_rois, a["descr"],
                                  a["valid"], None)

    assert descr(null_surface=True) == bad and b"NULL" in l.ppn_last_error()
    for surf in (dict(format=4), dict(format=-1), dict(matrix=2), dict(y=None), dict(u=None), dict(format=lib.PPN_PIX_I420),
                 dict(height=0), dict(width=0), dict(height=16385), dict(width=16386), dict(width=15), dict(height=15),
                 dict(pitch=15), dict(pitch_c=15), dict(frame_stride=255), dict(format=lib.PPN_PIX_YUYV, pitch=31),
                 dict(format=lib.PPN_PIX_BGR24, pitch=47), dict(format=lib.PPN_PIX_BGR24, pitch=48, frame_stride=767)):
        assert descr(surf=surf) == bad, surf
    for n in dargs:
        assert descr(**{n: None}) == bad and b"NULL" in l.ppn_last_error(), n
    assert descr(max_rois=0) == bad and descr(frames=0) == bad and descr(frames=-1) == bad
    assert descr(frames=257, max_rois=256) == bad and descr(frames=65536, max_rois=1) == bad

    # ---- ppn_reid_update
    good_cfg = dict(thr=6452, min_lost=1, memory=300, shift=2, max_rois=4)
    st_names = [n for n, _ in lib.ReIdState._fields_]
    st_ptrs = {n: 0x10000000 * (i + 1) for i, n in enumerate(st_names)}
    args = dict(count=0x100000000, ids=0x110000000, descr=0x120000000, valid=0x130000000, n_frames=0x140000000,
                out_pid=0x150000000, out_sim=0x160000000, out_live=0x170000000)

    def update(cfg=None, st=None, streams=1, frames=1, max_humans=7, null=(), **over):
        c = lib.ReIdCfg(**{**good_cfg, **(cfg or {})})
        s = lib.ReIdState(**{**st_ptrs, **(st or {})})
        a = {**args, **over}
        return l.ppn_reid_update(None if "cfg" in null else C.byref(c), None if "st" in null else C.byref(s), a["count"],
                                 a["ids"], a["descr"], a["valid"], streams, frames, max_humans, a["n_frames"], a["out_pid"],
                                 a["out_sim"], a["out_live"], None)

    for which in ("cfg", "st"):
        assert update(null=(which,)) == bad and b"NULL" in l.ppn_last_error(), which
    for n in st_names:
        assert update(st={n: None}) == bad and b"state" in l.ppn_last_error(), n
    for cfg in (dict(thr=-1), dict(thr=9217), dict(min_lost=0), dict(min_lost=-2), dict(memory=-1), dict(shift=-1), dict(shift=5),
                dict(max_rois=0), dict(max_rois=-3)):
        assert update(cfg=cfg) == bad, cfg
    for n in ("count", "ids", "descr", "valid", "out_pid", "out_sim", "out_live"):
        assert update(**{n: None}) == bad and b"NULL" in l.ppn_last_error(), n
    assert update(streams=0) == bad and update(frames=0) == bad and update(max_humans=0) == bad
    assert update(streams=-1) == bad and update(frames=-2) == bad and update(max_humans=-3) == bad
    assert update(max_humans=lib.PPN_MATCH_MAX_PEOPLE + 1) == unsupported and b"max_humans" in l.ppn_last_error()


def test_reid_rejects_bad_arguments_on_the_host():
    from pytorch_pose_proposal_network_amd import reid, rt
    good = dict(streams=2, frames=3, max_humans=5, src_hw=(48, 64), fmt="nv12", device="cpu")
    for kw in (dict(streams=0), dict(frames=0), dict(max_humans=0), dict(max_humans=1025), dict(K=0), dict(K=33),
               dict(max_rois=0), dict(max_rois=10923), dict(fmt="rgb"), dict(mode="head"), dict(matrix="bt2020"),
               dict(src_hw=(47, 64)), dict(src_hw=(48, 63)), dict(src_hw=(0, 64)), dict(src_hw=(16386, 64)),
               dict(coords_hw=(0, 5)), dict(margin=-0.1), dict(margin=float("nan")), dict(min_size=1), dict(sim_thr=-0.1),
               dict(sim_thr=1.1), dict(sim_thr=float("nan")), dict(min_lost=0), dict(memory=-1), dict(blend_shift=5),
               dict(blend_shift=-1)):
        with pytest.raises(ValueError):
            reid.ReId(**{**good, **kw})
    r = reid.ReId(**good, max_rois=4, K=4)
    assert r.pid.shape == r.sim.shape == (6, 5) and r.live.shape == (6,)
    assert r.roi.shape == (6, 4, 4) and r.status.shape == r.valid.shape == (6, 4) and r.descr.shape == (6, 4, 72)
    assert r.descr.element_size() == 2 and r.state["descr"].shape == (2, 128, 72) and r.state["pid"].shape == (2, 128)
    assert all(int(v.abs().sum()) == 0 for v in r.state.values())            # all zero bytes: fresh
    assert r.thr == 6452 and r.cfg.thr == 6452 and r.cfg.max_rois == 4 and r.cfg.memory == 300 and r.cfg.shift == 2
    assert reid.ReId(**good, sim_thr=1.0).thr == 9216 and reid.ReId(**good, sim_thr=0.0).thr == 0
    assert reid.ReId(**good, sim_thr=0.5).thr == 4608 and reid.ReId(**good, sim_thr=0.50001).thr == 4609
    assert r.roi_cfg.aspect == 0.0 and (r.roi_cfg.align_y, r.roi_cfg.align_x) == (2, 2) and r.roi_cfg.mode == 1
    assert reid.ReId(**{**good, "fmt": "bgr", "src_hw": (47, 63)}).roi_cfg.align_x == 1
    assert r.coords_hw == (48, 64) and reid.ReId(**good, coords_hw=(24, 32)).roi_cfg.sy == 2.0
    for call in (lambda: r.update(None, None), lambda: r.describe(None), lambda: r.rects(None), lambda: r.reid(None, None, None)):
        with pytest.raises(ValueError):
            call()                                                           # the kernels are the only implementation
    for s in (-1, 2):
        with pytest.raises(ValueError):
            r.reset(streams=[s])
    r.state["pid"][1, 3] = 9
    r.reset(streams=[1])
    assert r.flags().tolist() == [0, 0] and not r.state["pid"].any() and r.state_to_host()["descr"].dtype == np.uint16
    res = reid.ReIdResult(r.pid, r.sim, r.live, r.descr, r.valid, r.roi, r.status).to_host()
    assert res["descr"].dtype == np.uint16 and res["descr"].shape == (6, 4, 72) and (res["pid"] == -1).all()
    assert res["status"].tolist() == [[1] * 4] * 6 and res["live"].tolist() == [-1] * 6
    from pytorch_pose_proposal_network_amd.track import TrackResult
    tr = TrackResult(ids="i", hits="h", xy="x", live="l", count="c")
    at = r.out.as_tracks(tr)
    assert at.ids is r.pid and (at.hits, at.xy, at.live, at.count) == ("h", "x", "l", "c")
    with pytest.raises(ValueError):
        rt.inference_reid(None, "nv12", (48, 64), None, None, r, flip=True)
