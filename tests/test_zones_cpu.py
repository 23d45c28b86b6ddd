"""CPU-only checks of the zones and counting lines: the rules of ppn_zone_update (include/ppn.h) as tests/zones_ref.py
restates them, on hand-checked cases; the tracker's restatement chained into the zones'; and the library's argument
validation and struct layout without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import track_cases as TC
import track_ref as TR
import zones_cases as ZC
import zones_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SC = ZC.scenarios()


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def _zone0(steps):
    """Per call (occupancy, entered, exited, loitering) of zone 0 in image 0."""
    return [out["zone"][0, 0].tolist() for out, _ in steps]


def _line(steps, l=0):
    return [out["line"][0, l].tolist() for out, _ in steps]


# ---- zones ------------------------------------------------------------------------------------------------------------
def test_enter_stay_leave():
    steps = ZC.ref_steps(SC["enter_stay_leave"])
    assert _zone0(steps) == [[0, 0, 0, 0], [1, 1, 0, 1], [1, 0, 0, 1], [0, 0, 1, 0]]
    assert [int(st["dwell"][0, 0, 0]) for _, st in steps] == [0, 1, 2, 0]
    assert [int(st["inside"][0, 0]) for _, st in steps] == [0, 1, 1, 0]
    assert [out["inside"][0].tolist() for out, _ in steps] == [[0] * 4, [1, 0, 0, 0], [1, 0, 0, 0], [0] * 4]
    assert [out["slot"][0].tolist() for out, _ in steps] == [[0, -1, -1, -1]] * 4
    st = steps[-1][1]
    assert st["zone_total"][0, 0].tolist() == [1, 1] and not st["zone_total"][0, 1:].any() and not st["line_total"].any()
    assert st["last"][0, 0].tolist() == [40, 20] and st["id"][0, :2].tolist() == [5, 0]


def test_born_inside_counts_as_entered():
    steps = ZC.ref_steps(SC["born_inside"])
    assert _zone0(steps) == [[1, 1, 0, 1], [1, 0, 0, 1]]
    assert [int(st["dwell"][0, 0, 0]) for _, st in steps] == [1, 2]


def test_freed_while_inside_counts_as_exited():
    steps = ZC.ref_steps(SC["freed_inside"])                        # max_gap 1: the second unseen frame frees the slot
    assert _zone0(steps) == [[1, 1, 0, 1], [0, 0, 0, 1], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert [int(st["id"][0, 0]) for _, st in steps] == [5, 5, 0, 0]
    assert [int(st["gap"][0, 0]) for _, st in steps] == [0, 1, 0, 0]
    st = steps[2][1]
    assert st["zone_total"][0, 0].tolist() == [1, 1] and not st["inside"].any() and not st["dwell"].any()
    assert st["last"][0, 0].tolist() == [20, 20]                    # a freed slot keeps these bytes


def test_dwell_runs_on_while_unseen_and_loitering_starts_at_the_threshold():
    steps = ZC.ref_steps(SC["dwell_unseen"])                        # loiter 3, max_gap 2
    assert [int(st["dwell"][0, 0, 0]) for _, st in steps] == [1, 2, 3, 4]
    assert _zone0(steps) == [[1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 1]]
    assert steps[-1][1]["zone_total"][0, 0].tolist() == [1, 0]


def test_dwell_saturates():
    case = ZC.play([[(5, 20, 20)], [(5, 20, 20)], []], zones=[ZC.SQUARE])
    (_, st), = ZC.ref_steps(dict(case, calls=case["calls"][:1]))
    st["dwell"][0, 0, 0] = 2 ** 31 - 2
    steps = ZC.ref_steps(dict(case, calls=case["calls"][1:]), state=st)
    assert [int(s["dwell"][0, 0, 0]) for _, s in steps] == [2 ** 31 - 1, 2 ** 31 - 1]               # seen, then unseen


# ---- lines ------------------------------------------------------------------------------------------------------------
def test_crossing_forward_then_backward():
    steps = ZC.ref_steps(SC["forward_backward"])
    assert _line(steps) == [[0, 0], [1, 0], [0, 1]]
    assert steps[-1][1]["line_total"][0, 0].tolist() == [1, 1] and not steps[-1][1]["line_total"][0, 1:].any()


def test_crossing_is_evaluated_across_a_gap_of_unseen_frames():
    assert _line(ZC.ref_steps(SC["across_gap"])) == [[0, 0], [0, 0], [0, 0], [1, 0]]


def test_two_lines_in_one_step():
    steps = ZC.ref_steps(SC["two_lines"])
    assert _line(steps, 0) == [[0, 0], [1, 0]] and _line(steps, 1) == [[0, 0], [1, 0]]


def test_segment_ends():
    assert _line(ZC.ref_steps(SC["past_the_end"])) == [[0, 0], [0, 0]]              # beyond B: the sides differ, no count
    steps = ZC.ref_steps(SC["through_endpoints"])                                   # through B (e1 == 0) and through A (e0 == 0)
    assert _line(steps) == [[0, 0], [2, 0]]
    assert R.crossing(ZC.LINE, (F(100), F(40)), (F(100), F(60))) == 1 and R.crossing(ZC.LINE, (F(0), F(60)), (F(0), F(40))) == -1
    assert R.crossing(ZC.LINE, (F(100.5), F(40)), (F(100.5), F(60))) == 0


def test_on_the_line_is_the_non_negative_side():
    # arriving on the line from the negative side is the crossing; leaving it to the positive side is none, and back again
    assert _line(ZC.ref_steps(SC["on_the_line"])) == [[0, 0], [1, 0], [0, 0], [0, 0], [0, 1]]
    assert R.side(ZC.LINE, F(20), F(50)) and not R.side(ZC.LINE, F(20), np.nextafter(F(50), F(0)))
    assert _line(ZC.ref_steps(SC["along_the_line"])) == [[0, 0]] * 3


def test_a_zero_length_line_is_never_crossed():
    assert _line(ZC.ref_steps(SC["zero_length"])) == [[0, 0]] * 4


# ---- the polygon test --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_xy", (True, False))
@pytest.mark.parametrize("anchor", (R.ANCHOR_CENTER, R.ANCHOR_BOTTOM))
def test_polygon_knife_edges(anchor, with_xy):
    """Anchors on vertices, on horizontal, left and right edges, rays through vertices, a concave 8-gon, both windings, a
    collinear polygon: the sets worked out by hand."""
    (out, st), = ZC.ref_steps(ZC.knife_edges(with_xy, anchor))
    for z, name in enumerate(("square", "square", "diamond", "u", "u", "collinear")):
        got = {pt for p, pt in enumerate(ZC.KNIFE_POINTS) if out["inside"][0, p] >> z & 1}
        assert got == ZC.KNIFE_INSIDE[name], (z, name)
        assert out["zone"][0, z].tolist() == [len(got), len(got), 0, len(got)]
    assert not out["zone"][0, 6:].any() and out["slot"][0].tolist() == list(range(len(ZC.KNIFE_POINTS)))


def test_anchors():
    for name in ("bottom_anchor", "box_centres"):
        steps = ZC.ref_steps(SC[name])
        assert _zone0(steps) == [[0, 0, 0, 0], [1, 1, 0, 1], [0, 0, 1, 0]], name
        assert steps[1][1]["last"][0, 0].tolist() == [20, 20]
    box = np.array((10, 20, 31, 41), F)
    assert R.anchor_of(R.make_cfg(anchor=R.ANCHOR_CENTER), box, None) == (30.5, 20.5)
    assert R.anchor_of(R.make_cfg(anchor=R.ANCHOR_BOTTOM), box, None) == (30.5, 31)
    assert R.anchor_of(R.make_cfg(anchor=R.ANCHOR_CENTER), box, (7, 8)) == (7, 8)
    assert R.anchor_of(R.make_cfg(anchor=R.ANCHOR_BOTTOM), box, (7, 8)) == (30.5, 31)               # xy is the CENTRE: not used


@pytest.mark.parametrize("with_xy", (True, False))
def test_people_that_take_no_part(with_xy):
    steps = ZC.ref_steps(ZC.bystanders(with_xy))
    out, st = steps[0]                                              # count 6: NaN, inf, absent root, ids 0 and -4, id 14
    assert out["inside"][0].tolist() == [0, 0, 0, 1, 1, 1, 0, 0] and out["slot"][0].tolist() == [-1] * 5 + [0, -1, -1]
    assert out["zone"][0, 0].tolist() == [3, 1, 0, 1] and st["id"][0, :2].tolist() == [14, 0]
    out, st = steps[1]                                              # count -3: nobody; max_gap 0 frees 14
    assert not out["inside"].any() and (out["slot"] == -1).all() and out["zone"][0, 0].tolist() == [0, 0, 1, 0]
    out, st = steps[2]                                              # count M + 5: all 8 rows
    assert out["inside"][0].tolist() == [0, 0, 0, 1, 1, 1, 1, 1] and out["slot"][0].tolist() == [-1] * 5 + [0, 1, 2]
    assert out["zone"][0, 0].tolist() == [5, 3, 0, 3] and st["zone_total"][0, 0].tolist() == [4, 1]


# ---- whole cases -------------------------------------------------------------------------------------------------------
def test_invariant_entered_minus_exited_is_slots_inside():
    """ref_steps asserts it after every call of every case; the cases here are cut into calls of one frame."""
    n = 0
    for name, case in list(SC.items()) + [("geometry", ZC.geometry(7, 3, 16, 16)), ("crowd", ZC.geometry(300, 2, 16, 1))] + [
            (f"chunk{i}", c) for i, c in enumerate(ZC.chunking(7, "frames"))]:
        assert case["frames"] == 1
        steps = ZC.run_ref("inv/" + name, case)
        n += len(steps)
        ZC.assert_invariant(steps[-1][1])
    totals = ZC.run_ref("inv/geometry", ZC.geometry(7, 3, 16, 16))[-1][1]
    assert n > 60 and totals["zone_total"][0, :, 1].any() and totals["line_total"][0].any()
    broken = R.copy_state(totals)
    broken["zone_total"][0, 3, 0] += 1
    with pytest.raises(AssertionError):
        ZC.assert_invariant(broken)


def test_chunking_invariance():
    """The same videos as calls of 1 frame, of 3 frames, of 12 frames and with ragged n_frames: the same state bytes."""
    ZC.assert_chunking_invariant(ZC.chunking_views(7, ZC.run_ref))


def test_slot_overflow_sets_the_flag():
    steps = ZC.run_ref("frames3/300", ZC.frames3(300))
    assert steps[-1][1]["flags"].tolist() == [0, 1, 0] and (steps[1][0]["slot"][3] >= 0).sum() == 64   # stream 1, its frame 0
    assert ZC.run_ref("frames3/7", ZC.frames3(7))[-1][1]["flags"].tolist() == [0, 0, 0]


def test_clamped_tables():
    case = ZC.clamped()
    steps = ZC.run_ref("clamped", case)
    zone = np.concatenate([out["zone"] for out, _ in steps]).reshape(len(steps), 3, 16, 4)
    assert zone[:, 0, :, 0].any() and not zone[:, 0, [2, 3, 4, 9]].any()            # stream 0: zones of 2, 0, -5 and 1 vertices are empty
    assert zone[:, 1, :5].any() and not zone[:, 1, 5:].any() and not zone[:, 2].any()               # zone_n 5 and -3
    line = np.concatenate([out["line"] for out, _ in steps]).reshape(len(steps), 3, 16, 2)
    assert not line[:, 1].any() and not line[:, 2, 2:].any()                        # line_n -1 and 2


def _per_frame(case):
    """The calls of a tracker case cut into calls of one frame per stream (the same video, by chunking invariance)."""
    S, Fr = case["streams"], case["frames"]
    for c in case["calls"]:
        nf = np.full(S, Fr) if c["n_frames"] is None else c["n_frames"]
        for t in range(Fr):
            rows = [s * Fr + t for s in range(S)]
            yield {k: c[k][rows] for k in ("count", "kp_cell", "bbox", "score")}, (nf > t).astype(np.int32)


def test_zones_follow_the_tracker():
    """track_ref chained into zones_ref on the tracker's own cases, max_gap == max_age: after every frame the live ids of
    the zones are the tracker's and the overflow flag is never set.  Outcome of the stronger check: state.id is equal to
    the tracker's state.id BYTE FOR BYTE after every frame of every case below, and gap to its miss -- as was found for
    the clips: a tracked person has a present root and, in these cases, a finite anchor, so it is valid; the slots age as
    the tracks do, and births take the free slots in the same order.  (A tracked person with a non-finite box would take no
    part here, and the two would part.)  The invariant entered - exited == slots inside holds after every frame."""
    cases = [TC.drift(7), TC.absence(7, 1), TC.absence(7, 3), TC.freed_slot_reused(7), TC.two_want_one(7),
             TC.birth_threshold(7), TC.small_k(7, 0), TC.small_k(7, 2), TC.smoothing(7, 0.5), TC.edge_batch(300),
             TC.chunking(7, "streams")[0]]
    zones = [[(40, 40), (200, 40), (200, 250), (40, 250)], [(100, 0), (400, 0), (250, 300)]]
    lines = [(0, 150, 400, 150), (150, 0, 150, 400)]
    frames = crossings = 0
    for n, case in enumerate(cases):
        tcfg, S, K = case["cfg"], case["streams"], case["cfg"]["K"]
        zcfg = R.make_cfg(K, tcfg["max_age"], R.ANCHOR_CENTER if n % 2 else R.ANCHOR_BOTTOM)
        geom = R.make_geom([zones] * S, [lines] * S)
        tst, zst = TR.fresh_state(S, K), R.fresh_state(S)
        for c, nf in _per_frame(case):
            out = TR.track_update(tcfg, tst, c["count"], c["kp_cell"], c["bbox"], c["score"], S, 1, nf)
            z = R.zone_update(zcfg, geom, zst, c["count"], c["kp_cell"], c["bbox"], out["ids"], out["xy"], S, 1, nf)
            assert zst["id"].tobytes() == tst["id"].tobytes() and zst["gap"].tobytes() == tst["miss"].tobytes(), n
            assert not zst["flags"].any(), n
            assert ((z["slot"] >= 0) == (out["ids"] > 0)).all()                     # every tracked person has a slot
            ZC.assert_invariant(zst)
            frames += 1
        crossings += int(zst["line_total"].sum())
        assert zst["zone_total"].any(), n
    assert frames > 60 and crossings > 0


# ---- the library and the Python object without a GPU --------------------------------------------------------------------
def test_library_without_a_gpu(tmp_path):
    lib = _lib()
    l = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    assert " T ppn_zone_update" in out and "ppn_zone_update" in lib.EXPORTS
    assert l.ppn_zone_update.argtypes is not None and l.ppn_zone_update.restype is C.c_int
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ppn.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d\\n", '
           'sizeof(ppn_zone_cfg), sizeof(ppn_zone_geom), sizeof(ppn_zone_state), offsetof(ppn_zone_cfg, loiter), '
           'offsetof(ppn_zone_geom, line_xy), offsetof(ppn_zone_state, flags), PPN_ZONE_SLOTS, PPN_ZONE_MAX, PPN_ZONE_MAX_VERT, '
           'PPN_LINE_MAX, PPN_ZONE_FLAG_SLOT_OVERFLOW, PPN_ZONE_ANCHOR_CENTER, PPN_ZONE_ANCHOR_BOTTOM);return 0;}\n')
    exe = str(tmp_path / "ppn_zone_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    assert [int(v) for v in subprocess.check_output([exe]).split()] == [
        C.sizeof(lib.ZoneCfg), C.sizeof(lib.ZoneGeom), C.sizeof(lib.ZoneState), lib.ZoneCfg.loiter.offset,
        lib.ZoneGeom.line_xy.offset, lib.ZoneState.flags.offset, lib.PPN_ZONE_SLOTS, lib.PPN_ZONE_MAX, lib.PPN_ZONE_MAX_VERT,
        lib.PPN_LINE_MAX, lib.PPN_ZONE_FLAG_SLOT_OVERFLOW, lib.PPN_ZONE_ANCHOR_CENTER, lib.PPN_ZONE_ANCHOR_BOTTOM]
    assert (lib.PPN_ZONE_SLOTS, lib.PPN_ZONE_MAX, lib.PPN_ZONE_MAX_VERT, lib.PPN_LINE_MAX) == (
        R.SLOTS, R.ZONE_MAX, R.MAX_VERT, R.LINE_MAX) == (64, 16, 8, 16)
    assert (lib.PPN_ZONE_ANCHOR_CENTER, lib.PPN_ZONE_ANCHOR_BOTTOM, lib.PPN_ZONE_FLAG_SLOT_OVERFLOW) == (
        R.ANCHOR_CENTER, R.ANCHOR_BOTTOM, R.SLOT_OVERFLOW)
    assert [n for n, _ in lib.ZoneState._fields_] == list(R.fresh_state(1))
    assert [n for n, _ in lib.ZoneGeom._fields_] == list(R.fresh_geom(1))
    assert [n for n, _ in lib.ZoneCfg._fields_] == list(R.make_cfg())

    # addresses that are never dereferenced: every rejection happens before anything is launched
    good_cfg = dict(K=18, max_gap=15, anchor=lib.PPN_ZONE_ANCHOR_CENTER, loiter=1)
    st_names = [n for n, _ in lib.ZoneState._fields_]
    g_names = [n for n, _ in lib.ZoneGeom._fields_]
    st_ptrs = {n: 0x10000000 * (i + 1) for i, n in enumerate(st_names)}
    g_ptrs = {n: 0x10000000 * (i + 9) for i, n in enumerate(g_names)}
    args = dict(count=0x100000000, kp_cell=0x110000000, bbox=0x120000000, ids=0x140000000, xy=0x150000000,
                n_frames=0x160000000, out_slot=0x170000000, out_inside=0x180000000, out_zone=0x190000000,
                out_line=0x1a0000000)

    def update(cfg=None, geom=None, st=None, streams=1, frames=1, max_humans=7, null=(), **over):
        c = lib.ZoneCfg(**{**good_cfg, **(cfg or {})})
        g = lib.ZoneGeom(**{**g_ptrs, **(geom or {})})
        s = lib.ZoneState(**{**st_ptrs, **(st or {})})
        a = {**args, **over}
        return l.ppn_zone_update(None if "cfg" in null else C.byref(c), None if "geom" in null else C.byref(g),
                                 None if "st" in null else C.byref(s), a["count"], a["kp_cell"], a["bbox"], a["ids"], a["xy"],
                                 streams, frames, max_humans, a["n_frames"], a["out_slot"], a["out_inside"], a["out_zone"],
                                 a["out_line"], None)

    bad, unsupported = -1, -3
    for which in ("cfg", "geom", "st"):
        assert update(null=(which,)) == bad and b"NULL" in l.ppn_last_error(), which
    for n in st_names:
        assert update(st={n: None}) == bad and b"state" in l.ppn_last_error(), n
    for n in g_names:
        assert update(geom={n: None}) == bad and b"geometry" in l.ppn_last_error(), n
    for cfg in (dict(K=0), dict(K=lib.PPN_MAX_KP + 1), dict(max_gap=-1), dict(anchor=2), dict(anchor=-1), dict(loiter=0),
                dict(loiter=-5)):
        assert update(cfg=cfg) == bad, cfg
    for n in ("count", "kp_cell", "bbox", "ids", "out_slot", "out_inside", "out_zone", "out_line"):
        assert update(**{n: None}) == bad and b"NULL" in l.ppn_last_error(), n
    assert update(streams=0) == bad and update(frames=0) == bad and update(max_humans=0) == bad
    assert update(streams=-1) == bad and update(frames=-2) == bad and update(max_humans=-3) == bad
    assert update(max_humans=lib.PPN_MATCH_MAX_PEOPLE + 1) == unsupported and b"max_humans" in l.ppn_last_error()


def test_zones_rejects_bad_arguments_on_the_host():
    from pytorch_pose_proposal_network_amd import zones
    for kw in (dict(streams=0), dict(frames=0), dict(max_humans=0), dict(max_humans=1025), dict(K=0), dict(K=33),
               dict(max_gap=-1), dict(anchor="feet"), dict(loiter=0)):
        with pytest.raises(ValueError):
            zones.Zones(device="cpu", **kw)
    z = zones.Zones(streams=2, frames=3, max_humans=5, K=4, device="cpu")
    assert z.slot.shape == z.inside.shape == (6, 5) and z.zone.shape == (6, 16, 4) and z.line.shape == (6, 16, 2)
    assert z.state["dwell"].shape == (2, 64, 16) and z.state["last"].shape == (2, 64, 2)
    assert all(int(v.abs().sum()) == 0 for v in z.state.values())            # all zero bytes: fresh
    with pytest.raises(ValueError):
        z.update(None, None)                                                 # the kernel is the only implementation

    tri = [(0, 0), (10, 0), (0, 10)]
    octagon = [(np.cos(a), np.sin(a)) for a in np.arange(8) * np.pi / 4]
    for polys in ([tri[:2]], [octagon + [(0, 0)]], [[(0, 0), (1, np.nan), (2, 2)]], [[(0, 0), (1, np.inf), (2, 2)]],
                  [[(0, 0), (1, 1e39), (2, 2)]], [[(0, 0, 0), (1, 1, 1), (2, 2, 2)]], [[0, 1, 2]], [tri] * 17):
        with pytest.raises(ValueError):
            z.set_zones(0, polys)
    for segs in ([(0, 0, 1)], [(0, 0, 1, 1, 2)], [(0, 0, np.nan, 1)], [(0, -np.inf, 1, 1)], [(0, 0, 1, 1)] * 17, [[(0, 0), (1, 1)]]):
        with pytest.raises(ValueError):
            z.set_lines(0, segs)
    for s in (-1, 2):
        with pytest.raises(ValueError):
            z.set_zones(s, [tri])
        with pytest.raises(ValueError):
            z.set_lines(s, [(0, 0, 1, 1)])
        with pytest.raises(ValueError):
            z.reset(streams=[s])
    assert not any(int(t.abs().sum()) for t in z.geom.values())              # a rejected table uploads nothing

    z.set_zones(1, [tri, octagon])
    z.set_lines(1, [(1, 2, 3, 4)])
    want = R.make_geom([[], [tri, octagon]], [[], [(1, 2, 3, 4)]])
    for k, v in want.items():
        assert z.geom[k].numpy().tobytes() == v.tobytes(), k
    z.set_zones(1, [tri])                                                    # a shorter table clears the old entries
    z.set_lines(1, [])
    want = R.make_geom([[], [tri]], [[], []])
    for k, v in want.items():
        assert z.geom[k].numpy().tobytes() == v.tobytes(), k
    zt, lt = z.totals()
    assert zt.shape == lt.shape == (2, 16, 2) and not zt.any() and z.flags().tolist() == [0, 0]
    assert z.state_to_host()["inside"].dtype == np.uint32
