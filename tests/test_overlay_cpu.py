"""CPU-only checks of the monitoring overlay (include/ppn.h: ppn_draw_scene, ppn_draw_scene_yuv): the font and the number
formatting, the ABI, every refusal of the entries (all come before any launch), and that the cases of tests/overlay_cases.py
put the rules of the NumPy restatement tests/overlay_ref.py -- which tests/test_overlay_gpu.py holds the kernel to -- on
the spot."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import overlay_cases as OC
import overlay_ref as O
import render_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


# ---- 1. the font -----------------------------------------------------------------------------------------------------
DIGITS = {
    "0": (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
    "1": ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
    "2": (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),
    "3": ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),
    "4": ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),
    "5": ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),
    "6": ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),
    "7": ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),
    "8": (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),
    "9": (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),
}


def _bitmap(rows):
    return np.array([[ch == "#" for ch in row] for row in rows])


def test_the_header_prints_the_font_of_the_restatement():
    text = open(os.path.join(ROOT, "include", "ppn.h")).read()
    rows = re.findall(r"^ \*\s+FONT\s+(\d+)\s+((?:[0-9A-F]{2}\s+){7})", text, re.M)
    assert [int(r[0]) for r in rows] == list(range(16))
    assert tuple(tuple(int(v, 16) for v in r[1].split()) for r in rows) == O.FONT
    assert all(0 <= v < 32 for g in O.FONT for v in g) and len(O.GLYPHS) == 14


@pytest.mark.parametrize("scale", [1, 3])
def test_ten_digits_against_hand_written_bitmaps(scale):
    x0, y0 = 2, 1
    H, W = y0 + 7 * scale + 2, x0 + 60 * scale + 2
    got = O.text_mask(H, W, x0, y0, scale, O.codes_of("0123456789"))
    exp = np.zeros((H, W), bool)
    for i, d in enumerate("0123456789"):
        big = np.kron(_bitmap(DIGITS[d]), np.ones((scale, scale), bool))
        exp[y0:y0 + 7 * scale, x0 + 6 * scale * i:x0 + 6 * scale * i + 5 * scale] = big
    assert np.array_equal(got, exp)
    clipped = O.text_mask(H - 3, W - 7, x0, y0, scale, O.codes_of("0123456789"))       # a label cut at the right and bottom
    assert np.array_equal(clipped, exp[:H - 3, :W - 7])
    assert np.array_equal(O.text_mask(H, W, x0 - 4, y0 - 2, scale, O.codes_of("0123456789"))[:H - 2, :W - 4], exp[2:, 4:])


def test_the_other_glyphs():
    m = O.text_mask(7, 24, 0, 0, 1, O.codes_of(":-# "))
    assert m[:, 0:5].sum() == 4 and m[3, 6:11].all() and m[:, 6:11].sum() == 5 and m[:, 12:17].sum() == 20
    assert not m[:, 18:].any() and not m[:, 5].any() and not m[:, 11].any()


# ---- 2. the formatting -----------------------------------------------------------------------------------------------
def test_number_formatting():
    assert [O.count_text(v) for v in (0, 9, 10, 999999, 1000000, -5, 2 ** 31 - 1, -2 ** 31)] == \
        ["0", "9", "10", "999999", "999999", "0", "999999", "0"]
    assert O.id_text(2 ** 31 - 1) == "2147483647" and len(O.id_text(2 ** 31 - 1)) == 10 and O.id_text(1) == "1"
    assert O.codes_of("10:7") == [1, 0, 10, 7]
    assert O.wrap32(2 ** 31) == -2 ** 31 and O.wrap32(-2 ** 31 - 1) == 2 ** 31 - 1


# ---- 3. the ABI ------------------------------------------------------------------------------------------------------
def test_exports_are_bound():
    lib = _lib()
    l = lib.load()
    for name in ("ppn_draw_scene", "ppn_draw_scene_yuv", "ppn_draw_scene_workspace_bytes"):
        assert name in lib.EXPORTS and getattr(l, name).argtypes is not None
    from pytorch_pose_proposal_network_amd import render, rt
    assert callable(render.Overlay) and callable(rt.inference_batch_zones_drawn)
    c = render.make_cfg()
    people = l.ppn_draw_workspace_bytes(C.byref(c), 3, 5)
    assert l.ppn_draw_scene_workspace_bytes(C.byref(c), 3, 5) == people + 3 * (224 + 3 * 5) * 48
    assert l.ppn_draw_scene_workspace_bytes(C.byref(c), 0, 5) == 0 and l.ppn_draw_scene_workspace_bytes(None, 1, 1) == 0


@pytest.mark.parametrize("struct,names", [
    ("ppn_overlay_cfg", ("frames", "scale", "tick", "plates", "zone_colour", "line_colour", "id_colour", "active", "alert", "text",
                         "plate")),
    ("ppn_overlay_in", ("ids", "geom", "out_zone", "out_line", "line_total", "n_frames"))])
def test_ctypes_structs_match_the_header(tmp_path, struct, names):
    lib = _lib()
    mirror = {"ppn_overlay_cfg": lib.OverlayCfg, "ppn_overlay_in": lib.OverlayIn}[struct]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ppn.h"\nint main(){printf("%zu' + " %zu" * len(names) +
           f'\\n", sizeof({struct})' + "".join(f", offsetof({struct}, {n})" for n in names) + ');return 0;}\n')
    exe = str(tmp_path / (struct + "_sizeof"))
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    assert v == [C.sizeof(mirror)] + [getattr(mirror, n).offset for n in names]
    assert [n for n, _ in mirror._fields_] == list(names)


def test_overlay_cfg_carries_the_colours():
    from pytorch_pose_proposal_network_amd import render
    c = render.Overlay(frames=3, scale=2, tick=5.5, plates=False, colours=dict(zone=(1, 2, 3), id=OC.COLOURS["id"],
                                                                              alert=(9, 8, 7))).cfg()
    assert (c.frames, c.scale, c.tick, c.plates) == (3, 2, 5.5, 0)
    assert all(tuple(c.zone_colour[z])[:3] == (1, 2, 3) for z in range(16))
    assert [tuple(c.id_colour[i])[:3] for i in range(16)] == OC.COLOURS["id"] and tuple(c.alert)[:3] == (9, 8, 7)
    assert tuple(c.active)[:3] == render.DEFAULT_COLOURS["active"]
    for bad in (dict(frames=0), dict(scale=0), dict(scale=5), dict(tick=-1.0), dict(tick=float("nan")), dict(tick=float("inf")),
                dict(tick=1e39), dict(colours=dict(zone=[(1, 2, 3)] * 15)), dict(colours=dict(text=(1, 2, 256))),
                dict(colours=dict(glow=(1, 2, 3)))):
        with pytest.raises(ValueError):
            render.Overlay(**bad)


# ---- 4. the refusals -------------------------------------------------------------------------------------------------
def _call(lib, yuv=False, ov="good", oin="good", cfg="good", batch=4, ptr=(0x10000, 0x20000, 0x30000), ws=0x40000, zone=None,
          **ov_change):
    from pytorch_pose_proposal_network_amd import render
    c = render.make_cfg() if cfg == "good" else cfg
    o = render.Overlay(frames=2).cfg() if ov == "good" else ov
    for k, v in ov_change.items():
        setattr(o, k, v)
    i = lib.OverlayIn(ids=0x50000) if oin == "good" else oin
    for k, v in (zone or {}).items():
        setattr(i.geom if k in dict(lib.ZoneGeom._fields_) else i, k, v)
    head = (None if c is None else C.byref(c), None if o is None else C.byref(o), None if i is None else C.byref(i))
    if yuv:
        s, d = (lib.YuvSurface(format=lib.PPN_PIX_NV12, height=6, width=8, pitch=8, pitch_c=8, frame_stride=4096, y=base,
                               u=base + 0x1000, v=None, matrix=0, full_range=0) for base in (0x100000, 0x900000))
        return lib.load().ppn_draw_scene_yuv(*head, C.byref(s), C.byref(d), batch, *ptr, 4, ws, None)
    return lib.load().ppn_draw_scene(*head, 0x100000, 0x900000, batch, 6, 8, *ptr, 4, ws, None)


_ZONE_PART = dict(zone_n=0x60000, zone_nv=0x61000, zone_xy=0x62000, line_n=0x63000, line_xy=0x64000, out_zone=0x65000,
                  out_line=0x66000, line_total=0x67000)
REFUSALS = [
    ("NULL cfg", dict(cfg=None)),
    ("NULL overlay", dict(ov=None)),
    ("NULL in", dict(oin=None)),
    ("NULL count", dict(ptr=(None, 0x20000, 0x30000))),
    ("NULL kp_cell", dict(ptr=(0x10000, None, 0x30000))),
    ("NULL bbox", dict(ptr=(0x10000, 0x20000, None))),
    ("NULL workspace", dict(ws=None)),
    ("workspace off a 16-byte boundary", dict(ws=0x40008)),
    ("batch 0", dict(batch=0)),
    ("scale 0", dict(scale=0)),
    ("scale 5", dict(scale=5)),
    ("frames 0", dict(frames=0)),
    ("frames -1", dict(frames=-1)),
    ("batch no multiple of frames", dict(frames=3)),
    ("negative tick", dict(tick=-0.5)),
    ("tick NaN", dict(tick=float("nan"))),
    ("tick inf", dict(tick=float("inf"))),
] + [(f"zone part without {n}", dict(zone={k: v for k, v in _ZONE_PART.items() if k != n})) for n in _ZONE_PART]


@pytest.mark.parametrize("yuv", [False, True], ids=["rgb", "yuv"])
@pytest.mark.parametrize("what,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_launch(what, kw, yuv):
    lib = _lib()
    assert _call(lib, yuv, **kw) == -1, what                                    # PPN_E_INVALID
    assert lib.load().ppn_last_error().startswith(b"ppn_draw_scene_yuv" if yuv else b"ppn_draw_scene:"), lib.load().ppn_last_error()


@pytest.mark.parametrize("yuv", [False, True], ids=["rgb", "yuv"])
def test_good_overlays_pass_every_overlay_check(yuv):
    """Checked through the entry's LAST refusal (the workspace's alignment), so nothing is launched: the message names it."""
    lib = _lib()
    for kw in (dict(), dict(zone=_ZONE_PART), dict(oin=lib.OverlayIn()), dict(oin=lib.OverlayIn(), zone=_ZONE_PART),
               dict(scale=4, tick=0.0, frames=4), dict(frames=1, batch=5), dict(zone=dict(n_frames=0x70000))):
        assert _call(lib, yuv, ws=0x40008, **kw) == -1
        assert b"workspace must be 16-byte aligned" in lib.load().ppn_last_error(), (kw, lib.load().ppn_last_error())
    assert _call(lib, yuv, batch=65536, frames=1) == -3                         # ppn_draw_humans' limits still hold


# ---- 5 and 6. the cases and the rules --------------------------------------------------------------------------------
def _draw(case, wrong=None, stats=None, base=None):
    _, palette, order, edges, _ = RC.fixture()
    count, kp_cell, bbox = case["people"]
    frames = RC.gradient(len(count), case["H"], case["W"]) if base is None else base
    g = case["grid_step"]
    return O.scene_ref(frames, count, kp_cell, bbox, order, edges, palette, case["visbbox"], g > 0, max(g, 1),
                       overlay=case["overlay"], ids=case["ids"], zones=case["zones"], n_frames=case["n_frames"], wrong=wrong,
                       stats=stats)


CASES = OC.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cases_paint_what_they_claim_and_tell_the_rules_apart(case):
    stats = {}
    right = _draw(case, stats=stats)
    assert case["claims"] and all(stats.get(kind, 0) > 0 for kind in case["claims"]), (case["claims"], stats)
    plain = RC.ref_draw(RC.gradient(len(case["people"][0]), case["H"], case["W"]), *case["people"], case["visbbox"],
                        case["grid_step"] > 0, max(case["grid_step"], 1))
    assert (right != plain).any()
    for wrong in case["tells"]:
        assert (_draw(case, wrong) != right).any(), wrong


def test_the_cases_expose_every_wrong_rule():
    assert set().union(*(c["tells"] for c in CASES)) == set(O.WRONG)
    assert set().union(*(c["claims"] for c in CASES)) == set(O.KINDS)


def test_running_totals_frame_by_frame():
    case = OC.running()
    z = case["zones"]
    assert [O.running_totals(z["line_total"], z["out_line"], 3, 0, t, 0) for t in range(3)] == [(11, 20), (11, 20), (11, 22)]
    assert [O.running_totals(z["line_total"], z["out_line"], 3, 0, t, 0, suffix=False) for t in range(3)] == [(11, 22)] * 3
    wrapped = dict(line_total=np.array([[[-2 ** 31, 0]]], np.int32), out_line=np.array([[[0, 0]], [[1, 0]]], np.int32))
    assert O.running_totals(wrapped["line_total"], wrapped["out_line"], 2, 0, 0, 0) == (2 ** 31 - 1, 0)
    right, wrong = _draw(case), _draw(case, "no_suffix")
    assert np.array_equal(right[2], wrong[2]) and (right[0] != wrong[0]).any() and (right[1] != wrong[1]).any()
    # the labels themselves: "11:20" on frames 0 and 1, "11:22" on frame 2, at T(m) + (3, 3) = (31, 7)
    hit = (right == np.array(OC.COLOURS["text"], np.uint8)).all(-1)
    for t, text in enumerate(("11:20", "11:20", "11:22")):
        assert np.array_equal(hit[t], O.text_mask(24, 64, 31, 7, 1, O.codes_of(text))), t


def test_an_image_beyond_n_frames_gets_no_overlay_and_absent_parts_draw_nothing():
    both, cut = OC.reactive()
    a, b = _draw(both), _draw(cut)
    plain = RC.ref_draw(RC.gradient(2, both["H"], both["W"]), *both["people"])
    assert np.array_equal(a[0], b[0]) and np.array_equal(b[1], plain[1]) and (a[1] != plain[1]).any()
    assert np.array_equal(_draw(dict(both, ids=None, zones=None)), plain)


def test_the_chunk_case_puts_more_than_256_overlay_primitives_on_one_tile():
    case = [c for c in CASES if c["name"].startswith("more than 256")][0]
    count, kp_cell, bbox = case["people"]
    prims = O.overlay_prims(0, case["H"], case["W"], kp_cell.shape[1], count, kp_cell, bbox, case["overlay"], case["ids"],
                            case["zones"])
    assert case["H"] <= 8 and case["W"] <= 128                                  # the frame is one tile
    assert sum(bool(mask.any()) for _, _, mask, _ in prims) > 256
    assert [p[0] for p in prims] == sorted(p[0] for p in prims) and len({p[0] for p in prims}) == len(prims)
