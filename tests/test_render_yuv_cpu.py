"""CPU-only checks of drawing onto raw video surfaces (include/ppn.h: ppn_rgb_to_yuv, ppn_draw_humans_yuv): the ABI, the
forward colour rule on every colour, every refusal of the entry (all come before any launch), and the paint rule on the
NumPy restatement tests/render_yuv_ref.py that tests/test_render_yuv_gpu.py holds the kernel to."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import render_cases as RC
import render_yuv_cases as YC
import render_yuv_ref as R
import yuv_ref as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATRIX = {"bt601": 0, "bt709": 1}


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def _forward(lib, rgb, matrix="bt601", full_range=False):
    rgb = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
    out = np.empty_like(rgb)
    assert lib.load().ppn_rgb_to_yuv(MATRIX[matrix], int(full_range), rgb.ctypes.data, out.ctypes.data, len(rgb)) == 0
    return out


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_exports_are_bound():
    lib = _lib()
    l = lib.load()
    for name in ("ppn_rgb_to_yuv", "ppn_draw_humans_yuv"):
        assert name in lib.EXPORTS
        assert getattr(l, name).argtypes is not None and getattr(l, name).restype is C.c_int
    from pytorch_pose_proposal_network_amd import render, rt
    assert callable(render.Renderer.draw_yuv) and callable(render.draw_people_yuv) and callable(rt.inference_windows_drawn)


def test_ctypes_struct_matches_header(tmp_path):
    lib = _lib()
    names = ("format", "height", "width", "pitch", "pitch_c", "frame_stride", "y", "u", "v", "matrix", "full_range")
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ppn.h"\nint main(){printf("%zu' + " %zu" * len(names) +
           '\\n", sizeof(ppn_yuv_surface)' + "".join(f", offsetof(ppn_yuv_surface, {n})" for n in names) + ');return 0;}\n')
    exe = str(tmp_path / "ppn_yuv_surface_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    assert v == [C.sizeof(lib.YuvSurface)] + [getattr(lib.YuvSurface, n).offset for n in names]


# ---- the forward colour rule -----------------------------------------------------------------------------------------
def test_the_table_is_the_rounded_exact_definition():
    for (matrix, full), row in R.FORWARD.items():
        assert R.derive(matrix, full) == row, (matrix, full)
        assert sum(row[1]) == 0 and sum(row[2]) == 0                    # a grey has no chroma


def test_forward_rule_on_all_colours_of_the_default_set():
    lib = _lib()
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for r0 in range(0, 256, 32):                                        # 2^24 colours in eight slabs
        rgb = np.stack([np.broadcast_to(np.arange(r0, r0 + 32, dtype=np.uint8)[:, None, None], (32, 256, 256)),
                        np.broadcast_to(g, (32, 256, 256)), np.broadcast_to(b, (32, 256, 256))], -1).reshape(-1, 3)
        got, exp = _forward(lib, rgb), R.rgb_to_yuv(rgb)
        assert np.array_equal(got, exp), r0
        assert exp[:, 0].min() >= 16 and exp[:, 0].max() <= 235 and exp[:, 1:].min() >= 16 and exp[:, 1:].max() <= 240


@pytest.mark.parametrize("matrix,full", [s for s in R.SETS if s != ("bt601", False)], ids=lambda v: str(v))
def test_forward_rule_on_a_sample_of_the_other_sets(matrix, full):
    lib = _lib()
    rgb = np.random.default_rng(18).integers(0, 256, (1 << 18, 3), dtype=np.uint8)
    got, exp = _forward(lib, rgb, matrix, full), R.rgb_to_yuv(rgb, matrix, full)
    assert np.array_equal(got, exp)
    if not full:
        assert exp[:, 0].min() >= 16 and exp[:, 0].max() <= 235 and exp[:, 1:].min() >= 16 and exp[:, 1:].max() <= 240


@pytest.mark.parametrize("matrix,full", R.SETS, ids=lambda v: str(v))
def test_greys_corners_and_extremes(matrix, full):
    lib = _lib()
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    out = _forward(lib, grey, matrix, full)
    assert (out[:, 1:] == 128).all()
    assert (out[0, 0], out[255, 0]) == ((0, 255) if full else (16, 235))
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    out = _forward(lib, corners, matrix, full)
    assert np.array_equal(out, R.rgb_to_yuv(corners, matrix, full))
    blue, red, yellow, cyan = out[1], out[4], out[6], out[3]
    assert (blue[1], red[2]) == ((255, 255) if full else (240, 240))
    if not full:
        assert (yellow[1], cyan[2]) == (16, 16) and out[:, 0].min() == 16 and out[:, 0].max() == 235
    assert (out[0, 0], out[7, 0]) == ((0, 255) if full else (16, 235))
    if full:                                                            # 256 before the clamp: sat8 matters
        cy, cu, cv, yoff = R.FORWARD[(matrix, full)]
        assert (cu[2] * 255 + (1 << 19) + (128 << 20)) >> 20 == 256 and (cv[0] * 255 + (1 << 19) + (128 << 20)) >> 20 == 256
    assert lib.load().ppn_rgb_to_yuv(2, 0, corners.ctypes.data, out.ctypes.data, 8) == -1
    assert lib.load().ppn_rgb_to_yuv(0, 0, None, out.ctypes.data, 8) == -1


def test_red_in_the_default_set_by_hand():
    # Y = (269262 * 255 + 2^19 + 16 * 2^20) >> 20 = 85963314 >> 20 = 81; U = (-155423 * 255 + 2^19 + 128 * 2^20) >> 20 = 90;
    # V = (460551 * 255 + 2^19 + 128 * 2^20) >> 20 = 252182521 >> 20 = 240
    assert _forward(_lib(), [[255, 0, 0]]).tolist() == [[81, 90, 240]]
    assert R.rgb_to_yuv(np.array([255, 0, 0], np.uint8)).tolist() == [81, 90, 240]


# ---- the refusals ----------------------------------------------------------------------------------------------------
def _surface(lib, fmt, base=0x100000, h=6, w=8, **change):
    is420 = fmt != lib.PPN_PIX_YUYV
    s = lib.YuvSurface(format=fmt, height=h, width=w, pitch=w if is420 else 2 * w,
                       pitch_c=(w if fmt == lib.PPN_PIX_NV12 else w // 2) if is420 else 0, frame_stride=4096, y=base,
                       u=base + 0x1000 if is420 else None, v=base + 0x2000 if fmt == lib.PPN_PIX_I420 else None, matrix=0,
                       full_range=0)
    for k, v in change.items():
        setattr(s, k, v)
    return s


def _call(lib, fmt, src=None, dst=None, cfg="good", batch=2, ptr=(0x10000, 0x20000, 0x30000), max_humans=4, ws=0x40000,
          null_src=False, null_dst=False):
    from pytorch_pose_proposal_network_amd import render
    c = render.make_cfg() if cfg == "good" else cfg
    s = _surface(lib, fmt, **(src or {}))
    d = _surface(lib, fmt, **dict(dict(base=0x900000), **(dst or {})))
    return lib.load().ppn_draw_humans_yuv(None if c is None else C.byref(c), None if null_src else C.byref(s),
                                          None if null_dst else C.byref(d), batch, *ptr, max_humans, ws, None)


_ALL, _420, _I420 = (0, 1, 2), (0, 1), (1,)
_BOTH = lambda **kw: dict(src=kw, dst=kw)
REFUSALS = [
    # what ppn_draw_humans refuses
    ("NULL cfg", _ALL, dict(cfg=None)),
    ("NULL count", _ALL, dict(ptr=(None, 0x20000, 0x30000))),
    ("NULL kp_cell", _ALL, dict(ptr=(0x10000, None, 0x30000))),
    ("NULL bbox", _ALL, dict(ptr=(0x10000, 0x20000, None))),
    ("NULL workspace", _ALL, dict(ws=None)),
    ("workspace off a 16-byte boundary", _ALL, dict(ws=0x40008)),
    ("batch 0", _ALL, dict(batch=0)),
    ("max_humans 0", _ALL, dict(max_humans=0)),
    ("height 0", _ALL, _BOTH(height=0)),
    ("width 0", _ALL, _BOTH(width=0)),
    # the surfaces
    ("NULL src", _ALL, dict(null_src=True)),
    ("NULL dst", _ALL, dict(null_dst=True)),
    ("NULL src y", _ALL, dict(src=dict(y=None))),
    ("NULL dst y", _ALL, dict(dst=dict(y=None))),
    ("NULL src u", _420, dict(src=dict(u=None))),
    ("NULL dst u", _420, dict(dst=dict(u=None))),
    ("NULL src v", _I420, dict(src=dict(v=None))),
    ("NULL dst v", _I420, dict(dst=dict(v=None))),
    ("format bgr24", _ALL, _BOTH(format=3)),
    ("format 4", _ALL, _BOTH(format=4)),
    ("format -1", _ALL, _BOTH(format=-1)),
    ("matrix 2", _ALL, _BOTH(matrix=2)),
    ("matrix -1", _ALL, _BOTH(matrix=-1)),
    ("odd width", _ALL, _BOTH(width=7)),
    ("odd height", _420, _BOTH(height=5)),
    ("src pitch below the row", _ALL, dict(src=dict(pitch=7))),
    ("dst pitch below the row", _ALL, dict(dst=dict(pitch=7))),
    ("src pitch_c below the row", _420, dict(src=dict(pitch_c=3))),
    ("dst pitch_c below the row", _420, dict(dst=dict(pitch_c=3))),
    ("src frame_stride below the plane", _ALL, dict(src=dict(frame_stride=5 * 8 + 7))),
    ("dst frame_stride 0", _ALL, dict(dst=dict(frame_stride=0))),
    # src against dst
    ("another format", _ALL, dict(dst=dict(format=None))),                     # filled in below: the next format
    ("another height", _ALL, dict(dst=dict(height=4))),
    ("another width", _ALL, dict(dst=dict(width=6))),
    ("another matrix", _ALL, dict(dst=dict(matrix=1))),
    ("another range", _ALL, dict(dst=dict(full_range=1))),
    ("same y, other u", _420, dict(dst=dict(y=0x100000))),
    ("same u, other y", _420, dict(dst=dict(u=0x101000))),
    ("same v, other planes", _I420, dict(dst=dict(v=0x102000))),
    ("same planes, other pitch", _ALL, dict(dst=dict(base=0x100000, pitch=32))),
    ("same planes, other pitch_c", _420, dict(dst=dict(base=0x100000, pitch_c=16))),
    ("same planes, other frame_stride", _ALL, dict(dst=dict(base=0x100000, frame_stride=8192))),
]


@pytest.mark.parametrize("what,formats,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_launch(what, formats, kw):
    lib = _lib()
    for fmt in formats:
        kw2 = {k: dict(v) if isinstance(v, dict) else v for k, v in kw.items()}
        if what == "another format":                                            # a complete surface of the next format
            other = _surface(lib, (fmt + 1) % 3, base=0x900000)
            kw2["dst"] = {n: getattr(other, n) for n, _ in lib.YuvSurface._fields_}
        assert _call(lib, fmt, **kw2) == -1, (what, fmt)                       # PPN_E_INVALID
        assert lib.load().ppn_last_error().startswith(b"ppn_draw_humans_yuv"), lib.load().ppn_last_error()


def test_bad_cfgs_and_the_size_limits():
    from pytorch_pose_proposal_network_amd import render
    lib = _lib()
    for fmt in _ALL:
        bad = render.make_cfg()
        bad.kp_order[3] = 18
        assert _call(lib, fmt, cfg=bad) == -1
        bad = render.make_cfg()
        bad.K = 0
        assert _call(lib, fmt, cfg=bad) == -1
        bad = render.make_cfg(grid=True, grid_step=4)
        bad.grid_step = 0
        assert _call(lib, fmt, cfg=bad) == -1
        big = dict(height=32770, frame_stride=1 << 40)
        assert _call(lib, fmt, src=big, dst=big) == -3                          # PPN_E_UNSUPPORTED: ppn_draw_humans' limits
        big = dict(width=32770, pitch=70000, pitch_c=70000, frame_stride=1 << 40)
        assert _call(lib, fmt, src=big, dst=big) == -3
        assert _call(lib, fmt, batch=65536) == -3


def test_good_descriptors_pass_every_surface_check():
    """Checked through the entry's LAST refusal (the workspace's alignment), so nothing is launched: the message names it.
    Out of place, in place (every plane and the geometry equal), pitched, and YUYV with an odd height."""
    lib = _lib()
    l = lib.load()
    for fmt in _ALL:
        pitched = dict(pitch=24, pitch_c=12, frame_stride=5000)
        for kw in (dict(), dict(dst=dict(base=0x100000)), dict(src=pitched, dst=dict(pitched, base=0x100000)),
                   dict(src=pitched), dict(dst=pitched), dict(src=dict(base=0x100001), dst=dict(base=0x900003))):
            assert _call(lib, fmt, ws=0x40008, **kw) == -1
            assert b"workspace must be 16-byte aligned" in l.ppn_last_error(), (fmt, kw, l.ppn_last_error())
    odd = dict(height=5)
    assert _call(lib, lib.PPN_PIX_YUYV, src=odd, dst=odd, ws=0x40008) == -1 and b"workspace" in l.ppn_last_error()


# ---- the paint rule, on the restatement ------------------------------------------------------------------------------
RED = (255, 0, 0)                                                               # -> (81, 90, 240), by hand above


def _one_pixel(fmt, raw):
    hit = np.zeros((4, 4), bool)
    hit[1, 1] = True
    colour = np.zeros((4, 4, 3), np.uint8)
    colour[1, 1] = RED
    raw = np.array(raw, np.uint8)
    return R.draw_surface(raw, raw, fmt, 4, 4, hit, colour).tolist()


def test_a_four_by_four_example_per_format():
    y = list(range(10, 26))
    drawn_y = y[:5] + [81] + y[6:]
    assert _one_pixel("nv12", y + [100, 101, 102, 103, 104, 105, 106, 107]) == \
        drawn_y + [90, 240, 102, 103, 104, 105, 106, 107]
    assert _one_pixel("i420", y + [100, 101, 102, 103] + [110, 111, 112, 113]) == \
        drawn_y + [90, 101, 102, 103] + [240, 111, 112, 113]
    #                         Y0  U   Y1  V   Y2  U   Y3  V
    assert _one_pixel("yuyv", [10, 50, 11, 60, 12, 51, 13, 61,
                               14, 52, 15, 62, 16, 53, 17, 63,
                               18, 54, 19, 64, 20, 55, 21, 65,
                               22, 56, 23, 66, 24, 57, 25, 67]) == [10, 50, 11, 60, 12, 51, 13, 61,
                                                                    14, 90, 81, 240, 16, 53, 17, 63,
                                                                    18, 54, 19, 64, 20, 55, 21, 65,
                                                                    22, 56, 23, 66, 24, 57, 25, 67]


def test_pitch_padding_and_the_tail_keep_their_bytes_and_dst_takes_src_content():
    rng = np.random.default_rng(4)
    hit = np.zeros((4, 8), bool)
    hit[3, 5] = True
    colour = np.full((4, 8, 3), 200, np.uint8)
    for fmt in Y.FORMATS:
        pitch = 22 if fmt == "yuyv" else 14
        src, dst = YC.raw_frames(rng, fmt, 2, 4, 8, pitch, tail=5)
        out = R.draw_surface(src, dst, fmt, 4, 8, hit, colour, pitch=pitch)
        base = R.draw_surface(src, src, fmt, 4, 8, hit, colour, pitch=pitch)
        content = R.draw_surface(np.zeros_like(src), np.zeros_like(src), fmt, 4, 8, np.ones((4, 8), bool), colour, pitch=pitch) != 0
        assert np.array_equal(out[content], base[content]) and np.array_equal(out[~content], dst[~content])
        assert int(content.sum()) == (4 * 8 * 3) // 2 + (16 if fmt == "yuyv" else 0) and not content[-5:].any()
        assert int((base != src).sum()) <= 3 and (base != src).any()


@pytest.mark.parametrize("name,people,visbbox,grid_step,tells", YC.anchor_cases(), ids=[c[0] for c in YC.anchor_cases()])
def test_the_targeted_cases_tell_the_chroma_rules_apart(name, people, visbbox, grid_step, tells):
    """Each case gives other bytes under the wrong rules it is listed to expose (and the same bytes under the others: the
    list says what a case is for); between them the cases expose both wrong rules in every format."""
    _, palette, order, edges, _ = RC.fixture()
    H, W = YC.H, YC.W
    hit, colour = R.painted(1, H, W, *YC.pack_people(people), order, edges, palette, visbbox, grid_step)
    assert hit.any()
    for fmt in Y.FORMATS:
        raw = YC.raw_frames(np.random.default_rng(9), fmt, 1, H, W)[0]
        right = R.draw_surface(raw, raw, fmt, H, W, hit[0], colour[0])
        luma = R.draw_surface(raw, raw, fmt, H, W, hit[0], colour[0], anchor="topleft")
        for wrong in ("topleft", "last"):
            got = R.draw_surface(raw, raw, fmt, H, W, hit[0], colour[0], anchor=wrong)
            assert (got != right).any() == (wrong in tells), (fmt, wrong)
            assert np.array_equal(Y.planes(got, fmt, H, W)[0], Y.planes(luma, fmt, H, W)[0])   # the rules differ in chroma only


def test_the_cases_expose_both_wrong_rules():
    told = set().union(*(c[4] for c in YC.anchor_cases()))
    assert told == {"topleft", "last"}
