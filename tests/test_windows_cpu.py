"""CPU-only checks of the windowed inference (include/ppn.h: ppn_ingest_windows, ppn_merge_windows): WindowLayout.tiles, the
ABI (exports, struct sizes) and every refusal of the two entries, which all come before any launch, and the rules of the
merge on the NumPy restatement tests/windows_ref.py that tests/test_windows_gpu.py holds the kernel to."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import windows_cases as WC
import windows_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


@pytest.fixture(autouse=True)
def restatement_and_library_share_their_limits():
    """The restatement's limits and flag values are the library's: a rule checked on one is a rule of the other."""
    from pytorch_pose_proposal_network_amd import lib, windows
    assert (R.MAX_WINDOWS, R.MAX_CAND) == (lib.PPN_MAX_WINDOWS, lib.PPN_MERGE_MAX_CAND) == (windows.MAX_WINDOWS, windows.MAX_CAND)
    assert (R.CAND_OVERFLOW, R.OUT_OVERFLOW) == (lib.PPN_MERGE_FLAG_CAND_OVERFLOW, lib.PPN_MERGE_FLAG_OUT_OVERFLOW)
    assert R.FORMATS.index("bgr") == lib.PPN_PIX_BGR24


# ---- WindowLayout.tiles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_hw,rows,cols,overlap", [((1080, 1920), 2, 2, 0.25), ((1080, 1920), 3, 5, 0.1),
                                                      ((144, 208), 2, 2, 0.25), ((720, 1280), 1, 4, 0.5),
                                                      ((36, 52), 4, 4, 0.0), ((480, 640), 2, 3, 0.33)])
def test_tiles_cover_the_picture_with_even_windows_and_the_overlap(src_hw, rows, cols, overlap):
    from pytorch_pose_proposal_network_amd.windows import WindowLayout
    lay = WindowLayout.tiles(src_hw, rows, cols, overlap)
    H, W = src_hw
    assert lay.n == rows * cols == lay.struct.n and lay.src_hw == src_hw
    covered = np.zeros(src_hw, bool)
    sizes = {(h, w) for _, _, h, w in lay.windows}
    assert len(sizes) == 1                                                   # equal windows
    (h, w), = sizes
    for i, (y0, x0, wh, ww) in enumerate(lay.windows):
        assert y0 % 2 == 0 and x0 % 2 == 0 and wh % 2 == 0 and ww % 2 == 0
        assert 0 <= y0 and y0 + wh <= H and 0 <= x0 and x0 + ww <= W
        covered[y0:y0 + wh, x0:x0 + ww] = True
        s = lay.struct.win[i]
        assert (s.y0, s.x0, s.h, s.w) == (y0, x0, wh, ww)
    assert covered.all()
    ys, xs = sorted({y for y, *_ in lay.windows}), sorted({x for _, x, *_ in lay.windows})
    assert len(ys) == rows and len(xs) == cols and ys[0] == 0 and xs[0] == 0
    assert ys[-1] + h == H and xs[-1] + w == W                               # the last row and column end at the border
    for a, b in zip(ys, ys[1:]):
        assert a + h - b >= overlap * h - 2
    for a, b in zip(xs, xs[1:]):
        assert a + w - b >= overlap * w - 2


def test_tiles_one_by_one_is_the_whole_picture():
    from pytorch_pose_proposal_network_amd.windows import WindowLayout
    assert WindowLayout.tiles((1080, 1920), 1, 1).windows == ((0, 0, 1080, 1920),)
    assert WindowLayout.tiles((37, 53), 1, 1, 0.9).windows == ((0, 0, 37, 53),)


def test_layout_refuses_what_the_header_refuses():
    from pytorch_pose_proposal_network_amd.windows import WindowLayout
    ok = (0, 0, 10, 10)
    for bad in ([], [ok] * 17, [(0, 0, 0, 10)], [(0, 0, 10, 0)], [(-2, 0, 10, 10)], [(0, -2, 10, 10)], [(12, 0, 10, 10)],
                [(0, 22, 10, 10)], [(0, 0, 21, 10)], [(0, 0, 10, 31)], [ok, (0, 0, 10)]):
        with pytest.raises(ValueError):
            WindowLayout((20, 30), bad)
    assert WindowLayout((20, 30), [ok] * 16).n == 16 and WindowLayout((20, 30), [(10, 20, 10, 10)]).n == 1
    for bad in (((100, 100), 0, 1, 0.25), ((100, 100), 1, 0, 0.25), ((100, 100), 3, 6, 0.25), ((100, 100), 2, 2, 1.0),
                ((100, 100), 2, 2, -0.1), ((1, 100), 2, 2, 0.25), ((101, 100), 2, 1, 0.25), ((100, 101), 1, 2, 0.25)):
        with pytest.raises(ValueError):
            WindowLayout.tiles(*bad)
    with pytest.raises(ValueError):
        WindowLayout((0, 30), [ok])
    # an odd size along an axis that is NOT cut is fine: the one window of that axis spans it
    # (100 / (2 - 0.25) = 57.1 -> windows 58 wide, the second ending at column 100)
    assert WindowLayout.tiles((101, 100), 1, 2).windows == ((0, 0, 101, 58), (0, 42, 101, 58))


def test_flipped_layout_is_where_the_windows_lie_in_the_turned_picture():
    from pytorch_pose_proposal_network_amd.windows import WindowLayout
    lay = WindowLayout((100, 160), [(0, 0, 100, 100), (0, 60, 100, 100), (10, 20, 30, 40)])
    fl = lay.flipped()
    assert fl.windows == ((0, 60, 100, 100), (0, 0, 100, 100), (60, 100, 30, 40)) and fl.src_hw == lay.src_hw
    assert fl.flipped().windows == lay.windows
    # the person in the overlap of WC.overlap_person, seen by windows whose images are turned by 180 degrees: with the
    # flipped layout the two copies coincide again, at the turned place of the frame box (20, 70, 80, 90)
    c = WC.overlap_person()
    turned = WC.Case(list(WindowLayout((100, 160), c.windows).flipped().windows), c.in_hw, 1, c.M, c.K)
    turned.count[:] = c.count
    turned.kp_cell[:], turned.score[:] = c.kp_cell, c.score
    inH, inW = c.in_hw
    turned.bbox[..., 0], turned.bbox[..., 1] = inH - c.bbox[..., 2], inW - c.bbox[..., 3]
    turned.bbox[..., 2], turned.bbox[..., 3] = inH - c.bbox[..., 0], inW - c.bbox[..., 1]
    out, keeper = turned.ref(max_out=8)
    assert out["count"][0] == 2 and keeper[0][(1, 0)] == (0, 0)
    assert out["bbox"][0, 0, 0].tolist() == [100 - 80, 160 - 90, 100 - 20, 160 - 70]
    assert np.array_equal(out["src"], c.ref(max_out=8)[0]["src"])
    # with the unflipped layout the copies of the turned images lie 60 columns apart and both survive
    wrong = WC.Case(c.windows, c.in_hw, 1, c.M, c.K)
    wrong.count[:], wrong.kp_cell[:], wrong.score[:], wrong.bbox[:] = c.count, c.kp_cell, c.score, turned.bbox
    assert wrong.ref(max_out=8)[0]["count"][0] == 3


# ---- the library's argument checks ----------------------------------------------------------------------------------
def test_exports_are_bound():
    lib = _lib()
    l = lib.load()
    for name in ("ppn_ingest_windows", "ppn_merge_windows"):
        assert name in lib.EXPORTS
        assert getattr(l, name).argtypes is not None and getattr(l, name).restype is C.c_int
    assert lib.PPN_PIX_BGR24 == 3 and lib.PPN_MAX_WINDOWS == 16 and lib.PPN_MERGE_MAX_CAND == 512
    assert (lib.PPN_MERGE_FLAG_CAND_OVERFLOW, lib.PPN_MERGE_FLAG_OUT_OVERFLOW) == (1, 2)


def test_ctypes_structs_match_header(tmp_path):
    lib = _lib()
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ppn.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", '
           'sizeof(ppn_window), sizeof(ppn_window_layout), offsetof(ppn_window_layout, win), sizeof(ppn_merge_cfg), '
           'offsetof(ppn_merge_cfg, merge_thr), offsetof(ppn_merge_cfg, fuse), PPN_PIX_BGR24, PPN_MAX_WINDOWS, '
           'PPN_MERGE_MAX_CAND, PPN_MERGE_FLAG_CAND_OVERFLOW, PPN_MERGE_FLAG_OUT_OVERFLOW);return 0;}\n')
    exe = str(tmp_path / "ppn_windows_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    assert v[:6] == [C.sizeof(lib.Window), C.sizeof(lib.WindowLayout), lib.WindowLayout.win.offset, C.sizeof(lib.MergeCfg),
                     lib.MergeCfg.merge_thr.offset, lib.MergeCfg.fuse.offset]
    assert v[6:] == [lib.PPN_PIX_BGR24, lib.PPN_MAX_WINDOWS, lib.PPN_MERGE_MAX_CAND, lib.PPN_MERGE_FLAG_CAND_OVERFLOW,
                     lib.PPN_MERGE_FLAG_OUT_OVERFLOW]


def _layout(lib, wins):
    lay = lib.WindowLayout()
    lay.n = len(wins)
    for i, w in enumerate(wins[:16]):
        lay.win[i] = lib.Window(*w)
    return lay


def _good_desc(lib, fmt):
    """A descriptor the entry would launch: frames of 6 x 8 -> 3 x 4, batch 2, fake (never dereferenced) pointers."""
    h, w = 6, 8
    is420 = fmt in (lib.PPN_PIX_NV12, lib.PPN_PIX_I420)
    row = {lib.PPN_PIX_NV12: w, lib.PPN_PIX_I420: w, lib.PPN_PIX_YUYV: 2 * w, lib.PPN_PIX_BGR24: 3 * w}[fmt]
    return lib.IngestDesc(format=fmt, batch=2, src_h=h, src_w=w, pitch=row,
                          pitch_c=(w if fmt == lib.PPN_PIX_NV12 else w // 2) if is420 else 0, frame_stride=4096, y=0x10000,
                          u=0x20000 if is420 else None, v=0x30000 if fmt == lib.PPN_PIX_I420 else None, matrix=0,
                          full_range=0, dst=0x40000, dst_h=3, dst_w=4, flip=0, dst_bgr=0)


_ALL, _YUV, _420, _I420 = (0, 1, 2, 3), (0, 1, 2), (0, 1), (1,)
GOOD_WINDOWS = [(0, 0, 6, 8), (2, 4, 4, 4)]
# what, formats, descriptor changes, windows (None: GOOD_WINDOWS; "NULL": no layout at all)
INGEST_REFUSALS = [
    # everything ppn_ingest_yuv refuses
    ("NULL dst", _ALL, dict(dst=None), None),
    ("NULL y", _ALL, dict(y=None), None),
    ("NULL u", _420, dict(u=None), None),
    ("NULL v", _I420, dict(v=None), None),
    ("format 4", _ALL, dict(format=4), None),
    ("format -1", _ALL, dict(format=-1), None),
    ("matrix 2", _ALL, dict(matrix=2), None),
    ("odd src_w", _YUV, dict(src_w=7), [(0, 0, 6, 6)]),
    ("odd src_h", _420, dict(src_h=5), [(0, 0, 4, 8)]),
    ("pitch below the row", _ALL, dict(pitch=7), None),
    ("pitch below the packed bgr row", (3,), dict(pitch=23), None),
    ("pitch_c below the row", _420, dict(pitch_c=3), None),
    ("frame_stride below the plane", _ALL, dict(frame_stride=5 * 8 + 7), None),
    ("frame_stride 0", _ALL, dict(frame_stride=0), None),
    ("batch 0", _ALL, dict(batch=0), None),
    ("src_h 0", _ALL, dict(src_h=0), None),
    ("src_w 0", _ALL, dict(src_w=0), None),
    ("dst_h 0", _ALL, dict(dst_h=0), None),
    ("dst_w 0", _ALL, dict(dst_w=0), None),
    ("batch 65536", _ALL, dict(batch=65536), None),
    ("dst_h 65536", _ALL, dict(dst_h=65536), None),
    ("src_h 16386", _ALL, dict(src_h=16386, frame_stride=1 << 40), None),
    ("src_w 16386", _ALL, dict(src_w=16386, pitch=60000, pitch_c=60000, frame_stride=1 << 40), None),
    # the layout
    ("NULL layout", _ALL, {}, "NULL"),
    ("no window", _ALL, {}, []),
    ("17 windows", _ALL, {}, [(0, 0, 6, 8)] * 17),
    ("h 0", _ALL, {}, [(0, 0, 0, 8)]),
    ("w 0", _ALL, {}, [(0, 0, 6, 0)]),
    ("negative h", _ALL, {}, [(0, 0, -2, 8)]),
    ("negative y0", _ALL, {}, [(-2, 0, 6, 8)]),
    ("negative x0", _ALL, {}, [(0, -2, 6, 8)]),
    ("below the picture", _ALL, {}, [(2, 0, 6, 8)]),
    ("right of the picture", _ALL, {}, [(0, 2, 6, 8)]),
    ("y0 + h overflows int32", _ALL, {}, [(2, 0, 2 ** 31 - 2, 8)]),
    ("the second window is bad", _ALL, {}, [(0, 0, 6, 8), (0, 6, 6, 4)]),
    ("odd x0", _YUV, {}, [(0, 1, 6, 6)]),
    ("odd w", _YUV, {}, [(0, 0, 6, 5)]),
    ("odd y0", _420, {}, [(1, 0, 4, 8)]),
    ("odd h", _420, {}, [(0, 0, 5, 8)]),
    ("F * n above 65535", _ALL, dict(batch=4096), [(0, 0, 6, 8)] * 16),
]


@pytest.mark.parametrize("what,formats,change,wins", INGEST_REFUSALS, ids=[r[0] for r in INGEST_REFUSALS])
def test_ingest_refusals_come_before_any_launch(what, formats, change, wins):
    lib = _lib()
    l = lib.load()
    for fmt in formats:
        d = _good_desc(lib, fmt)
        for k, v in change.items():
            setattr(d, k, v)
        lay = None if wins == "NULL" else C.byref(_layout(lib, GOOD_WINDOWS if wins is None else wins))
        assert l.ppn_ingest_windows(C.byref(d), lay, None) == -1, (what, fmt)              # PPN_E_INVALID
        assert l.ppn_last_error().startswith(b"ppn_ingest_windows"), l.ppn_last_error()
    assert l.ppn_ingest_windows(None, C.byref(_layout(lib, GOOD_WINDOWS)), None) == -1
    assert l.ppn_last_error().startswith(b"ppn_ingest_windows")


def test_the_format_rules_border_on_what_is_accepted():
    """What the parity refusals border on is legal elsewhere: YUYV takes odd y0 and h, packed BGR any parity and an odd
    picture.  Checked through a later refusal (F * n above 65535), so nothing is launched: the message names that refusal,
    which comes after the window checks."""
    lib = _lib()
    l = lib.load()
    for fmt, src, win in ((lib.PPN_PIX_YUYV, (7, 8), (1, 2, 5, 4)), (lib.PPN_PIX_BGR24, (7, 9), (1, 3, 5, 5)),
                          (lib.PPN_PIX_NV12, (6, 8), (2, 2, 4, 6))):
        d = _good_desc(lib, fmt)
        d.src_h, d.src_w, d.batch = src[0], src[1], 4096
        d.pitch = {lib.PPN_PIX_YUYV: 2, lib.PPN_PIX_BGR24: 3, lib.PPN_PIX_NV12: 1}[fmt] * src[1]
        assert l.ppn_ingest_windows(C.byref(d), C.byref(_layout(lib, [win] * 16)), None) == -1
        assert b"exceed 65535" in l.ppn_last_error(), l.ppn_last_error()


def test_ingest_yuv_still_refuses_packed_bgr():
    lib = _lib()
    l = lib.load()
    d = _good_desc(lib, lib.PPN_PIX_BGR24)
    assert l.ppn_ingest_yuv(C.byref(d), None) == -1
    assert l.ppn_last_error().startswith(b"ppn_ingest_yuv: unknown format 3")


def _merge_call(lib, cfg=None, lay="good", null=None, frames=1, misalign=None, **cfg_change):
    c = lib.MergeCfg(18, 96, 96, 36, 72, 0.3, 1) if cfg is None else cfg
    for k, v in cfg_change.items():
        setattr(c, k, v)
    layout = _layout(lib, GOOD_WINDOWS) if lay == "good" else lay
    ptr = [0x10000 * (i + 1) for i in range(9)]                      # count kp_cell bbox score | count src bbox score flags
    if null is not None:
        ptr[null] = None
    if misalign is not None:
        ptr[misalign] += 4
    return lib.load().ppn_merge_windows(C.byref(c) if c != "NULL" else None, None if layout is None else C.byref(layout),
                                        *ptr[:4], frames, *ptr[4:], None)


MERGE_REFUSALS = [("NULL " + n, dict(null=i)) for i, n in enumerate(
    ("count", "kp_cell", "bbox", "score", "out_count", "out_src", "out_bbox", "out_score", "out_flags"))] + [
    ("NULL cfg", dict(cfg="NULL")), ("NULL layout", dict(lay=None)),
    ("K 0", dict(K=0)), ("K 33", dict(K=33)), ("max_out 0", dict(max_out=0)), ("max_humans 0", dict(max_humans=0)),
    ("max_humans 1025", dict(max_humans=1025)), ("frames 0", dict(frames=0)), ("negative frames", dict(frames=-1)),
    ("NaN merge_thr", dict(merge_thr=float("nan"))), ("inH 0", dict(inH=0)), ("inW 0", dict(inW=0)),
    ("no window", dict(lay=[])), ("17 windows", dict(lay=[(0, 0, 4, 4)] * 17)), ("h 0", dict(lay=[(0, 0, 0, 4)])),
    ("w 0", dict(lay=[(0, 0, 4, 0)])), ("negative origin", dict(lay=[(0, 0, 4, 4), (-2, 0, 4, 4)])),
    ("bbox 4 bytes off a 16-byte boundary", dict(misalign=2)), ("out_bbox 4 bytes off a 16-byte boundary", dict(misalign=6)),
]


@pytest.mark.parametrize("what,kw", MERGE_REFUSALS, ids=[r[0] for r in MERGE_REFUSALS])
def test_merge_refusals_come_before_any_launch(what, kw):
    lib = _lib()
    kw = dict(kw)
    if isinstance(kw.get("lay"), list):
        kw["lay"] = _layout(lib, kw["lay"])
    assert _merge_call(lib, **kw) == -1, what                                              # PPN_E_INVALID
    assert lib.load().ppn_last_error().startswith(b"ppn_merge_windows"), lib.load().ppn_last_error()


# ---- the rules, on the restatement ----------------------------------------------------------------------------------
def _people(case, out, f=0):
    """[(src of keypoint 0, {j: src}), ...] of frame f."""
    n = min(int(out["count"][f]), out["src"].shape[1])
    return [(int(out["src"][f, r, 0]), {j: int(s) for j, s in enumerate(out["src"][f, r]) if s >= 0}) for r in range(n)]


def test_a_person_in_the_overlap_comes_out_once_with_the_better_keypoints():
    c = WC.overlap_person()
    M = c.M
    out, keeper = c.ref(max_out=8)
    A, B, other = 0 * M + 0, 1 * M + 0, 1 * M + 1
    assert out["count"][0] == 2 and out["flags"][0] == 0
    assert keeper[0] == {(0, 0): (0, 0), (1, 0): (0, 0), (1, 1): (1, 1)}
    assert _people(c, out) == [(A, {0: A, 1: A, 2: B, 3: B}), (other, {0: other, 4: other})]
    # frame pixels: the root of window 0 at scale 2, keypoint 3 from window 1 (origin x 60)
    assert out["bbox"][0, 0, 0].tolist() == [20, 70, 80, 90] and out["bbox"][0, 0, 3].tolist() == [60, 78, 64, 82]
    assert out["score"][0, 0].tolist() == [F(0.9), F(0.5), F(0.9), F(0.4), 0]
    assert out["src"][0, 0, 4] == -1 and not out["bbox"][0, 0, 4].any()
    plain, _ = c.ref(max_out=8, fuse=False)
    assert _people(c, plain) == [(A, {0: A, 1: A, 2: A}), (other, {0: other, 4: other})]
    assert plain["score"][0, 0].tolist() == [F(0.9), F(0.5), F(0.8), 0, 0]


def test_two_people_of_one_window_both_survive():
    c = WC.same_window_pair()
    a, b = c.bbox[0, 0, 0], c.bbox[0, 1, 0]
    assert R.iou(a, R.area(a), b, R.area(b)) > F(0.6)
    out, _ = c.ref(max_out=4)
    assert out["count"][0] == 2 and [p[0] for p in _people(c, out)] == [0, 1]


def test_a_duplicate_suppresses_nobody():
    c = WC.chain()
    A, B, C_ = (c.bbox[i, 0, 0] for i in range(3))
    io = lambda a, b: R.iou(a, R.area(a), b, R.area(b))
    assert io(A, B) >= F(0.3) and io(B, C_) >= F(0.3) and io(A, C_) < F(0.3)
    out, keeper = c.ref(max_out=4)
    assert keeper[0] == {(0, 0): (0, 0), (1, 0): (0, 0), (2, 0): (2, 0)}
    assert _people(c, out) == [(0, {0: 0, 1: c.M}), (2 * c.M, {0: 2 * c.M, 1: 2 * c.M})]      # A takes B's better keypoint 1


def test_equal_root_scores_go_to_the_lower_window_and_row():
    c = WC.equal_scores()
    out, keeper = c.ref(max_out=4)
    M = c.M
    assert keeper[0] == {(0, 0): (0, 0), (1, 0): (0, 0), (2, 0): (0, 0), (0, 1): (0, 1), (1, 1): (0, 1), (2, 1): (0, 1)}
    # equal keypoint scores: only a strictly larger one replaces the keeper's
    assert _people(c, out) == [(0, {0: 0, 1: 0}), (1, {0: 1})]
    assert M == 3


def test_rootless_people_bad_counts_and_nan_roots_are_skipped():
    c = WC.skipped()
    out, keeper = c.ref(max_out=16)
    M = c.M
    assert sorted(keeper[0]) == [(0, 0), (0, 2)] + [(2, p) for p in range(4)]
    assert out["count"][0] == 6 and out["flags"][0] == 0
    assert [p[0] for p in _people(c, out)] == [0, 2, 2 * M, 2 * M + 1, 2 * M + 2, 2 * M + 3]


def test_both_overflow_flags():
    c = WC.crowd()
    out, keeper = c.ref(max_out=100, out=R.fresh_outputs(2, 100, c.K, fill=0xC3))
    assert len(keeper[0]) == 512 and out["count"].tolist() == [512, 1]
    assert out["flags"].tolist() == [R.CAND_OVERFLOW | R.OUT_OVERFLOW, 0]
    assert (out["src"][0, :, 0] >= 0).all()
    sentinel = np.full(4, 0xC3, np.uint8).view(np.int32)[0]
    assert (out["src"][1, 1:] == sentinel).all() and (out["bbox"][1, 1:].view(np.int32) == sentinel).all()      # untouched
    assert _people(c, out, 1) == [(0, {0: 0, 2: c.M})]
    roomy, _ = c.ref(max_out=600)
    assert roomy["flags"].tolist() == [R.CAND_OVERFLOW, 0] and roomy["count"].tolist() == [512, 1]


def test_one_whole_picture_window_at_the_input_size_returns_the_people():
    c = WC.identity()
    out, _ = c.ref(max_out=c.M)
    for f in range(2):
        P = int(c.count[f])
        assert out["count"][f] == P
        assert np.array_equal(out["bbox"][f, :P].view(np.int32), c.bbox[f, :P].view(np.int32))         # bit-identical
        assert np.array_equal(out["score"][f, :P].view(np.int32), c.score[f, :P].view(np.int32))
        assert np.array_equal(out["src"][f, :P] >= 0, c.kp_cell[f, :P] >= 0)
        assert np.array_equal(out["src"][f, :P, 0], np.arange(P))


def test_the_threshold_sweep_straddles_merge_thr_and_tells_a_reciprocal_divide_apart():
    """Conditions on the inputs (seed 1, 24 pairs x 6 values, merge_thr 0.3), not measurements: 144 frames, of which 72
    have iou >= thr and 72 iou < thr in the restatement's arithmetic; 3 frames change sides under inter * (1 / den) and 3
    under a denominator ai + aj - inter that is rounded once."""
    c, frames = WC.threshold_sweep()
    exact, _ = c.ref(max_out=2)
    merged = exact["count"] == 1
    print(f"{c.frames} frames: {int(merged.sum())} merged, {int((~merged).sum())} apart")
    assert merged.sum() >= 10 and (~merged).sum() >= 10
    recip, _ = c.ref(max_out=2, recip_iou=True)
    fused, _ = c.ref(max_out=2, fused_iou=True)
    n_recip, n_fused = int((recip["count"] != exact["count"]).sum()), int((fused["count"] != exact["count"]).sum())
    print(f"{n_recip} frames change sides under a reciprocal divide, {n_fused} under a fused denominator")
    assert n_recip + n_fused >= 1
    thr = F(0.3)
    for f, (A, B) in enumerate(frames):                                                   # every frame sits at the knife edge
        v = R.iou(A, R.area(A), B, R.area(B))
        assert abs(float(v) - 0.3) < 1e-5 and (v >= thr) == bool(merged[f])


def test_the_mapping_sweep_tells_a_fused_multiply_add_apart():
    """Conditions on the inputs (seed 2, 200 people x 2 keypoints x 4 coordinates = 1600 mapped numbers): the fused form
    y * sy + y0 in one rounding differs from multiply-then-add in 193 of them."""
    c = WC.mapping_sweep()
    exact, _ = c.ref(max_out=c.M)
    fused, _ = c.ref(max_out=c.M, fused_map=True)
    assert np.array_equal(exact["src"], fused["src"])
    differ = int((exact["bbox"].view(np.int32) != fused["bbox"].view(np.int32)).sum())
    print(f"{differ} of {exact['bbox'].size} mapped coordinates differ under a fused multiply-add")
    assert differ >= 10
