"""CPU-only checks of the person crops (include/ppn.h: ppn_people_rois, ppn_ingest_rois): the properties of the ROI rule on
the NumPy restatement tests/crops_ref.py that tests/test_crops_gpu.py holds the kernels to, the ABI (exports, struct sizes)
and every refusal of the two entries, which all come before any launch."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import crops_cases as CC
import crops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


@pytest.fixture(autouse=True)
def restatement_and_library_share_their_constants():
    from pytorch_pose_proposal_network_amd import crops, lib
    assert (R.OK, R.EMPTY, R.DEGENERATE, R.BAD) == (lib.PPN_ROI_OK, lib.PPN_ROI_EMPTY, lib.PPN_ROI_DEGENERATE, lib.PPN_ROI_BAD)
    assert (R.MODE_ROOT, R.MODE_PEOPLE) == (lib.PPN_ROI_MODE_ROOT, lib.PPN_ROI_MODE_PEOPLE)
    assert R.ALIGN == crops._ALIGN


# ---- the rule, on the restatement -----------------------------------------------------------------------------------
def _rois(case, mode, margin, keep, align, max_rois, min_size=4):
    sy, sx = R.scales(CC.SRC_HW, CC.COORDS_HW)
    aspect = R.aspect_of(CC.OUT_HW) if keep else F(0)
    return R.people_rois(case.count, case.kp_cell, case.bbox, CC.SRC_HW, sy, sx, max_rois, mode, margin, aspect, align, min_size)


def _mapped_box(case, f, r, mode):
    """The person's mapped box in float64 from the f32 products (exact), clipped to the picture."""
    sy, sx = R.scales(CC.SRC_HW, CC.COORDS_HW)
    b, fin = R.person_box(case.kp_cell[f, r], case.bbox[f, r], mode)
    assert fin
    m = [float(F(b[0] * sy)), float(F(b[1] * sx)), float(F(b[2] * sy)), float(F(b[3] * sx))]
    H, W = CC.SRC_HW
    return max(m[0], 0.0), max(m[1], 0.0), min(m[2], float(H)), min(m[3], float(W))


@pytest.mark.parametrize("mode,margin,keep,align,max_rois", CC.CONFIGS)
def test_ok_rois_are_inside_aligned_large_enough_and_hold_the_box(mode, margin, keep, align, max_rois):
    H, W = CC.SRC_HW
    seen = 0
    for case in (CC.planted(), CC.random_people(1), CC.random_people(2)):
        roi, status = _rois(case, mode, margin, keep, align, max_rois)
        assert roi.shape == (case.frames, max_rois, 4) and status.shape == (case.frames, max_rois)
        for f in range(case.frames):
            P = min(max(int(case.count[f]), 0), CC.M)
            for r in range(max_rois):
                y0, x0, h, w = (int(v) for v in roi[f, r])
                person = r < P and case.kp_cell[f, r, 0] >= 0
                assert (status[f, r] == R.EMPTY) == (not person)
                if status[f, r] != R.OK:
                    assert (y0, x0, h, w) == (0, 0, 0, 0) and status[f, r] in (R.EMPTY, R.DEGENERATE)
                    continue
                seen += 1
                assert 0 <= y0 and y0 + h <= H and 0 <= x0 and x0 + w <= W                      # inside the picture
                assert y0 % align[0] == 0 and h % align[0] == 0 and x0 % align[1] == 0 and w % align[1] == 0
                assert h >= 4 and w >= 4                                                        # min_size
                ymin, xmin, ymax, xmax = _mapped_box(case, f, r, mode)
                if ymin < ymax and xmin < xmax:                                                 # the box's part of the picture
                    assert y0 <= ymin and ymax <= y0 + h and x0 <= xmin and xmax <= x0 + w, (f, r)
    assert seen >= 10


@pytest.mark.parametrize("mode", [0, 1])
def test_without_margin_aspect_and_alignment_the_roi_is_the_hull_of_the_mapped_box(mode):
    H, W = CC.SRC_HW
    sy, sx = R.scales(CC.SRC_HW, CC.COORDS_HW)
    seen = 0
    for case in (CC.planted(), CC.random_people(3), CC.random_people(4)):
        roi, status = _rois(case, mode, 0.0, False, (1, 1), CC.M, min_size=1)
        for f, r in zip(*np.nonzero(status == R.OK)):
            b, _ = R.person_box(case.kp_cell[f, r], case.bbox[f, r], mode)
            m = [F(b[0] * sy), F(b[1] * sx), F(b[2] * sy), F(b[3] * sx)]
            # centre +- half in f32 gives the edges back up to one rounding each: the hull of [edge - ulp, edge + ulp]
            lo = lambda v, n: min(max(math.floor(float(v)), 0), n)
            hi = lambda v, n: min(max(math.ceil(float(v)), 0), n)
            exact = (lo(m[0], H), lo(m[1], W), hi(m[2], H) - lo(m[0], H), hi(m[3], W) - lo(m[1], W))
            got = tuple(int(v) for v in roi[f, r])
            frac = [abs(float(v) - round(float(v))) for v in m]
            if min(frac) > 1e-3:                          # no edge within a rounding of an integer: the hull is exact
                assert got == exact, (f, r, m)
                seen += 1
            else:
                assert all(abs(a - b) <= 1 for a, b in zip(got, exact))
    assert seen >= 10


def test_planted_people_get_the_status_their_name_says():
    case = CC.planted()
    roi, status = _rois(case, R.MODE_PEOPLE, 0.1, True, (2, 2), 8)
    assert status[0, :5].tolist() == [R.OK] * 5 and status[0, 5:].tolist() == [R.EMPTY] * 3      # five people, slots to spare
    assert roi[0, 0, :2].tolist() == [0, 0] and roi[0, 3, 0] + roi[0, 3, 2] == CC.SRC_HW[0]      # the corners touch the borders
    assert roi[0, 1, 1] + roi[0, 1, 3] == CC.SRC_HW[1] and roi[0, 2, 1] == 0
    # frame 1: outside, zero area, NaN, no root, wild absent keypoints (a normal person), infinity; count 9 -> 6 people
    assert status[1].tolist() == [R.DEGENERATE, R.DEGENERATE, R.DEGENERATE, R.EMPTY, R.OK, R.DEGENERATE, R.EMPTY, R.EMPTY]
    assert roi[1, 4, 2] < 40 and roi[1, 4, 3] < 40                                               # the wild boxes were not read
    assert (status[2] == R.EMPTY).all() and not roi[2].any()                                     # count -3
    # mode root does not look at keypoint 3's NaN, but at the root's
    _, st_root = _rois(case, R.MODE_ROOT, 0.1, True, (2, 2), 8)
    assert st_root[1, 2] == R.OK and st_root[1, 5] == R.DEGENERATE
    one = CC.nan_root()
    for mode in (0, 1):
        assert _rois(one, mode, 0.0, False, (1, 1), 2)[1].tolist() == [[R.DEGENERATE, R.EMPTY]]
    # the first max_rois people are taken
    roi4, st4 = _rois(case, R.MODE_PEOPLE, 0.1, True, (2, 2), 4)
    assert np.array_equal(roi4, roi[:, :4]) and np.array_equal(st4, status[:, :4])
    # a zero-area box is a crop once min_size allows its 1 x 1 (aligned: 2 x 2) hull
    _, st1 = _rois(case, R.MODE_ROOT, 0.0, False, (1, 1), 8, min_size=1)
    assert st1[1, 1] == R.OK


def test_every_f32_step_is_rounded_on_its_own():
    """The restatement tells one IEEE operation per step from a contracted hh + hh * margin: some planted margin makes the
    two differ in the ROI, so equality with the kernel (tests/test_crops_gpu.py) pins the kernel's form."""
    differ = 0
    rng = np.random.default_rng(5)
    for _ in range(4000):
        lo, hi, margin = F(rng.uniform(0, 40)), F(rng.uniform(40, 90)), F(rng.uniform(0, 0.5))
        c, half = R._span(lo, hi, margin)
        h0 = F(F(hi - lo) * R.HALF)
        fused = F(np.float64(h0) + np.float64(h0) * np.float64(margin))
        differ += int(half != fused)
    assert differ > 100


def test_judge_names_every_kind_of_bad_rectangle():
    H, W = 36, 52
    good = {"nv12": (2, 4, 10, 12), "i420": (2, 4, 10, 12), "yuyv": (3, 4, 9, 12), "bgr": (3, 5, 9, 11)}
    for fmt, g in good.items():
        assert R.judge(g, fmt, (H, W)) == R.OK and R.judge((0, 0, 0, 0), fmt, (H, W)) == R.EMPTY
        assert R.judge((0, 0, H, W), fmt, (H, W)) == R.OK
        for bad in ((-2, 4, 10, 12), (2, -4, 10, 12), (2, 4, 0, 12), (2, 4, 10, 0), (2, 4, -10, 12), (28, 4, 10, 12),
                    (2, 42, 10, 12), (0, 0, 0, 2), (2, 4, 2 ** 31 - 2, 12)):
            assert R.judge(bad, fmt, (H, W)) == R.BAD, (fmt, bad)
    assert R.judge((2, 5, 10, 12), "yuyv", (H, W)) == R.BAD and R.judge((2, 4, 10, 11), "nv12", (H, W)) == R.BAD
    assert R.judge((3, 4, 10, 12), "i420", (H, W)) == R.BAD and R.judge((2, 4, 9, 12), "nv12", (H, W)) == R.BAD


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_exports_are_bound():
    lib = _lib()
    l = lib.load()
    for name in ("ppn_people_rois", "ppn_ingest_rois"):
        assert name in lib.EXPORTS
        assert getattr(l, name).argtypes is not None and getattr(l, name).restype is C.c_int


def test_ctypes_structs_match_header(tmp_path):
    lib = _lib()
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ppn.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d\\n", '
           'sizeof(ppn_roi_cfg), offsetof(ppn_roi_cfg, src_h), offsetof(ppn_roi_cfg, sy), offsetof(ppn_roi_cfg, mode), '
           'offsetof(ppn_roi_cfg, aspect), offsetof(ppn_roi_cfg, align_y), offsetof(ppn_roi_cfg, min_size), PPN_ROI_OK, '
           'PPN_ROI_EMPTY, PPN_ROI_DEGENERATE, PPN_ROI_BAD, PPN_ROI_MODE_ROOT, PPN_ROI_MODE_PEOPLE);return 0;}\n')
    exe = str(tmp_path / "ppn_crops_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    T = lib.RoiCfg
    assert v[:7] == [C.sizeof(T), T.src_h.offset, T.sy.offset, T.mode.offset, T.aspect.offset, T.align_y.offset,
                     T.min_size.offset]
    assert v[7:] == [lib.PPN_ROI_OK, lib.PPN_ROI_EMPTY, lib.PPN_ROI_DEGENERATE, lib.PPN_ROI_BAD, lib.PPN_ROI_MODE_ROOT,
                     lib.PPN_ROI_MODE_PEOPLE]


# ---- refusals: fake pointers that a launch would fault on, no stream, no device --------------------------------------
def _roi_call(lib, null=None, frames=2, misalign=None, **change):
    c = lib.RoiCfg(18, 36, 16, 1080, 1920, 2.8125, 5.0, 1, 0.1, 0.5, 2, 2, 8)
    for k, v in change.items():
        setattr(c, k, v)
    ptr = dict(count=0x10000, kp_cell=0x20000, bbox=0x30000, roi=0x40000, status=0x50000)
    if misalign:
        ptr[misalign] += 4
    if null and null != "cfg":
        ptr[null] = None
    return lib.load().ppn_people_rois(None if null == "cfg" else C.byref(c), ptr["count"], ptr["kp_cell"], ptr["bbox"], frames,
                                      ptr["roi"], ptr["status"], None)


ROI_REFUSALS = [dict(null=n) for n in ("cfg", "count", "kp_cell", "bbox", "roi", "status")] + [
    dict(K=0), dict(K=33), dict(max_humans=0), dict(max_humans=1025), dict(max_rois=0), dict(max_rois=-1), dict(frames=0),
    dict(src_h=0), dict(src_w=0), dict(src_h=16386), dict(src_w=-2), dict(min_size=0), dict(align_y=0), dict(align_y=3),
    dict(align_x=4), dict(align_x=-1), dict(min_size=1), dict(align_y=2, src_h=1081, align_x=1), dict(mode=2), dict(mode=-1),
    dict(margin=float("nan")), dict(margin=-0.1), dict(margin=float("inf")), dict(aspect=float("nan")), dict(aspect=-1.0),
    dict(aspect=float("inf")), dict(sy=0.0), dict(sx=-1.0), dict(sy=float("nan")), dict(sx=float("inf")),
    dict(misalign="bbox"), dict(misalign="roi"),
]


@pytest.mark.parametrize("change", ROI_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c in ROI_REFUSALS])
def test_people_rois_refusals_come_before_any_launch(change):
    lib = _lib()
    assert _roi_call(lib, **change) == -1, change                                         # PPN_E_INVALID
    assert lib.load().ppn_last_error().startswith(b"ppn_people_rois"), lib.load().ppn_last_error()


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
# what, formats, descriptor changes, (roi pointer, max_rois)
INGEST_REFUSALS = [
    # everything ppn_ingest_windows refuses of the descriptor
    ("NULL dst", _ALL, dict(dst=None), None),
    ("NULL y", _ALL, dict(y=None), None),
    ("NULL u", _420, dict(u=None), None),
    ("NULL v", _I420, dict(v=None), None),
    ("format 4", _ALL, dict(format=4), None),
    ("format -1", _ALL, dict(format=-1), None),
    ("matrix 2", _ALL, dict(matrix=2), None),
    ("odd src_w", _YUV, dict(src_w=7), None),
    ("odd src_h", _420, dict(src_h=5), None),
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
    # the table
    ("NULL roi", _ALL, {}, (None, 4)),
    ("max_rois 0", _ALL, {}, (0x50000, 0)),
    ("max_rois -1", _ALL, {}, (0x50000, -1)),
    ("F * max_rois above 65535", _ALL, dict(batch=4096), (0x50000, 16)),
    ("F * max_rois overflows int32", _ALL, dict(batch=65535), (0x50000, 2 ** 31 - 1)),
]


@pytest.mark.parametrize("what,formats,change,table", INGEST_REFUSALS, ids=[r[0] for r in INGEST_REFUSALS])
def test_ingest_rois_refusals_come_before_any_launch(what, formats, change, table):
    lib = _lib()
    l = lib.load()
    roi, max_rois = (0x50000, 4) if table is None else table
    for fmt in formats:
        d = _good_desc(lib, fmt)
        for k, v in change.items():
            setattr(d, k, v)
        for status in (None, 0x60000):
            assert l.ppn_ingest_rois(C.byref(d), roi, max_rois, status, None) == -1, (what, fmt)      # PPN_E_INVALID
            assert l.ppn_last_error().startswith(b"ppn_ingest_rois"), l.ppn_last_error()
    assert l.ppn_ingest_rois(None, 0x50000, 4, None, None) == -1
    assert l.ppn_last_error().startswith(b"ppn_ingest_rois")


def test_cropper_refuses_bad_arguments_without_a_device():
    from pytorch_pose_proposal_network_amd.crops import PersonCropper
    good = dict(frames=2, max_humans=36, src_hw=(64, 96), fmt="nv12", out_hw=(12, 8), device="cpu")
    c = PersonCropper(**good)
    assert (c.cfg.align_y, c.cfg.align_x) == (2, 2) and c.coords_hw == (64, 96) and c.cfg.sy == 1.0
    assert c.cfg.aspect == float(R.aspect_of((12, 8))) and c.cfg.mode == R.MODE_PEOPLE
    assert tuple(c.crops.shape) == (2, 16, 12, 8, 3) and tuple(c.roi.shape) == (2, 16, 4) and tuple(c.status.shape) == (2, 16)
    y = PersonCropper(**dict(good, fmt="yuyv", src_hw=(63, 96), keep_aspect=False, mode="root", coords_hw=(24, 40)))
    assert (y.cfg.align_y, y.cfg.align_x, y.cfg.aspect, y.cfg.mode) == (1, 2, 0.0, R.MODE_ROOT)
    assert (F(y.cfg.sy), F(y.cfg.sx)) == R.scales((63, 96), (24, 40))
    for bad in (dict(frames=0), dict(max_humans=0), dict(max_humans=1025), dict(max_crops=0), dict(fmt="p010"), dict(mode="face"),
                dict(src_hw=(63, 96)), dict(src_hw=(64, 95)), dict(out_hw=(0, 8)), dict(coords_hw=(0, 40)), dict(margin=-0.5),
                dict(margin=float("nan")), dict(min_size=1), dict(min_size=0), dict(K=0), dict(K=33),
                dict(frames=4096, max_crops=16)):
        with pytest.raises(ValueError):
            PersonCropper(**dict(good, **bad))
