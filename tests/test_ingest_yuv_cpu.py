"""CPU-only checks of the raw-video ingest (include/ppn.h: ppn_ingest_yuv): the coefficient table, the properties of the
NumPy restatement tests/yuv_ref.py that tests/test_ingest_yuv_gpu.py holds the kernel to, the ABI (exports, struct size) and
every refusal of the entry, which all come before any launch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import yuv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = [("bt601", False), ("bt709", False), ("bt601", True), ("bt709", True)]


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


@pytest.fixture(scope="module")
def triples():
    """10^6 random (Y, U, V) triples, shared and never written."""
    t = np.random.default_rng(0).integers(0, 256, (1000, 1000, 3), dtype=np.uint8)
    t.setflags(write=False)
    return t


def test_coefficient_table():
    lib = _lib()
    l = lib.load()
    out = (C.c_int32 * 6)()
    for matrix, full in SETS:
        assert l.ppn_yuv_coefficients(int(matrix == "bt709"), int(full), out) == 0
        assert tuple(out) == R.COEFF[(matrix, full)], (matrix, full)
        real = R.REAL[(matrix, full)]
        assert tuple(int(round(c * 2 ** 20)) for c in real[:5]) + (real[5],) == R.COEFF[(matrix, full)]
    # OpenCV's ITUR_BT_601_CY, _CVR, _CVG, _CUG, _CUB (color_yuv.simd.hpp) and its shift of 20
    assert l.ppn_yuv_coefficients(0, 0, out) == 0
    assert tuple(out)[:5] == (1220542, 1673527, -852492, -409993, 2116026) and out[5] == 16
    assert l.ppn_yuv_coefficients(2, 0, out) == -1 and l.ppn_yuv_coefficients(-1, 0, out) == -1
    assert l.ppn_yuv_coefficients(0, 0, None) == -1


@pytest.mark.parametrize("matrix,full", SETS)
def test_fixed_point_rule_is_within_one_lsb_of_the_real_formula(triples, matrix, full):
    Y, U, V = (triples[..., i] for i in range(3))
    cy, cvr, cvg, cug, cub, yoff = R.REAL[(matrix, full)]
    y = np.maximum(0.0, Y.astype(np.float64) - yoff) * cy
    uu, vv = U.astype(np.float64) - 128, V.astype(np.float64) - 128
    real = np.clip(np.rint(np.stack([y + cvr * vv, y + cvg * vv + cug * uu, y + cub * uu], -1)), 0, 255)
    d = np.abs(R.convert(Y, U, V, matrix, full).astype(np.int64) - real.astype(np.int64))
    assert d.max() <= 1, d.max()


def test_bt601_full_range_is_within_one_lsb_of_pillow(triples):
    from PIL import Image
    pil = np.asarray(Image.fromarray(np.ascontiguousarray(triples), "YCbCr").convert("RGB")).astype(np.int64)
    d = np.abs(R.convert(triples[..., 0], triples[..., 1], triples[..., 2], "bt601", True).astype(np.int64) - pil)
    print(f"max |diff| {d.max()}, {100.0 * (d == 1).mean():.1f} % of values differ by 1")
    assert d.max() <= 1, d.max()


@pytest.mark.parametrize("matrix,full", SETS)
def test_gray_pixels_stay_gray(matrix, full):
    Y = np.arange(256, dtype=np.uint8)
    g = np.full(256, 128, np.uint8)
    rgb = R.convert(Y, g, g, matrix, full)
    assert np.array_equal(rgb[:, 0], rgb[:, 1]) and np.array_equal(rgb[:, 1], rgb[:, 2])
    if full:
        assert np.array_equal(rgb[:, 0], Y)
    else:
        assert rgb[16, 0] == 0 and rgb[235, 0] == 255 and rgb[:17, 0].max() == 0 and rgb[235:, 0].min() == 255


def _picture(seed, h, w):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8),
            rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8))


def test_one_picture_in_three_packings_converts_to_the_same_rgb():
    h, w = 12, 20
    Y, U, V = _picture(1, h, w)
    ref = R.convert(Y, np.repeat(np.repeat(U, 2, 0), 2, 1), np.repeat(np.repeat(V, 2, 0), 2, 1))
    for fmt in R.FORMATS:
        raw = R.pack(Y, U, V, fmt)
        assert raw.size == R.frame_bytes(fmt, h, w)
        assert np.array_equal(R.to_rgb(raw, fmt, h, w), ref), fmt
    # YV12 is I420 with the chroma planes swapped
    yv12 = R.pack(Y, V, U, "i420")
    n = h * w
    swapped = np.concatenate([yv12[:n], yv12[n + n // 4:], yv12[n:n + n // 4]])
    assert np.array_equal(R.to_rgb(swapped, "i420", h, w), ref)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_pitched_packing_equals_the_tight_one(fmt):
    h, w = 8, 10
    Y, U, V = _picture(2, h, w)
    pitch = 64
    tight, wide = R.pack(Y, U, V, fmt), R.pack(Y, U, V, fmt, pitch)
    assert wide.size == R.frame_bytes(fmt, h, w, pitch) > tight.size
    assert np.array_equal(R.to_rgb(wide, fmt, h, w, pitch), R.to_rgb(tight, fmt, h, w))
    for a, b in zip(R.planes(wide, fmt, h, w, pitch), R.planes(tight, fmt, h, w)):
        assert np.array_equal(a, b)
    assert np.array_equal(R.ingest(wide, fmt, h, w, (5, 7), pitch, flip=True), R.ingest(tight, fmt, h, w, (5, 7))[::-1, ::-1])


def test_exports_are_bound():
    lib = _lib()
    l = lib.load()
    for name in ("ppn_ingest_yuv", "ppn_yuv_coefficients"):
        assert name in lib.EXPORTS
        assert getattr(l, name).argtypes is not None and getattr(l, name).restype is C.c_int
    assert (lib.PPN_PIX_NV12, lib.PPN_PIX_I420, lib.PPN_PIX_YUYV) == (0, 1, 2)


def test_ctypes_descriptor_matches_header(tmp_path):
    lib = _lib()
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ppn.h"\nint main(){printf("%zu %zu %zu %zu %d %d %d\\n", '
           'sizeof(ppn_ingest_desc), offsetof(ppn_ingest_desc, frame_stride), offsetof(ppn_ingest_desc, dst), '
           'offsetof(ppn_ingest_desc, dst_bgr), PPN_PIX_NV12, PPN_PIX_I420, PPN_PIX_YUYV);return 0;}\n')
    exe = str(tmp_path / "ppn_ingest_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    size, o_stride, o_dst, o_bgr, nv12, i420, yuyv = map(int, subprocess.check_output([exe]).split())
    D = lib.IngestDesc
    assert size == C.sizeof(D)
    assert (o_stride, o_dst, o_bgr) == (D.frame_stride.offset, D.dst.offset, D.dst_bgr.offset)
    assert (nv12, i420, yuyv) == (lib.PPN_PIX_NV12, lib.PPN_PIX_I420, lib.PPN_PIX_YUYV)


def _good(lib, fmt):
    """A descriptor the entry would launch: 8x6 -> 4x3, batch 2, fake (never dereferenced) non-NULL pointers."""
    h, w = 6, 8
    d = lib.IngestDesc(format=fmt, batch=2, src_h=h, src_w=w, pitch=2 * w if fmt == lib.PPN_PIX_YUYV else w,
                       pitch_c=0 if fmt == lib.PPN_PIX_YUYV else (w if fmt == lib.PPN_PIX_NV12 else w // 2),
                       frame_stride=4096, y=0x10000, u=None if fmt == lib.PPN_PIX_YUYV else 0x20000,
                       v=0x30000 if fmt == lib.PPN_PIX_I420 else None, matrix=0, full_range=0, dst=0x40000, dst_h=3, dst_w=4,
                       flip=0, dst_bgr=0)
    return d


_ANY, _NV12, _I420, _YUYV, _420 = (0, 1, 2), (0,), (1,), (2,), (0, 1)
REFUSALS = [
    ("NULL dst", _ANY, dict(dst=None)),
    ("NULL y", _ANY, dict(y=None)),
    ("NULL u", _420, dict(u=None)),
    ("NULL v", _I420, dict(v=None)),
    ("format 3", _ANY, dict(format=3)),
    ("format -1", _ANY, dict(format=-1)),
    ("matrix 2", _ANY, dict(matrix=2)),
    ("matrix -1", _ANY, dict(matrix=-1)),
    ("odd src_w", _ANY, dict(src_w=7)),
    ("odd src_h", _420, dict(src_h=5)),
    ("pitch below the row", _420, dict(pitch=7)),
    ("pitch below the packed row", _YUYV, dict(pitch=15)),
    ("pitch_c below the row (nv12)", _NV12, dict(pitch_c=7)),
    ("pitch_c below the row (i420)", _I420, dict(pitch_c=3)),
    ("frame_stride below the Y plane", _420, dict(frame_stride=5 * 8 + 7)),
    ("frame_stride below the packed plane", _YUYV, dict(frame_stride=5 * 16 + 15)),
    ("frame_stride below the chroma plane", _NV12, dict(pitch=8, pitch_c=4096, frame_stride=4096)),
    ("frame_stride 0", _ANY, dict(frame_stride=0)),
    ("batch 0", _ANY, dict(batch=0)),
    ("src_h 0", _ANY, dict(src_h=0)),
    ("src_w 0", _ANY, dict(src_w=0)),
    ("dst_h 0", _ANY, dict(dst_h=0)),
    ("dst_w 0", _ANY, dict(dst_w=0)),
    ("negative dst_w", _ANY, dict(dst_w=-4)),
    ("batch 65536", _ANY, dict(batch=65536)),
    ("dst_h 65536", _ANY, dict(dst_h=65536)),
    ("src_h 16386", _ANY, dict(src_h=16386, frame_stride=1 << 40)),
    ("src_w 16386", _ANY, dict(src_w=16386, pitch=40000, pitch_c=40000, frame_stride=1 << 40)),
]


@pytest.mark.parametrize("what,formats,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_before_any_launch(what, formats, change):
    lib = _lib()
    l = lib.load()
    for fmt in formats:
        d = _good(lib, fmt)
        for k, v in change.items():
            setattr(d, k, v)
        assert l.ppn_ingest_yuv(C.byref(d), None) == -1, (what, fmt)           # PPN_E_INVALID
        assert l.ppn_last_error().startswith(b"ppn_ingest_yuv")
    assert l.ppn_ingest_yuv(None, None) == -1


def test_yuyv_accepts_an_odd_height_and_the_limits_themselves():
    """The validation accepts what the refusals border on (checked through the Python-side layout, which needs no device):
    an odd YUYV height, and rt.yuv_frame_layout agrees with yuv_ref.frame_bytes."""
    from pytorch_pose_proposal_network_amd import rt
    for fmt in R.FORMATS:
        for (h, w, pitch) in ((6, 8, None), (32, 48, 64), (1080, 1920, 2048), (2, 2, None)):
            if pitch is not None and fmt == "yuyv":
                pitch *= 2                                              # a packed row holds 2 bytes per pixel
            n, p, pc, uo, vo = rt.yuv_frame_layout(fmt, (h, w), pitch)
            assert n == R.frame_bytes(fmt, h, w, pitch), (fmt, h, w, pitch)
            assert (uo is None) == (fmt == "yuyv") and (vo is None) == (fmt != "i420")
    assert rt.yuv_frame_layout("yuyv", (5, 8))[0] == 5 * 16
    for bad in (("nv12", (5, 8), None), ("i420", (6, 7), None), ("yuyv", (6, 7), None), ("nv12", (6, 8), 7),
                ("i420", (6, 8), 9), ("p010", (6, 8), None)):
        with pytest.raises(ValueError):
            rt.yuv_frame_layout(*bad)
