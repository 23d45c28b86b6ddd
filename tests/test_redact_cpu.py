"""CPU-only checks of the redaction (include/ppn.h: ppn_redact_cells, ppn_redact_yuv): the NumPy restatement
tests/redact_ref.py against plain Python loops and its own properties, the coverage of tests/redact_cases.py (every planted
situation is reached, every deliberately wrong rule is told from the right one), the ABI (exports, struct sizes) and every
refusal of the two entries and of Redactor, all before any device work."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import redact_cases as RC
import redact_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SMALL = {"nv12": (10, 20), "i420": (10, 20), "yuyv": (9, 20), "bgr": (9, 19)}    # cell 8: 2 x 3 cells, partial last row / column


def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


@pytest.fixture(autouse=True)
def restatement_and_library_share_their_constants():
    from pytorch_pose_proposal_network_amd import lib
    assert (R.FALLBACK_PERSON, R.FALLBACK_NONE, R.FLAG_BAD_BOX) == (lib.PPN_REDACT_FALLBACK_PERSON, lib.PPN_REDACT_FALLBACK_NONE,
                                                                    lib.PPN_REDACT_FLAG_BAD_BOX)
    assert (R.MOSAIC, R.FILL) == (lib.PPN_REDACT_MOSAIC, lib.PPN_REDACT_FILL)


# ---- the restatement --------------------------------------------------------------------------------------------------
def _loops(raw, fmt, h, w, pitch, mask, cell, mode, fill):
    """ppn_redact_yuv's rule pixel by pixel on one frame, independent of redact_ref's offset tables: a dict from byte offset to
    (set key) is built by walking every pixel, then every set is averaged."""
    row = {"bgr": 3 * w, "yuyv": 2 * w}.get(fmt, w)
    pitch = row if pitch is None else pitch
    sets = {}                                                    # (cy, cx, channel) -> list of byte offsets

    def put(cy, cx, ch, off):
        sets.setdefault((cy, cx, ch), []).append(off)
    for y in range(h):
        for x in range(w):
            cy, cx = y // cell, x // cell
            if fmt == "bgr":
                for c in range(3):
                    put(cy, cx, c, y * pitch + 3 * x + c)
            elif fmt == "yuyv":
                put(cy, cx, 0, y * pitch + 2 * x)
                if x % 2 == 0:
                    put(cy, cx, 1, y * pitch + 2 * x + 1)
                    put(cy, cx, 2, y * pitch + 2 * x + 3)
            else:
                put(cy, cx, 0, y * pitch + x)
                if x % 2 == 0 and y % 2 == 0:
                    i, j = y // 2, x // 2
                    if fmt == "nv12":
                        put(cy, cx, 1, h * pitch + i * pitch + 2 * j)
                        put(cy, cx, 2, h * pitch + i * pitch + 2 * j + 1)
                    else:
                        pc = pitch // 2
                        put(cy, cx, 1, h * pitch + i * pc + j)
                        put(cy, cx, 2, h * pitch + (h // 2) * pc + i * pc + j)
    out = [int(v) for v in raw]
    for (cy, cx, ch), offs in sets.items():
        if not (int(mask[cy, cx // 32]) >> (cx % 32)) & 1:
            continue
        s, n = sum(int(raw[o]) for o in offs), len(offs)
        for o in offs:
            out[o] = fill[ch] if mode == R.FILL else (s + n // 2) // n
    return np.array(out, np.uint8)


@pytest.mark.parametrize("mode", [R.MOSAIC, R.FILL])
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("fmt", list(SMALL))
def test_restatement_equals_plain_loops(fmt, padded, mode):
    h, w = SMALL[fmt]
    pitch = None if not padded else {"nv12": w + 6, "i420": w + 6, "yuyv": 2 * w + 5, "bgr": 3 * w + 4}[fmt]
    rng = np.random.default_rng(len(fmt) + 7 * padded)
    raw = rng.integers(0, 256, R.frame_bytes(fmt, h, w, pitch) + 5, dtype=np.uint8)
    mask = np.array([[0b101 | 0xfffffff8], [0b110]], np.uint32)          # garbage above CW = 3 in the first row
    got = R.redact(raw, fmt, h, w, mask, 8, mode, (11, 22, 33), pitch)
    assert np.array_equal(got, _loops(raw, fmt, h, w, pitch, mask, 8, mode, (11, 22, 33)))
    assert (got != raw).any()


@pytest.mark.parametrize("cell", RC.CELLS)
@pytest.mark.parametrize("fmt", list(RC.PICTURES))
def test_restatement_is_idempotent_and_keeps_everything_else(fmt, cell):
    h, w = RC.PICTURES[fmt]
    pitch = RC.padded_pitch(fmt)
    raw, mask = RC.frames_of(fmt, 3, pitch, extra=9, frames=1)[0], RC.random_mask(fmt, cell, 4, frames=1)[0]
    once = R.redact(raw, fmt, h, w, mask, cell, pitch=pitch)
    assert np.array_equal(R.redact(once, fmt, h, w, mask, cell, pitch=pitch), once)             # the mean of equal values
    content = np.zeros(len(raw), bool)
    content[R.content_offsets(fmt, h, w, pitch)] = True
    assert np.array_equal(once[~content], raw[~content]) and (~content).sum() > h              # pitch padding and the tail
    none = np.zeros_like(mask)
    assert np.array_equal(R.redact(raw, fmt, h, w, none, cell, pitch=pitch), raw)
    CH, CW, _ = R.grid_of((h, w), cell)
    for cy in range(CH):                                                                        # unmasked cells keep their bytes
        for cx in range(CW):
            idx = np.concatenate([s[0] for s in R.sample_sets(fmt, h, w, pitch, cell, cy, cx)])
            if not R.bit(mask, cy, cx):
                assert np.array_equal(once[idx], raw[idx])
    # the sample sets of all cells are the content, each byte once
    every = np.concatenate([s[0] for cy in range(CH) for cx in range(CW) for s in R.sample_sets(fmt, h, w, pitch, cell, cy, cx)])
    assert np.array_equal(np.sort(every), np.sort(R.content_offsets(fmt, h, w, pitch)))


@pytest.mark.parametrize("fmt", list(RC.PICTURES))
def test_fill_is_the_converted_colour(fmt):
    lib = _lib()
    h, w = RC.PICTURES[fmt]
    rgb = (200, 30, 90)
    fill = R.fill_bytes(fmt, rgb, "bt709", True)
    if fmt == "bgr":
        assert fill == (90, 30, 200)
    else:
        buf = (C.c_uint8 * 3)(*rgb)
        assert lib.load().ppn_rgb_to_yuv(1, 1, buf, buf, 1) == 0 and tuple(buf) == fill
    raw = RC.frames_of(fmt, 5, frames=1)[0]
    ones = np.full(R.grid_of((h, w), 16)[0::2], 0xffffffff, np.uint32)
    got = R.redact(raw, fmt, h, w, ones, 16, R.FILL, fill)
    for cy, cx in ((0, 0), (2, 33)):
        for idx, which, _ in R.sample_sets(fmt, h, w, None, 16, cy, cx):
            assert (got[idx] == fill[which]).all()
    assert np.array_equal(np.unique(got[R.content_offsets(fmt, h, w)]), np.unique(fill))


# ---- case coverage ------------------------------------------------------------------------------------------------------
def test_cases_reach_every_planted_situation():
    assert RC.self_check()


def _cells_all(rule):
    out = []
    for case, S, T in ((RC.planted(), RC.FRAMES, 1), (RC.hold_sequence(), RC.STREAMS, RC.STEPS)):
        for cell in RC.CELLS:
            for hold in RC.HOLDS:
                CH, CW, _ = R.grid_of(RC.PICTURES["nv12"], cell)
                ttl = np.zeros((S, CH, CW), np.uint8)
                out.append(R.cells(case.count, case.kp_cell, case.bbox, ttl, S, T, rule=rule, **RC.cells_args("nv12", cell, hold=hold)))
    return out


@pytest.mark.parametrize("rule", [r for r in R.CELLS_RULES if r])
def test_wrong_cells_rules_differ_on_the_cases(rule):
    right, wrong = _cells_all(None), _cells_all(rule)
    assert any(not np.array_equal(a[0], b[0]) for a, b in zip(right, wrong))


@pytest.mark.parametrize("rule", [r for r in R.REDACT_RULES if r])
def test_wrong_redact_rules_differ_on_the_cases(rule):
    differ = 0
    for fmt in RC.PICTURES:
        h, w = RC.PICTURES[fmt]
        raw, mask = RC.frames_of(fmt, 6), RC.random_mask(fmt, 16, 7)
        mask[:, -1, -1] |= np.uint32(2)                                      # the bottom-right partial cell (bit 33 - 32)
        differ += int(not np.array_equal(R.redact_frames(raw, fmt, h, w, mask, 16), R.redact_frames(raw, fmt, h, w, mask, 16, rule=rule)))
    assert differ >= (3 if rule == "uv_together" else 4)                     # packed BGR has no U and V


def test_every_f32_step_is_rounded_on_its_own():
    """A contracted hh + hh * margin rounds differently often enough that byte equality with the kernel pins its form (as in
    tests/test_crops_cpu.py)."""
    differ, rng = 0, np.random.default_rng(5)
    for _ in range(4000):
        lo, hi, margin = F(rng.uniform(0, 40)), F(rng.uniform(40, 90)), F(rng.uniform(0, 0.5))
        _, half = R._span(lo, hi, margin)
        h0 = F(F(hi - lo) * R.HALF)
        differ += int(half != F(np.float64(h0) + np.float64(h0) * np.float64(margin)))
    assert differ > 100


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_exports_are_bound():
    lib = _lib()
    l = lib.load()
    for name in ("ppn_redact_cells", "ppn_redact_yuv"):
        assert name in lib.EXPORTS
        assert getattr(l, name).argtypes is not None and getattr(l, name).restype is C.c_int


def test_ctypes_structs_match_header(tmp_path):
    lib = _lib()
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "ppn.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", '
           'sizeof(ppn_redact_cells_cfg), offsetof(ppn_redact_cells_cfg, cell), offsetof(ppn_redact_cells_cfg, sy), '
           'offsetof(ppn_redact_cells_cfg, kp_mask), offsetof(ppn_redact_cells_cfg, margin), offsetof(ppn_redact_cells_cfg, hold), '
           'sizeof(ppn_redact_cfg), offsetof(ppn_redact_cfg, mode), offsetof(ppn_redact_cfg, fill), PPN_REDACT_FALLBACK_PERSON, '
           'PPN_REDACT_FALLBACK_NONE, PPN_REDACT_FLAG_BAD_BOX, PPN_REDACT_MOSAIC, PPN_REDACT_FILL);return 0;}\n')
    exe = str(tmp_path / "ppn_redact_sizeof")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    v = list(map(int, subprocess.check_output([exe]).split()))
    T, U = lib.RedactCellsCfg, lib.RedactCfg
    assert v[:9] == [C.sizeof(T), T.cell.offset, T.sy.offset, T.kp_mask.offset, T.margin.offset, T.hold.offset, C.sizeof(U),
                     U.mode.offset, U.fill.offset]
    assert v[9:] == [lib.PPN_REDACT_FALLBACK_PERSON, lib.PPN_REDACT_FALLBACK_NONE, lib.PPN_REDACT_FLAG_BAD_BOX,
                     lib.PPN_REDACT_MOSAIC, lib.PPN_REDACT_FILL]


# ---- refusals: fake pointers that a launch would fault on, no stream, no device ----------------------------------------
def _cells_call(lib, null=None, streams=2, frames=3, misalign=None, **change):
    c = lib.RedactCellsCfg(18, 36, 1080, 1920, 16, 2.8125, 5.0, RC.HEAD, 0, 0.25, 8)
    for k, v in change.items():
        setattr(c, k, v)
    ptr = dict(ttl=0x10000, count=0x20000, kp_cell=0x30000, bbox=0x40000, mask=0x50000, flags=0x60000)
    if misalign:
        ptr[misalign] += 4
    if null and null != "cfg":
        ptr[null] = None
    return lib.load().ppn_redact_cells(None if null == "cfg" else C.byref(c), ptr["ttl"], ptr["count"], ptr["kp_cell"], ptr["bbox"],
                                       streams, frames, ptr["mask"], ptr["flags"], None)


CELLS_REFUSALS = [dict(null=n) for n in ("cfg", "ttl", "count", "kp_cell", "bbox", "mask", "flags")] + [
    dict(K=0), dict(K=33), dict(max_humans=0), dict(max_humans=1025), dict(streams=0), dict(frames=0), dict(streams=-1),
    dict(src_h=0), dict(src_w=0), dict(src_h=16385), dict(src_w=16385), dict(src_w=-2), dict(cell=0), dict(cell=4), dict(cell=12),
    dict(cell=64), dict(cell=-16), dict(sy=0.0), dict(sx=-1.0), dict(sy=float("nan")), dict(sx=float("inf")),
    dict(margin=float("nan")), dict(margin=-0.1), dict(margin=float("inf")), dict(hold=-1), dict(hold=255), dict(fallback=2),
    dict(fallback=-1), dict(kp_mask=0), dict(kp_mask=1 << 18), dict(kp_mask=1 << 4, K=4), dict(misalign="bbox"),
]


@pytest.mark.parametrize("change", CELLS_REFUSALS, ids=[",".join(f"{k}={v}" for k, v in c.items()) for c in CELLS_REFUSALS])
def test_redact_cells_refusals_come_before_any_launch(change):
    lib = _lib()
    assert _cells_call(lib, **change) == -1, change                                       # PPN_E_INVALID
    assert lib.load().ppn_last_error().startswith(b"ppn_redact_cells"), lib.load().ppn_last_error()


def _surface(lib, fmt, base=0x100000, **change):
    """A surface the entry would launch on: 6 x 8 pixels, fake (never dereferenced) pointers."""
    h, w = 6, 8
    is420 = fmt in (lib.PPN_PIX_NV12, lib.PPN_PIX_I420)
    row = {lib.PPN_PIX_NV12: w, lib.PPN_PIX_I420: w, lib.PPN_PIX_YUYV: 2 * w, lib.PPN_PIX_BGR24: 3 * w}[fmt]
    s = lib.YuvSurface(format=fmt, height=h, width=w, pitch=row, pitch_c=(w if fmt == lib.PPN_PIX_NV12 else w // 2) if is420 else 0,
                       frame_stride=4096, y=base, u=base + 0x1000 if is420 else None,
                       v=base + 0x2000 if fmt == lib.PPN_PIX_I420 else None, matrix=0, full_range=0)
    for k, v in change.items():
        setattr(s, k, v)
    return s


_ALL, _YUV, _420, _I420 = (0, 1, 2, 3), (0, 1, 2), (0, 1), (1,)
# what, formats, changes of both surfaces, changes of dst alone
SURFACE_REFUSALS = [
    ("NULL y", _ALL, dict(y=None), {}),
    ("NULL u", _420, dict(u=None), {}),
    ("NULL v", _I420, dict(v=None), {}),
    ("format 4", _ALL, dict(format=4), {}),
    ("format -1", _ALL, dict(format=-1), {}),
    ("matrix 2", _YUV, dict(matrix=2), {}),
    ("odd width", _YUV, dict(width=7), {}),
    ("odd height", _420, dict(height=5), {}),
    ("height 0", _ALL, dict(height=0), {}),
    ("width 0", _ALL, dict(width=0), {}),
    ("pitch below the row", _ALL, dict(pitch=7), {}),
    ("pitch below the packed bgr row", (3,), dict(pitch=23), {}),
    ("pitch_c below the row", _420, dict(pitch_c=3), {}),
    ("frame_stride below the plane", _ALL, dict(frame_stride=5 * 8 + 7), {}),
    ("frame_stride 0", _ALL, dict(frame_stride=0), {}),
    ("dst of another format", _ALL, {}, dict(format=None)),
    ("dst of another height", _ALL, {}, dict(height=4)),
    ("dst of another width", _ALL, {}, dict(width=6)),
    ("dst of another matrix", _YUV, {}, dict(matrix=1)),
    ("dst of another range", _YUV, {}, dict(full_range=1)),
    ("dst shares y but not the pitch", _ALL, {}, dict(y=0x100000, pitch=64)),
    ("dst shares y but not the stride", _ALL, {}, dict(y=0x100000, frame_stride=8192)),
    ("dst shares u alone", _420, {}, dict(u=0x101000)),
    ("dst shares v alone", _I420, {}, dict(v=0x102000)),
]


@pytest.mark.parametrize("what,formats,both,dst_only", SURFACE_REFUSALS, ids=[r[0] for r in SURFACE_REFUSALS])
def test_redact_yuv_refuses_what_draw_humans_yuv_refuses_of_a_surface_pair(what, formats, both, dst_only):
    lib = _lib()
    l = lib.load()
    cfg = lib.RedactCfg(16, 0, (C.c_uint8 * 4)(1, 2, 3, 0))
    for fmt in formats:
        src = _surface(lib, fmt, **both)
        if "format" in dst_only:
            dst = _surface(lib, (fmt + 1) % 4, base=0x300000)                 # a good surface of another format
        else:
            dst = _surface(lib, fmt, base=0x300000, **dict(both, **dst_only))
        assert l.ppn_redact_yuv(C.byref(cfg), C.byref(src), C.byref(dst), 2, 0x50000, None) == -1, (what, fmt)
        assert l.ppn_last_error().startswith(b"ppn_redact_yuv"), l.ppn_last_error()


def test_redact_yuv_refuses_bad_arguments_before_any_launch():
    lib = _lib()
    l = lib.load()
    good = lambda: lib.RedactCfg(16, 0, (C.c_uint8 * 4)(1, 2, 3, 0))
    for fmt in _ALL:
        src, dst = _surface(lib, fmt), _surface(lib, fmt, base=0x300000)
        calls = [(None, src, dst, 2, 0x50000), (good(), None, dst, 2, 0x50000), (good(), src, None, 2, 0x50000),
                 (good(), src, dst, 2, None), (good(), src, dst, 0, 0x50000), (good(), src, dst, -1, 0x50000),
                 (good(), src, dst, 65536, 0x50000)]
        for cell in (0, 4, 12, 64, -8):
            calls.append((lib.RedactCfg(cell, 0, (C.c_uint8 * 4)()), src, dst, 2, 0x50000))
        for mode in (2, -1):
            calls.append((lib.RedactCfg(16, mode, (C.c_uint8 * 4)()), src, dst, 2, 0x50000))
        for cfg, s, d, batch, mask in calls:
            ref = lambda x: None if x is None else C.byref(x)
            assert l.ppn_redact_yuv(ref(cfg), ref(s), ref(d), batch, mask, None) == -1, (fmt, batch, mask)
            assert l.ppn_last_error().startswith(b"ppn_redact_yuv"), l.ppn_last_error()
    # packed BGR of an odd size is no refusal of the surface check: the call above failed for its own reason only
    odd = dict(height=5, width=7, pitch=21)
    assert l.ppn_redact_yuv(C.byref(good()), C.byref(_surface(lib, 3, **odd)), C.byref(_surface(lib, 3, base=0x300000, **odd)), 0,
                            0x50000, None) == -1
    assert b"batch" in l.ppn_last_error()


def test_redactor_refuses_bad_arguments_without_a_device():
    from pytorch_pose_proposal_network_amd import redact
    _lib()
    good = dict(streams=2, frames=3, max_humans=36, src_hw=(38, 534), fmt="nv12", device="cpu")
    r = redact.Redactor(**good)
    assert (r.CH, r.CW, r.MW) == (3, 34, 2) and r.cfg.kp_mask == RC.HEAD and r.cfg.hold == 8 and r.cfg.margin == 0.25
    assert r.cfg.fallback == R.FALLBACK_PERSON and r.apply_cfg.mode == R.MOSAIC and r.coords_hw == (38, 534) and r.cfg.sy == 1.0
    assert tuple(r.ttl.shape) == (2, 3, 34) and tuple(r.mask.shape) == (6, 3, 2) and tuple(r.flags.shape) == (6,)
    assert r.fill == R.fill_bytes("nv12", (0, 0, 0))
    y = redact.Redactor(**dict(good, fmt="yuyv", src_hw=(37, 534), parts="person", cell=8, coords_hw=(24, 40), fallback="none",
                               mode="fill", fill_rgb=(200, 30, 90), matrix="bt709", full_range=True, hold=0))
    assert y.cfg.kp_mask == RC.PERSON and (y.CW, y.MW) == (67, 3) and y.cfg.fallback == R.FALLBACK_NONE
    assert (F(y.cfg.sy), F(y.cfg.sx)) == R.scales((37, 534), (24, 40)) and y.fill == R.fill_bytes("yuyv", (200, 30, 90), "bt709", True)
    assert redact.Redactor(**dict(good, fmt="bgr", src_hw=(37, 533), mode="fill", fill_rgb=(1, 2, 3))).fill == (3, 2, 1)
    assert redact.Redactor(**dict(good, parts=("left_ankle", "top"))).cfg.kp_mask == (1 << 11 | 1 << 16)
    for bad in (dict(streams=0), dict(frames=0), dict(max_humans=0), dict(max_humans=1025), dict(fmt="p010"), dict(cell=12),
                dict(cell=0), dict(parts="face"), dict(parts=("nose",)), dict(parts=()), dict(parts=("top",), K=4), dict(margin=-0.5),
                dict(margin=float("nan")), dict(fallback="root"), dict(hold=-1), dict(hold=255), dict(hold=1.5), dict(mode="blur"),
                dict(fill_rgb=(0, 0, 256)), dict(fill_rgb=(0, 0)), dict(coords_hw=(0, 40)), dict(src_hw=(37, 534)),
                dict(src_hw=(38, 533)), dict(src_hw=(38, 16386)), dict(matrix="bt2020"), dict(K=0), dict(K=33),
                dict(streams=4096, frames=16)):
        with pytest.raises(ValueError):
            redact.Redactor(**dict(good, **bad))
    with pytest.raises(ValueError):
        r.cells(None)                                                        # the buffers live on the CPU
