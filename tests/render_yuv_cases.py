"""Shared inputs of tests/test_render_yuv_cpu.py and tests/test_render_yuv_gpu.py: hand-placed people that put the chroma rule
of ppn_draw_humans_yuv (include/ppn.h: the first painted pixel of a group in row-major order) on the spot, and raw frames.

How a single pixel gets painted: a root (keypoint 0) whose box lies inside one pixel is a one-pixel outline whatever
`visbbox` says; with visbbox set a keypoint k > 0 with such a box is one too, and a limb between two of them at the same
pixel is the zero-length limb, painted after both.  Without visbbox a keypoint k > 0 is a disc of 4 or 5 pixels each way, so
the lone pixel of those cases is the root's."""
import numpy as np

import render_cases as RC
import yuv_ref as Y

K = RC.K
H, W = 18, 34                                   # the smallest frame of the GPU test: less than one tile, W % 4 == 2


def tiny(x, y):
    """A box inside pixel (x, y)."""
    return np.array([y + 0.25, x + 0.25, y + 0.75, x + 0.75], np.float32)


def span(x0, y0, x1, y1):
    """The box whose outline is the pixel box [x0, y0, x1, y1]."""
    return np.array([y0 + 0.5, x0 + 0.5, y1 + 0.5, x1 + 0.5], np.float32)


def pack_people(people, M=None):
    """[{keypoint: box}] of ONE image -> (count i32[1], kp_cell i32[1,M,K], bbox f32[1,M,K,4])."""
    M = max(len(people), 1) if M is None else M
    kp_cell = np.full((1, M, K), -1, np.int32)
    bbox = np.zeros((1, M, K, 4), np.float32)
    for i, hm in enumerate(people):
        for k, b in hm.items():
            kp_cell[0, i, k], bbox[0, i, k] = 1, b
    return np.array([len(people)], np.int32), kp_cell, bbox


def anchor_cases():
    """[(name, people, visbbox, grid_step, wrong rules the case tells from the right one)] on an H x W frame."""
    edges = RC.fixture()[3]
    s, t = edges[0]
    a, b, c = [k for k in range(1, K) if k not in (s, t)][:3]
    # a disc around (10, 10) covers [8, 12]^2 without its corners: in the group (8..9, 8..9) the top-left pixel is bare, the
    # other three carry the disc's colour -- until a later person's one-pixel root takes (9, 9)
    two_f = [{a: RC.box(10.5, 10.5, 1, 1)}, {0: tiny(9, 9)}]
    # group (8..9, 8..9): three colours at (8, 9), (9, 8) and (9, 9), the top-left pixel bare; row 9 is a YUYV pair of two colours
    two_t = [{a: tiny(9, 8)}, {b: tiny(8, 9)}, {c: tiny(9, 9)}]
    borders = [{0: tiny(W - 1, H - 1)}, {0: tiny(W - 1, 3)}, {0: tiny(5, H - 1)}]
    return [
        ("bottom-right only, zero-length limb", [{s: tiny(7, 5), t: tiny(7, 5)}], True, 0, {"topleft"}),
        ("bottom-right only, one-pixel root", [{0: tiny(7, 5)}], False, 0, {"topleft"}),
        ("two colours in a group, discs", two_f, False, 0, {"topleft", "last"}),
        ("two colours in a group, boxes", two_t, True, 0, {"topleft", "last"}),
        ("last row pair and last column pair", borders, False, 0, {"topleft"}),
        ("last row pair and last column pair, boxes", borders, True, 0, {"topleft"}),
        ("one-pixel outline on odd rows and columns", [{a: span(3, 3, 11, 9)}], True, 0, {"topleft"}),
        ("root outline from an odd corner", [{0: span(3, 3, 11, 9)}], False, 0, {"topleft"}),
        ("grid at step 16 over two colours", two_f, False, 16, {"topleft", "last"}),
        ("grid at step 5", [], False, 5, {"topleft"}),
        ("grid at step 5 over boxes", two_t, True, 5, {"topleft", "last"}),
    ]


def raw_frames(rng, fmt, F, h, w, pitch=None, tail=0):
    """Random raw frames u8 [F, frame bytes + tail]: every byte random, pitch padding and tail included."""
    return rng.integers(0, 256, (F, Y.frame_bytes(fmt, h, w, pitch) + tail), dtype=np.uint8)
