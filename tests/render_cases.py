"""Shared inputs of tests/test_render_cpu.py and tests/test_render_gpu.py: the frames the reference drew
(tests/golden/draw_cases.npz, written by tests/golden/make_draw_golden.py) and hand-made people in the compact layout."""
import functools
import os

import numpy as np

import render_ref as R

K, E = 18, 17
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "draw_cases.npz")
F32 = np.float32


@functools.lru_cache(maxsize=None)
def fixture():
    """(cases, palette, kp_order, edges, pillow_version); a case is a dict of NumPy arrays and flags."""
    g = np.load(GOLDEN)
    cases = []
    for i in range(int(g["n_cases"])):
        cases.append(dict(name=str(g["names"][i]), base=g[f"{i}/base"], count=int(g[f"{i}/count"]),
                          kp_cell=g[f"{i}/kp_cell"], bbox=g[f"{i}/bbox"], visbbox=bool(g[f"{i}/visbbox"]),
                          grid=bool(g[f"{i}/grid"]), grid_step=int(g[f"{i}/grid_step"]), expected=g[f"{i}/expected"]))
    return cases, g["palette"], [int(k) for k in g["kp_order"]], [tuple(int(v) for v in e) for e in g["edges"]], \
        str(g["pillow_version"])


def ref_draw(frames, count, kp_cell, bbox, visbbox=False, grid=False, grid_step=16):
    _, palette, order, edges, _ = fixture()
    return R.draw_ref(frames, count, kp_cell, bbox, order, edges, palette, visbbox, grid, grid_step)


def gradient(B, H, W, seed=0):
    """u8 [B,H,W,3] frames that contain neither a palette colour nor the grid's grey."""
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([np.stack([(x * 3 + 7 * b + seed) % 97 + 1, (y * 5 + 3 * b) % 89 + 2, (x + 2 * y + b) % 83 + 4], -1)
                     for b in range(B)]).astype(np.uint8)


def box(cx, cy, w, h):
    cx, cy, w, h = F32(cx), F32(cy), F32(w), F32(h)
    return np.array([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], F32)


def people(rng, B, M, H, W, n=None, spread=None, missing=0.2, garbage=False):
    """Random people in the compact layout: (count i32[B], kp_cell i32[B,M,K], bbox f32[B,M,K,4]).  `spread` = (cx, cy, r)
    keeps every keypoint within r of a point; absent slots hold NaN / huge boxes when `garbage` is set."""
    count = np.full(B, M if n is None else n, np.int32)
    kp_cell = np.full((B, M, K), -1, np.int32)
    bbox = np.zeros((B, M, K, 4), F32)
    if garbage:
        bbox[...] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e9, -7e8, 12.5], F32), bbox.shape)
    for b in range(B):
        for m in range(M):
            for k in range(K):
                if k and rng.random() < missing:
                    continue
                if spread is None:
                    cx, cy = rng.uniform(-10, W + 10), rng.uniform(-10, H + 10)
                else:
                    cx, cy = spread[0] + rng.uniform(-spread[2], spread[2]), spread[1] + rng.uniform(-spread[2], spread[2])
                kp_cell[b, m, k] = int(rng.integers(0, 36))
                bbox[b, m, k] = box(cx, cy, rng.uniform(0.5, 30), rng.uniform(0.5, 30))
    return count, kp_cell, bbox
