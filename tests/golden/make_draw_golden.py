"""Generate tests/golden/draw_cases.npz by running the REFERENCE's own draw_humans (datatest.py:162-232) through the
installed Pillow (reference checkout only; it is imported, never copied).

Usage:  python tests/golden/make_draw_golden.py

Every case stores the base frame, the people in the compact decode layout (count, kp_cell, bbox), the flags, and the frame
the reference drew; the palette, the paint order of the keypoints and the Pillow version are stored once.  People are
built as dicts in config.kp_paint_order() -- the order get_humans_by_feature inserts keypoints in -- and one case takes
its people from the reference's get_humans_by_feature on a 6 x 6 head, which pins that order.  Root boxes are at least
three pixels in each extent (the reference raises below that), and boxes drawn with visbbox at least one pixel high.
The script checks tests/render_ref.py against every frame before writing.
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

import make_golden as MG  # noqa: E402

import numpy as np  # noqa: E402

from pytorch_pose_proposal_network_amd import config as cfg, synth  # noqa: E402
from oracle import decode_ref as D  # noqa: E402
import render_ref as R  # noqa: E402

SIZES = [(96, 96), (64, 96), (96, 64)]          # (H, W)
ORDER = cfg.kp_paint_order()
F32 = np.float32


def base_frame(H, W, i):
    """A compressible frame: three gradients in steps of eight pixels, shifted per case (no colour of the palette and not
    the grid's grey, so every drawn pixel differs from the base)."""
    y, x = np.mgrid[0:H, 0:W]
    x, y = x // 8, y // 8
    frame = np.stack([(x * 16 + 17 * i) % 200 + 3, (y * 16 + 5 * i) % 200 + 7, ((x + y) * 8 + 29 * i) % 200 + 11],
                     -1).astype(np.uint8)
    used = [tuple(c) for c in cfg.COLOR_MAP.values()] + [R.GRID_COLOUR]
    assert not any((frame == np.array(c, np.uint8)).all(-1).any() for c in used)
    return frame


def box(cx, cy, w, h):
    cx, cy, w, h = F32(cx), F32(cy), F32(w), F32(h)
    return np.array([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], F32)


def person(rng, H, W, lo=-12.0, hi=12.0, missing=0.25, at=None):
    hm = {}
    for k in ORDER:
        if k and rng.random() < missing:
            continue
        cx, cy = (rng.uniform(lo, W + hi), rng.uniform(lo, H + hi)) if at is None else \
            (at[0] + rng.uniform(-14, 14), at[1] + rng.uniform(-14, 14))
        hm[k] = box(cx, cy, rng.uniform(3.5, 40), rng.uniform(3.5, 40))
    return hm


def build_cases(datatest):
    rng = np.random.default_rng(20240611)
    cases = []                                   # (name, H, W, humans, visbbox, gridOn)
    for i in range(12):                          # random people reaching over every border, with negative coordinates
        H, W = SIZES[i % 3]
        humans = [person(rng, H, W) for _ in range(1 + i % 4)]
        cases.append((f"random{i}", H, W, humans, bool(i // 3 % 2), i >= 9))
    for j, (H, W) in enumerate(SIZES):
        # wholly outside the frame on each side, beside one person inside
        outside = [person(rng, H, W, at=c) for c in ((-60, H / 2), (W + 60, H / 2), (W / 2, -70), (W / 2, H + 70))]
        cases.append((f"outside{j}", H, W, outside[:3] + [person(rng, H, W, 10, -10)], False, False))
        # people with a root only
        only_root = [{0: box(W / 2, H / 2, 30, 20)}, {0: box(2, 3, 9, 11)}, {0: box(W - 1, H - 2, 8, 8)}]
        cases.append((f"rootonly{j}", H, W, only_root, bool(j % 2), False))
        # overlapping people: the same pose shifted by a pixel or two, painter's order decides
        first = person(rng, H, W, 8, -8, missing=0.1)
        shifted = [{k: b + F32(d) for k, b in first.items()} for d in (1.0, 2.5)]
        cases.append((f"overlap{j}", H, W, [first] + shifted, False, j == 2))
        cases.append((f"overlap_vis{j}", H, W, [first] + shifted, True, j == 1))
        # zero-length limbs: neck and thorax (and an elbow / wrist pair) share their truncated centre
        hm = person(rng, H, W, 10, -10, missing=0.0)
        names = cfg.KEYPOINT_NAMES
        hm[names.index("thorax")] = hm[names.index("neck")] + F32(0.25)
        hm[names.index("left_wrist")] = box(20.75, 30.5, 6, 6)
        hm[names.index("left_elbow")] = box(20.25, 30.25, 9, 4)
        cases.append((f"zerolimb{j}", H, W, [hm], False, False))
    # people decoded by the reference itself from a 6 x 6 head (pins the dicts' insertion order)
    datatest.insize, datatest.outsize, datatest.gridsize = (96, 96), (6, 6), (16, 16)
    datatest.inW = datatest.inH = 96
    datatest.outW = datatest.outH = 6
    for seed in (7, 8):
        head = synth.planted_crowd_head(seed, n_people=4, n_decoys=1, out_hw=(6, 6))
        humans, _ = datatest.get_humans_by_feature(*D.split_head(head), detection_thresh=0.15)
        assert humans, "the planted head decoded to nobody"
        for hm in humans:
            keys = list(hm.keys())
            assert keys == [k for k in ORDER if k in hm], f"dict order {keys} is not the paint order"
        cases.append((f"decoded{seed}", 96, 96, humans, False, seed == 8))
    datatest.outW = 24                           # draw_humans' grid step is int(width / outW) with the module's default
    return cases


def compact(humans):
    n = len(humans)
    kp_cell = np.full((max(n, 1), cfg.K), -1, np.int32)
    bbox = np.zeros((max(n, 1), cfg.K, 4), F32)
    for i, hm in enumerate(humans):
        for k, b in hm.items():
            kp_cell[i, k] = 0
            bbox[i, k] = b
    return np.int32(n), kp_cell, bbox


def main():
    import PIL
    from PIL import Image
    _, _, datatest = MG.import_reference()
    assert [tuple(datatest.COLOR_MAP[n]) for n in datatest.KEYPOINT_NAMES] == [cfg.COLOR_MAP[n] for n in cfg.KEYPOINT_NAMES]
    assert [list(e) for e in datatest.EDGES] == cfg.EDGES
    palette = np.array([cfg.COLOR_MAP[n] for n in cfg.KEYPOINT_NAMES], np.uint8)
    cases = build_cases(datatest)
    out = dict(n_cases=len(cases), palette=palette, kp_order=np.array(ORDER, np.int32), edges=np.array(cfg.EDGES, np.int32),
               pillow_version=PIL.__version__, names=np.array([c[0] for c in cases]))
    for i, (name, H, W, humans, visbbox, grid_on) in enumerate(cases):
        base = base_frame(H, W, i)
        drawn = datatest.draw_humans(datatest.KEYPOINT_NAMES, datatest.EDGES, Image.fromarray(base.copy()), humans,
                                     visbbox=visbbox, gridOn=grid_on)
        expected = np.array(drawn)
        count, kp_cell, bbox = compact(humans)
        step = int(W / datatest.outW)
        mine = R.draw_ref(base[None], [count], kp_cell[None], bbox[None], ORDER, cfg.EDGES, palette, visbbox, grid_on, step)[0]
        diff = int((mine != expected).any(-1).sum())
        print(f"{name}: {H}x{W}, {len(humans)} people, visbbox {visbbox}, grid {grid_on}: "
              f"{int((expected != base).any(-1).sum())} pixels drawn, restatement differs in {diff}")
        assert diff == 0, name
        out.update({f"{i}/base": base, f"{i}/count": count, f"{i}/kp_cell": kp_cell, f"{i}/bbox": bbox,
                    f"{i}/visbbox": np.int32(visbbox), f"{i}/grid": np.int32(grid_on), f"{i}/grid_step": np.int32(step),
                    f"{i}/expected": expected})
    path = os.path.join(HERE, "draw_cases.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(cases)} cases, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
