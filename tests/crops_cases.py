"""Planted and random people for the ROI rule (tests/crops_ref.py, csrc/crops.hip), test infrastructure only.  The arrays
are read-only: every test takes copies."""
import itertools

import numpy as np

F = np.float32
SRC_HW = (64, 96)               # the picture the ROIs are cut from
COORDS_HW = (24, 40)            # the space the boxes are in: sy = 64 / 24 and sx = 96 / 40 are not representable
M, K = 6, 5


class Case:
    def __init__(self, frames):
        self.frames = frames
        self.count = np.zeros(frames, np.int32)
        self.kp_cell = np.full((frames, M, K), -1, np.int32)
        self.bbox = np.zeros((frames, M, K, 4), F)
        self.score = np.zeros((frames, M, K), F)

    def person(self, f, p, boxes, absent=()):
        """Person p of frame f with keypoint j in boxes[j] (ymin, xmin, ymax, xmax in COORDS_HW pixels); `absent` keypoints
        keep their box but have kp_cell -1."""
        for j, b in enumerate(boxes):
            self.bbox[f, p, j] = b
            self.kp_cell[f, p, j] = -1 if j in absent else 7 * p + j
            self.score[f, p, j] = 0.5
        return self

    def freeze(self):
        for a in (self.count, self.kp_cell, self.bbox, self.score):
            a.setflags(write=False)
        return self


def _around(cy, cx, rng, n=K, spread=3.0, size=2.0):
    """n keypoint boxes scattered around (cy, cx); box 0 (the root) is the largest."""
    out = [(cy - 2 * size, cx - size, cy + 2 * size, cx + size)]
    for _ in range(n - 1):
        y, x = cy + rng.uniform(-spread, spread), cx + rng.uniform(-spread, spread)
        out.append((y - size / 2, x - size / 2, y + size / 2, x + size / 2))
    return out


def planted(seed=0):
    """3 frames.  Frame 0: five people (more than a max_rois of 4), one in each corner of the picture reaching over it and one
    inside.  Frame 1: count 9 above max_humans 6 -- a box wholly outside, a zero-area box, a NaN box, an absent root, a
    person whose absent keypoints carry wild boxes, an infinite box.  Frame 2: count -3 over rows that look like people."""
    rng = np.random.default_rng(seed)
    H, W = COORDS_HW
    c = Case(3)
    c.count[:] = (5, 9, -3)
    for p, (cy, cx) in enumerate(((1.5, 1.0), (2.0, W - 1.5), (H - 1.0, 2.5), (H - 2.5, W - 0.5), (H / 2 + 0.3, W / 2 - 0.7))):
        c.person(0, p, _around(cy, cx, rng))
    c.person(1, 0, _around(-20.0, W + 30.0, rng))                                        # wholly outside
    c.person(1, 1, [(7.25, 9.5, 7.25, 9.5)] * K)                                         # zero area: a 1 x 1 hull at most
    nan = _around(10.0, 20.0, rng)
    nan[3] = (9.0, np.nan, 11.0, 21.0)                                                   # a NaN in a keypoint (union mode)
    c.person(1, 2, nan)
    c.person(1, 3, _around(12.0, 12.0, rng), absent=(0,))                                # an absent root: no person
    wild = _around(14.0, 30.0, rng)
    wild[2], wild[4] = (-500.0, -500.0, 900.0, 900.0), (np.nan, np.inf, -np.inf, 3.0)    # absent: must not be read into the box
    c.person(1, 4, wild, absent=(2, 4))
    inf = _around(8.0, 8.0, rng)
    inf[0] = (2.0, 3.0, np.inf, 9.0)                                                     # an infinity in the root box
    c.person(1, 5, inf)
    for p in range(M):
        c.person(2, p, _around(12.0, 5.0 + 6 * p, rng))
    return c.freeze()


def nan_root():
    """One frame, one person whose ROOT box holds the NaN (mode root sees it too)."""
    c = Case(1)
    c.count[:] = 1
    c.person(0, 0, [(np.nan, 3.0, 9.0, 9.0)] + [(4.0, 4.0, 6.0, 6.0)] * (K - 1))
    return c.freeze()


def random_people(seed, frames=4):
    """Boxes of all sizes, many reaching over the picture, some keypoints absent."""
    rng = np.random.default_rng(seed)
    H, W = COORDS_HW
    c = Case(frames)
    c.count[:] = rng.integers(0, M + 1, frames)
    for f, p in itertools.product(range(frames), range(M)):
        boxes = _around(rng.uniform(-4, H + 4), rng.uniform(-4, W + 4), rng, spread=rng.uniform(0.5, 8), size=rng.uniform(0.1, 6))
        c.person(f, p, boxes, absent=tuple(j for j in range(1, K) if rng.random() < 0.3))
    return c.freeze()


# mode, margin, keep_aspect, (align_y, align_x), max_rois (4: below frame 0's people; 8: above max_humans)
CONFIGS = [(mode, margin, keep, align, max_rois)
           for mode in (0, 1) for margin, keep in ((0.0, False), (0.1, True), (0.25, False), (0.0, True))
           for align, max_rois in (((1, 1), 4), ((2, 2), 8), ((1, 2), 8))]
OUT_HW = (12, 8)                # aspect 8 / 12: not representable
