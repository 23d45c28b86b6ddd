"""Planted inputs of the window-merge tests (tests/test_windows_cpu.py on the restatement, tests/test_windows_gpu.py on the
kernel): each builder returns a `Case` -- the windows, the network input size and the packed arrays of a DecodeResult of
frames * n images -- small enough to read, built once and never written."""
from dataclasses import dataclass, field

import numpy as np

import windows_ref as R

F = np.float32
WHOLE = (0, 0, 64, 64)                      # with IN_HW = (64, 64) the mapping is y * 1 + 0: boxes map to themselves
IN_HW = (64, 64)


@dataclass
class Case:
    windows: list
    in_hw: tuple
    frames: int
    M: int
    K: int
    count: np.ndarray = field(init=False)
    kp_cell: np.ndarray = field(init=False)
    bbox: np.ndarray = field(init=False)
    score: np.ndarray = field(init=False)

    def __post_init__(self):
        B = self.frames * len(self.windows)
        self.count = np.zeros(B, np.int32)
        self.kp_cell = np.full((B, self.M, self.K), -1, np.int32)
        self.bbox = np.zeros((B, self.M, self.K, 4), F)
        self.score = np.zeros((B, self.M, self.K), F)

    def add(self, image, root, root_score, kps=None, root_cell=7):
        """Append a person to `image`: root box and score, kps = {j: (box, score)}.  Returns its row p."""
        p = int(self.count[image])
        self.count[image] += 1
        self.kp_cell[image, p, 0], self.bbox[image, p, 0], self.score[image, p, 0] = root_cell, root, root_score
        for j, (box, s) in (kps or {}).items():
            self.kp_cell[image, p, j], self.bbox[image, p, j], self.score[image, p, j] = 3, box, s
        return p

    def freeze(self):
        for a in (self.count, self.kp_cell, self.bbox, self.score):
            a.setflags(write=False)
        return self

    def ref(self, max_out, merge_thr=0.3, fuse=True, out=None, **kw):
        return R.merge(self.windows, self.in_hw, self.count, self.kp_cell, self.bbox, self.score, self.frames, max_out,
                       merge_thr, fuse, out, **kw)


def overlap_person(K=5):
    """A 100 x 160 picture, two 100 x 100 windows that share columns 60..99, network input 50 x 50 (scale 2, exact).  One
    person stands in the overlap: copy A in window 0 (root .9; keypoints 1: .5, 2: .8), copy B in window 1 (root .7;
    keypoints 1: .3, 2: .9, 3: .4); a bystander in window 1 only."""
    c = Case([(0, 0, 100, 100), (0, 60, 100, 100)], (50, 50), 1, 4, K)
    kp = lambda y, x: (y, x, y + 2, x + 2)
    c.add(0, (10, 35, 40, 45), 0.9, {1: (kp(12, 36), 0.5), 2: (kp(20, 38), 0.8)})
    c.add(1, (10, 5, 40, 15), 0.7, {1: (kp(12, 6), 0.3), 2: (kp(20, 8), 0.9), 3: (kp(30, 9), 0.4)})
    c.add(1, (5, 30, 45, 45), 0.6, {4: (kp(8, 33), 0.2)})
    return c.freeze()


def same_window_pair(K=3):
    """Two people of ONE window whose root boxes overlap with IoU 0.67: the decode's NMS has judged them, both survive."""
    c = Case([WHOLE, WHOLE], IN_HW, 1, 4, K)
    c.add(0, (0, 0, 10, 10), 0.9)
    c.add(0, (0, 2, 10, 12), 0.8)
    return c.freeze()


def chain(K=3):
    """A (window 0, .9), B (window 1, .8), C (window 2, .7) in a row: iou(A, B) = iou(B, C) = 7/13, iou(A, C) = 1/4.  B is a
    duplicate of A; C overlaps only B, and a duplicate suppresses nobody: C is kept."""
    c = Case([WHOLE, WHOLE, WHOLE], IN_HW, 1, 2, K)
    c.add(0, (0, 0, 10, 10), 0.9, {1: ((1, 1, 2, 2), 0.1)})
    c.add(1, (0, 3, 10, 13), 0.8, {1: ((1, 4, 2, 5), 0.2)})
    c.add(2, (0, 6, 10, 16), 0.7, {1: ((1, 7, 2, 8), 0.3)})
    return c.freeze()


def equal_scores(K=3):
    """Three copies of one person with equal root scores (one of them -0.0 against +0.0 in a second trio): the lowest (i, p)
    is the keeper, the others its duplicates in (i, p) order."""
    c = Case([WHOLE, WHOLE, WHOLE], IN_HW, 1, 3, K)
    c.add(2, (0, 0, 10, 10), 0.5, {1: ((1, 1, 2, 2), 0.3)})
    c.add(1, (0, 0, 10, 10), 0.5, {1: ((1, 1, 2, 2), 0.3)})
    c.add(0, (0, 0, 10, 10), 0.5, {1: ((1, 1, 2, 2), 0.3)})
    c.add(1, (30, 30, 40, 40), -0.0)
    c.add(0, (30, 30, 40, 40), 0.0)
    c.add(2, (30, 30, 40, 40), 0.0)
    return c.freeze()


def skipped(K=3):
    """Window 0: a rootless person between two good ones and a NaN root score; window 1: a negative count over good-looking
    rows; window 2: a count above max_humans (its M rows take part)."""
    c = Case([WHOLE, WHOLE, WHOLE], IN_HW, 1, 4, K)
    c.add(0, (0, 0, 10, 10), 0.9)
    p = c.add(0, (20, 0, 30, 10), 0.8, {1: ((21, 1, 22, 2), 0.5)})
    c.kp_cell[0, p, 0] = -1
    c.add(0, (40, 0, 50, 10), 0.7)
    c.add(0, (40, 20, 50, 30), np.nan)
    c.add(1, (0, 40, 10, 50), 0.95)
    c.count[1] = -3
    for r in range(4):
        c.add(2, (20 + 10 * r, 40, 28 + 10 * r, 50), 0.6 - 0.1 * r)
    c.count[2] = 9
    return c.freeze()


def crowd(frames=2, M=300, K=3):
    """Frame 0: two windows of 300 people each on a grid of disjoint boxes -- 600 candidates, the first 512 take part and
    all of them are kept; frame 1 is quiet (one person per window, the same one)."""
    c = Case([(0, 0, 64, 64), (0, 0, 64, 64)], IN_HW, frames, M, K)
    rng = np.random.default_rng(5)
    for i in range(2):
        sc = np.sort(rng.random(M).astype(F))[::-1]
        for p in range(M):
            y, x = divmod(i * M + p, 25)
            c.add(i, (2 * y, 2 * x, 2 * y + 1.5, 2 * x + 1.5), sc[p], {1: ((2 * y, 2 * x, 2 * y + 1, 2 * x + 1), 0.5)})
    if frames > 1:
        c.add(2, (0, 0, 10, 10), 0.9)
        c.add(3, (0, 0, 10, 10), 0.8, {2: ((1, 1, 2, 2), 0.4)})
    return c.freeze()


def mixed_batch(M=7, K=18):
    """One batch of n = 2 windows that mixes P = 0, P = M, a count above M, a negative count and rootless people."""
    c = Case([(0, 0, 48, 64), (16, 0, 48, 64)], (48, 64), 3, M, K)
    rng = np.random.default_rng(11)

    def fill(image, P, partner=None):
        sc = np.sort(rng.random(P).astype(F))[::-1]
        for p in range(P):
            y, x = int(rng.integers(16, 30)), int(rng.integers(0, 50))
            kps = {int(j): ((y + j, x, y + j + 2, x + 3), F(rng.random())) for j in rng.choice(np.arange(1, K), 5, False)}
            c.add(image, (y, x, y + 12, x + 10), sc[p], kps)
            if partner is not None:                              # window 1 sees the same person 16 rows higher
                c.add(partner, (y - 16, x, y - 4, x + 10), F(sc[p] * F(0.5)), {1: ((y - 16, x, y - 15, x + 1), 0.99)})
    fill(1, M)                       # frame 0: P = 0 beside P = M
    fill(2, 3, partner=3)            # frame 1: three people, each seen by both windows
    c.kp_cell[2, 1, 0] = -1          # ... one of them rootless in window 0
    fill(4, M, partner=5)            # frame 2: a count above M beside a negative one
    c.count[4] = M + 5
    c.count[5] = -1
    return c.freeze()


def planted(rows=4, cols=4, K=32, M=7, frames=2, people=9, seed=7):
    """A 256 x 256 picture under rows x cols windows of 96 x 96 at the network input 48 x 48 (scale 2, exact): `people`
    per frame at random places; every window that holds a person's root box sees a copy of it, moved by quarter pixels,
    with a random root score and a random half of the keypoints at random scores."""
    ys = [round(i * (256 - 96) / max(rows - 1, 1) / 2) * 2 for i in range(rows)]
    xs = [round(i * (256 - 96) / max(cols - 1, 1) / 2) * 2 for i in range(cols)]
    wins = [(y, x, 96, 96) for y in ys for x in xs]
    c = Case(wins, (48, 48), frames, M, K)
    rng = np.random.default_rng(seed)
    for f in range(frames):
        for _ in range(people):
            y, x = 2 * int(rng.integers(0, 100)), 2 * int(rng.integers(0, 100))
            h, w = 2 * int(rng.integers(10, 28)), 2 * int(rng.integers(6, 20))
            for i, (wy, wx, wh, ww) in enumerate(wins):
                b = f * len(wins) + i
                if not (wy <= y and y + h <= wy + wh and wx <= x and x + w <= wx + ww) or c.count[b] >= M:
                    continue
                j = rng.integers(-2, 3, 4) * 0.25
                root = ((y - wy) / 2 + j[0], (x - wx) / 2 + j[1], (y + h - wy) / 2 + j[2], (x + w - wx) / 2 + j[3])
                kps = {int(k): ((root[0] + k % 5, root[1] + k % 3, root[0] + k % 5 + 2, root[1] + k % 3 + 2), F(rng.random()))
                       for k in rng.choice(np.arange(1, K), (K - 1) // 2, False)}
                c.add(b, root, F(rng.random()), kps)
    # the decode lists an image's people by descending root score
    for b in range(len(c.count)):
        P = int(c.count[b])
        o = np.argsort(-c.score[b, :P, 0], kind="stable")
        for a in (c.kp_cell, c.bbox, c.score):
            a[b, :P] = a[b, :P][o]
    return c.freeze()


def identity(M=6, K=4):
    """One window that is the whole picture at the network's input size: the people come back as they went in."""
    c = Case([(0, 0, 37, 53)], (37, 53), 2, M, K)
    rng = np.random.default_rng(3)
    for f in range(2):
        sc = np.sort(rng.random(M - f).astype(F))[::-1]
        for p in range(M - f):
            b = rng.random(4).astype(F) * F(30)
            c.add(f, (b[0], b[1], b[0] + b[2], b[1] + b[3]), sc[p], {1 + p % (K - 1): (rng.random(4).astype(F), F(rng.random()))})
    return c.freeze()


def threshold_sweep(seed=1, pairs=24, ulps=3, thr=0.3):
    """Root-box pairs within `ulps` f32 steps of iou == thr: per pair, box B's xmax is bisected to the f32 value at which
    iou(A, B) >= thr changes, and one frame is planted for each of the 2 * ulps values around it (A in window 0, B in
    window 1, identity mapping).  Returns (case, ious): the restatement's iou of every frame."""
    rng = np.random.default_rng(seed)
    frames = []
    for _ in range(pairs):
        h, w = F(5 + 20 * rng.random()), F(5 + 20 * rng.random())
        y, x = F(20 * rng.random()), F(20 * rng.random())
        A = np.array([y, x, y + h, x + w], F)
        dy = F(h * F(0.1 * rng.random()))
        B0 = np.array([y + dy, x, y + dy + h, 0], F)
        val = lambda xm: R.iou(A, R.area(A), np.array([B0[0], B0[1], B0[2], xm], F), R.area(np.array([B0[0], B0[1], B0[2], xm], F)))
        lo, hi = F(x + w * F(0.05)), F(x + w)                       # iou grows with xmax on [x, x + w]
        if not (val(lo) < F(thr) <= val(hi)):
            continue
        while np.nextafter(lo, F(np.inf)) < hi:
            mid = F((np.float64(lo) + np.float64(hi)) / 2)
            lo, hi = (lo, mid) if val(mid) >= F(thr) else (mid, hi)
        xm = hi
        for _ in range(ulps):
            xm = np.nextafter(xm, F(-np.inf))
        for _ in range(2 * ulps):
            frames.append((A, np.array([B0[0], B0[1], B0[2], xm], F)))
            xm = np.nextafter(xm, F(np.inf))
    c = Case([WHOLE, WHOLE], IN_HW, len(frames), 2, 2)
    for f, (A, B) in enumerate(frames):
        c.add(2 * f, A, 0.9)
        c.add(2 * f + 1, B, 0.8)
    return c.freeze(), frames


def mapping_sweep(seed=2, M=200, K=2):
    """One window whose scales are not representable (h 100 / 96, w 150 / 96) at an odd origin: 200 random boxes whose
    mapped coordinates a fused multiply-add would round differently in places."""
    c = Case([(37, 21, 100, 150)], (96, 96), 1, M, K)
    rng = np.random.default_rng(seed)
    sc = np.sort(rng.random(M).astype(F))[::-1]
    for p in range(M):
        b = (rng.random(4) * 96).astype(F)
        c.add(0, (min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3])), sc[p], {1: ((rng.random(4) * 96).astype(F), 0.5)})
    return c.freeze()
