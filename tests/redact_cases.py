"""Pictures, planted people and hold sequences for the redaction (tests/redact_ref.py, csrc/redact.hip), test infrastructure
only.  The arrays are read-only: every test takes copies.  `self_check` (run by tests/test_redact_cpu.py) asserts that the
cases reach every situation they are meant to."""
import numpy as np

import redact_ref as R

F = np.float32
# 3 frames each.  Cell 16: CW = 34, two mask words with two bits in the second, the last column 6 (BGR: 5) pixels wide and the
# last row 6 (YUYV, BGR: 5) high.  Cell 8: CW = 67, three words.  Cell 32: CW = 17.
PICTURES = {"nv12": (38, 534), "i420": (38, 534), "yuyv": (37, 534), "bgr": (37, 533)}
FRAMES = 3
COORDS_HW = (24, 40)            # the space the boxes are in: 38 / 24, 534 / 40, ... are not representable
M, K = 6, 18
NECK, TOP, ANKLE = 15, 16, 11
HEAD = 1 << NECK | 1 << TOP
PERSON = (1 << K) - 1
HOLDS = (0, 1, 3)
CELLS = (8, 16, 32)


class Case:
    def __init__(self, frames):
        self.frames = frames
        self.count = np.zeros(frames, np.int32)
        self.kp_cell = np.full((frames, M, K), -1, np.int32)
        self.bbox = np.zeros((frames, M, K, 4), F)
        self.score = np.zeros((frames, M, K), F)

    def person(self, f, p, body, head=None, absent=(), **boxes):
        """Person p of frame f: every keypoint's box is `body` (ymin, xmin, ymax, xmax in COORDS_HW pixels), neck and top
        get `head` (None: they are absent); `boxes` replaces single keypoints' boxes by index ("k11=(..)"); `absent`
        keypoints keep their box but have kp_cell -1."""
        for j in range(K):
            self.bbox[f, p, j] = body
            self.kp_cell[f, p, j] = 7 * p + j
            self.score[f, p, j] = 0.5
        for j in (NECK, TOP):
            if head is None:
                self.kp_cell[f, p, j] = -1
            else:
                self.bbox[f, p, j] = head
        for name, b in boxes.items():
            self.bbox[f, p, int(name[1:])] = b
        for j in absent:
            self.kp_cell[f, p, j] = -1
        return self

    def freeze(self):
        for a in (self.count, self.kp_cell, self.bbox, self.score):
            a.setflags(write=False)
        return self


def planted():
    """3 frames of people in COORDS_HW.  Frame 0 (count 6): two overlapping people, one in the partial border cells of both
    axes (its bit lies in the last mask word), one in the middle (cell 8: the second word), one without neck and top (the
    fallbacks differ), one without a root.  Frame 1 (count 9 above max_humans 6): wholly outside, an inverted box, a NaN and
    an infinity in a used box, the same in an unused box, a person whose right edge is a multiple of every cell size (its last
    column is (r - 1) / cell, not r / cell).  Frame 2: count -3 over rows that look like people."""
    H, W = COORDS_HW
    nan, inf = np.nan, np.inf
    c = Case(FRAMES)
    c.count[:] = (6, 9, -3)
    c.person(0, 0, (4.0, 2.0, 20.0, 7.0), head=(4.2, 3.1, 7.9, 5.2))
    c.person(0, 1, (5.0, 3.5, 21.0, 9.0), head=(5.5, 4.4, 8.6, 6.7))                       # overlaps person 0
    c.person(0, 2, (H - 9.0, W - 4.0, H + 2.0, W + 1.0), head=(H - 2.3, W - 0.9, H - 0.1, W - 0.05))   # the last row and column
    c.person(0, 3, (6.0, 20.0, 22.0, 25.0), head=(6.3, 21.2, 9.1, 23.4))                   # the middle of the row
    c.person(0, 4, (10.0, 12.0, 23.0, 16.0))                                               # no neck, no top
    c.person(0, 5, (1.0, 28.0, 23.0, 36.0), head=(1.0, 30.0, 5.0, 34.0), absent=(0,))      # no root: no person
    c.person(1, 0, (-30.0, W + 20.0, -10.0, W + 30.0), head=(-29.0, W + 22.0, -25.0, W + 26.0))        # wholly outside
    c.person(1, 1, (3.0, 10.0, 20.0, 14.0), head=(9.0, 13.0, 4.0, 11.0))                   # inverted: ymax < ymin, xmax < xmin
    c.person(1, 2, (3.0, 15.0, 20.0, 19.0), head=(4.0, 16.0, 7.0, 18.0), k15=(4.0, nan, 7.0, 18.0))    # NaN in a used box
    c.person(1, 3, (3.0, 21.0, 20.0, 25.0), head=(4.0, 22.0, 7.0, 24.0), k16=(4.0, 22.0, inf, 24.0))   # infinity in a used box
    c.person(1, 4, (3.0, 27.0, 20.0, 31.0), head=(4.0, 28.0, 7.0, 30.0), k11=(nan, 27.0, inf, 31.0))   # both in an unused box
    c.person(1, 5, (3.0, 33.0, 20.0, 37.0), head=(4.0, 34.0, 7.0, 35.705))                 # right edge 479.5 -> r = 480 = 15 * 32
    for p in range(M):
        c.person(2, p, (2.0, 1.0 + 6 * p, 22.0, 5.0 + 6 * p), head=(2.5, 2.0 + 6 * p, 6.0, 4.0 + 6 * p))
    return c.freeze()


def random_people(seed, frames=FRAMES):
    """Heads and bodies of all sizes, many reaching over the picture, some keypoints absent."""
    rng = np.random.default_rng(seed)
    H, W = COORDS_HW
    c = Case(frames)
    c.count[:] = rng.integers(0, M + 1, frames)
    for f in range(frames):
        for p in range(M):
            cy, cx, s = rng.uniform(-2, H + 2), rng.uniform(-2, W + 2), rng.uniform(0.3, 4)
            c.person(f, p, (cy - 2 * s, cx - s, cy + 2 * s, cx + s),
                     head=None if rng.random() < 0.2 else (cy - 2 * s, cx - s / 3, cy - s, cx + s / 3),
                     absent=tuple(j for j in range(1, K) if rng.random() < 0.2))
    return c.freeze()


STREAMS, STEPS = 2, 5


def hold_sequence():
    """2 streams x 5 frames (image s * 5 + t).  Stream 0: person A (left) is there at t = 0 only -- its cells are covered, then
    uncovered for `hold` frames and for one more with hold 1 and 3; person B (right) is there at t = 0 and again at t = 2,
    while its cells count down.  Stream 1: nobody at t = 0, A at t = 1 and t = 4, B at t = 3."""
    c = Case(STREAMS * STEPS)
    A = dict(body=(4.0, 4.0, 20.0, 9.0), head=(4.5, 5.0, 8.0, 7.5))
    B = dict(body=(6.0, 26.0, 22.0, 31.0), head=(6.5, 27.0, 10.0, 29.5))
    plan = {0: [A, B], 1: [], 2: [B], 3: [], 4: [], 5: [], 6: [A], 7: [], 8: [B], 9: [A]}
    for b, people in plan.items():
        c.count[b] = len(people)
        for p, who in enumerate(people):
            c.person(b, p, **who)
    return c.freeze()


def frames_of(fmt, seed, pitch=None, extra=0, frames=FRAMES):
    """Random raw frames u8 [frames, frame bytes + extra] of PICTURES[fmt]."""
    h, w = PICTURES[fmt]
    return np.random.default_rng(seed).integers(0, 256, (frames, R.frame_bytes(fmt, h, w, pitch) + extra), dtype=np.uint8)


def padded_pitch(fmt):
    """A pitch above the row's bytes (even, as I420 needs; not a multiple of 4: the byte-store path)."""
    w = PICTURES[fmt][1]
    return {"nv12": w + 12, "i420": w + 12, "yuyv": 2 * w + 10, "bgr": 3 * w + 7}[fmt]


def random_mask(fmt, cell, seed, frames=FRAMES, garbage=True):
    """u32 [frames, CH, MW]: every cell masked with probability 1/3; `garbage`: the bits at and above CW are random."""
    CH, CW, MW = R.grid_of(PICTURES[fmt], cell)
    rng = np.random.default_rng(seed)
    m = np.zeros((frames, CH, MW), np.uint32)
    for f, cy, cx in zip(*np.nonzero(rng.random((frames, CH, CW)) < 1 / 3)):
        m[f, cy, cx >> 5] |= np.uint32(1 << (cx & 31))
    if garbage and CW % 32:
        m[:, :, -1] |= rng.integers(0, 2 ** 32, (frames, CH), dtype=np.uint64).astype(np.uint32) & np.uint32((0xffffffff << (CW % 32)) & 0xffffffff)
    return m


def cells_args(fmt, cell, kp_mask=HEAD, fallback=R.FALLBACK_PERSON, margin=0.25, hold=0):
    """The restatement's keyword arguments for a picture of `fmt`."""
    sy, sx = R.scales(PICTURES[fmt], COORDS_HW)
    return dict(src_hw=PICTURES[fmt], cell=cell, sy=sy, sx=sx, kp_mask=kp_mask, fallback=fallback, margin=margin, hold=hold)


def self_check():
    """The cases reach what they are meant to (asserts)."""
    case = planted()
    a = cells_args("nv12", 16)
    why = {(f, p): R.person_cells(case.kp_cell[f, p], case.bbox[f, p], a["src_hw"], 16, a["sy"], a["sx"], HEAD)
           for f in range(FRAMES) for p in range(M)}
    CH, CW, MW = R.grid_of(PICTURES["nv12"], 16)
    assert (CH, CW, MW) == (3, 34, 2) and R.grid_of(PICTURES["nv12"], 8)[1:] == (67, 3) and R.grid_of(PICTURES["bgr"], 32)[1:] == (17, 1)
    r0, r1 = why[0, 0][0], why[0, 1][0]
    assert r0 and r1 and max(r0[0], r1[0]) <= min(r0[1], r1[1]) and max(r0[2], r1[2]) <= min(r0[3], r1[3])   # overlapping
    assert why[0, 2][0][1] == CH - 1 and why[0, 2][0][3] == CW - 1 and CW - 1 >= 32            # partial cells, the second word
    r8 = R.person_cells(case.kp_cell[0, 3], case.bbox[0, 3], a["src_hw"], 8, a["sy"], a["sx"], HEAD)[0]
    assert 32 <= r8[2] and r8[3] < 64                                                           # cell 8: the middle word
    assert why[0, 4][2] == "fallback" and R.person_cells(case.kp_cell[0, 4], case.bbox[0, 4], a["src_hw"], 16, a["sy"], a["sx"],
                                                         HEAD, R.FALLBACK_NONE)[2] == "none"
    assert case.kp_cell[0, 5, 0] < 0
    assert why[1, 0][1:] == (False, "empty") and why[1, 1][1:] == (False, "empty")              # outside; inverted
    assert why[1, 2][1:] == (True, "box") and why[1, 3][1:] == (True, "box")                    # NaN, infinity in a used box
    assert why[1, 4][1:] == (False, "ok") and not np.isfinite(case.bbox[1, 4, ANKLE]).all()     # ... in an unused box
    assert R.person_cells(case.kp_cell[1, 4], case.bbox[1, 4], a["src_hw"], 16, a["sy"], a["sx"], PERSON)[1:] == (True, "box")
    for cell in CELLS:                                                                          # r = 480: a multiple of the cell
        one = [R.person_cells(case.kp_cell[1, 5], case.bbox[1, 5], a["src_hw"], cell, a["sy"], a["sx"], HEAD, rule=r)[0] for r in (None, "last_col")]
        assert one[0][3] == 480 // cell - 1 and one[1][3] == 480 // cell
    assert case.count[1] > M and case.count[2] < 0 and (case.kp_cell[2, :, 0] >= 0).all()
    mask, flags, _ = R.cells(case.count, case.kp_cell, case.bbox, None, FRAMES, 1, **a)
    assert flags.tolist() == [0, R.FLAG_BAD_BOX, 0] and not mask[2].any() and mask[0].any() and mask[1].any()
    assert mask[0, :, 1].any()                                                                  # a bit in the second word
    # the hold sequences: per hold, a cell of A in stream 0 is on for exactly 1 + hold frames and off for the rest; a cell of
    # B is covered again while it counts down
    seq = hold_sequence()
    ra = R.person_cells(seq.kp_cell[0, 0], seq.bbox[0, 0], a["src_hw"], 16, a["sy"], a["sx"], HEAD)[0]
    rb = R.person_cells(seq.kp_cell[0, 1], seq.bbox[0, 1], a["src_hw"], 16, a["sy"], a["sx"], HEAD)[0]
    for hold in HOLDS:
        ttl = np.zeros((STREAMS, CH, CW), np.uint8)
        on_a, on_b, life_b = [], [], []
        for t in range(STEPS):                                                                  # frame by frame: the ttl trace
            idx = [s * STEPS + t for s in range(STREAMS)]
            m, _, ttl = R.cells(seq.count[idx], seq.kp_cell[idx], seq.bbox[idx], ttl, STREAMS, 1, **dict(a, hold=hold))
            on_a.append(R.bit(m[0], ra[0], ra[2]))
            on_b.append(R.bit(m[0], rb[0], rb[2]))
            life_b.append(0 if ttl is None else int(ttl[0, rb[0], rb[2]]))
        assert on_a == [t <= hold for t in range(STEPS)], (hold, on_a)                          # hold frames more, then off
        assert on_b == [t <= hold or 2 <= t <= 2 + hold for t in range(STEPS)], (hold, on_b)
        if hold == 3:
            assert life_b == [4, 3, 4, 3, 2]                                                    # reloaded while counting down
    return True
