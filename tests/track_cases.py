"""Seeded generators of tracking cases: count / kp_cell / bbox / score arrays built directly, no network involved.

A case is dict(cfg=track_ref.make_cfg(..), streams, frames, M, calls=[dict(count, kp_cell, bbox, score, n_frames)]): the
calls run in order on one tracker.  `run_ref` runs a case through the NumPy restatement once and keeps the result, so the
CPU tests and the GPU tests share one reference per case."""
import numpy as np

import track_ref as R

F = np.float32
H, W = 40.0, 24.0                      # a person's root box; the default gate radius is 0.1 * sqrt(H * W) = 3.1 pixels


def person(cy, cx, K=18, h=H, w=W, score=0.9, present=None, kp_shift=(0.0, 0.0)):
    """(kp_cell i32[K], bbox f32[K,4], score f32[K]): a root box centred at (cy, cx) and keypoints 1..K-1 at fixed places
    inside it (6 x 6 boxes), moved by kp_shift (dy, dx) relative to the root."""
    kp = np.full(K, -1, np.int32)
    bb = np.zeros((K, 4), F)
    sc = np.zeros(K, F)
    for k in range(K):
        if present is not None and k not in present:
            continue
        kp[k], sc[k] = 100 + k, score
        if k == 0:
            bb[0] = (cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2)
        else:
            y = cy + ((k * 7) % 11 / 11.0 - 0.5) * 0.8 * h + kp_shift[0]
            x = cx + ((k * 5) % 7 / 7.0 - 0.5) * 0.8 * w + kp_shift[1]
            bb[k] = (y - 3, x - 3, y + 3, x + 3)
    return kp, bb, sc


def pack(images, M, K, counts=None):
    """A list of images, each a list of person() tuples -> the four arrays of one call; people beyond M are dropped from
    the arrays (the count still names them unless `counts` overrides it).  Unused rows hold values that must not matter."""
    B = len(images)
    count = np.zeros(B, np.int32)
    kp_cell = np.full((B, M, K), 7, np.int32)                       # rows >= count claim present keypoints: never read
    bbox = np.full((B, M, K, 4), 5.0, F)
    score = np.full((B, M, K), 0.99, F)
    for b, people in enumerate(images):
        count[b] = len(people) if counts is None or counts[b] is None else counts[b]
        for p, (kp, bb, sc) in enumerate(people[:M]):
            kp_cell[b, p], bbox[b, p], score[b, p] = kp, bb, sc
    return dict(count=count, kp_cell=kp_cell, bbox=bbox, score=score, n_frames=None)


def _case(cfg, streams, frames, M, calls):
    return dict(cfg=cfg, streams=streams, frames=frames, M=M, calls=calls)


def _drift_sequence(seed, n_people, T, K, step=2.0):
    """n_people well separated people, each drifting by up to `step` pixels per frame and axis: T images."""
    rng = np.random.default_rng(seed)
    start = np.array([(60.0 + 90.0 * (i // 3), 50.0 + 80.0 * (i % 3)) for i in range(n_people)])
    vel = rng.uniform(-step, step, (n_people, 2))
    return [[person(start[i, 0] + vel[i, 0] * t, start[i, 1] + vel[i, 1] * t, K, score=0.9 - 0.1 * i)
             for i in range(n_people)] for t in range(T)]


def drift(M, K=18, **cfg):
    """Three people drifting a few pixels per frame for 12 frames, one call per frame."""
    seq = _drift_sequence(1, 3, 12, K)
    return _case(R.make_cfg(K=K, **cfg), 1, 1, M, [pack([img], M, K) for img in seq])


def absence(M, gap, max_age=2, K=18):
    """Two people; the second is absent for `gap` frames after frame 1, then returns where it was."""
    a = lambda t: person(60 + t, 50, K, score=0.9)
    b = person(200, 150, K, score=0.8)
    seq = [[a(0), b], [a(1), b]] + [[a(2 + g)] for g in range(gap)] + [[a(2 + gap), b]]
    return _case(R.make_cfg(K=K, max_age=max_age), 1, len(seq), M, [pack(seq, M, K)])


def close_beats_iou(M, K=18):
    """Tracks A and B; the person of frame 1 has A's root box (iou 1 with A, none with B) and B's keypoints."""
    A, B = person(60, 50, K, score=0.9), person(60, 130, K, score=0.8)
    kp, bb, sc = person(60, 130, K, score=0.9)
    bb[0] = A[1][0]
    return _case(R.make_cfg(K=K), 1, 2, M, [pack([[A, B], [(kp, bb, sc)]], M, K)])


def equal_keys(M, K=18):
    """Two identical tracks, then one identical person: the lowest slot takes it."""
    A = person(60, 50, K)
    return _case(R.make_cfg(K=K), 1, 2, M, [pack([[A, A], [A]], M, K)])


def iou_breaks_ties(M, K=18):
    """Two overlapping root-only tracks (n_close 0 with anybody), then a person nearer to the second: the larger iou."""
    A, B = person(60, 50, K, present={0}), person(60, 60, K, score=0.8, present={0})
    return _case(R.make_cfg(K=K), 1, 2, M, [pack([[A, B], [person(60, 58, K, present={0})]], M, K)])


def two_want_one(M, K=18):
    """One track, then two people on top of it: the lower p takes it, the other starts a track."""
    return _case(R.make_cfg(K=K), 1, 2, M, [pack([[person(60, 50, K)], [person(61, 51, K, score=0.9),
                                                                      person(60, 50, K, score=0.8)]], M, K)])


def freed_slot_reused(M, K=18):
    """max_age 0: A (slot 0) vanishes in frame 1 while a new person appears; frame 2 brings one more."""
    A, B = person(60, 50, K), person(200, 150, K, score=0.8)
    C, Dn = person(60, 250, K, score=0.7), person(200, 300, K, score=0.6)
    return _case(R.make_cfg(K=K, max_age=0), 1, 3, M, [pack([[A, B], [B, C], [B, C, Dn]], M, K)])


def smoothing(M, alpha, K=18):
    """One person moving for four frames, a keypoint that comes and goes."""
    seq = [[person(60 + 1.7 * t, 50 - 1.3 * t, K, present=None if t != 1 else set(range(K)) - {5})] for t in range(4)]
    return _case(R.make_cfg(K=K, alpha=alpha), 1, 4, M, [pack(seq, M, K)])


def chunking(M, layout, K=18):
    """The same three 12-frame sequences as 12 calls of (1, 1) each, one call of (1, 12) each, or three calls of (3, 4).
    Returns a list of cases (one per tracker) and, per case, which sequence each of its streams follows."""
    seqs = [_drift_sequence(10 + i, 2 + i, 12, K, step=2.5) for i in range(3)]
    for i, seq in enumerate(seqs):                                  # people come and go, so that ageing and births happen
        for t in (4, 5):
            seq[t] = seq[t][1:]
        seq[8 + i] = seq[8 + i] + [person(300, 40 + 60 * i, K, score=0.3)]
    cfg = R.make_cfg(K=K, max_age=3, alpha=0.5)
    if layout == "frames":
        return [_case(cfg, 1, 1, M, [pack([img], M, K) for img in seq]) for seq in seqs]
    if layout == "sequence":
        return [_case(cfg, 1, 12, M, [pack(seq, M, K)]) for seq in seqs]
    assert layout == "streams"
    return [_case(cfg, 3, 4, M, [pack([seqs[s][c * 4 + t] for s in range(3) for t in range(4)], M, K) for c in range(3)])]


def birth_threshold(M, K=18):
    """birth_thr 0.5: the people of score 0.4 never start a track, those of 0.6 do."""
    seq = [[person(60, 50, K, score=0.6), person(200, 150, K, score=0.4), person(60, 250, K, score=0.5)]] * 3
    return _case(R.make_cfg(K=K, birth_thr=0.5), 1, 3, M, [pack(seq, M, K)])


def small_k(M, max_age):
    """K = 3, with the given max_age: people that come, go and return."""
    K = 3
    seq = _drift_sequence(5, 4, 8, K)
    seq[2], seq[3], seq[4] = seq[2][:2], seq[3][:2], seq[4][:3]
    return _case(R.make_cfg(K=K, max_age=max_age, min_close=2), 2, 4, M,
                 [pack(seq[:4] + seq[4:], M, K), pack(seq[4:] + seq[:4], M, K)])


def large_k(M):
    """K = 32: the widest kernel instantiation (and, at M >= 225, more than 64 KB of LDS)."""
    K = 32
    seq = _drift_sequence(6, 3, 4, K)
    return _case(R.make_cfg(K=K, alpha=0.25), 1, 4, M, [pack(seq, M, K)])


# ---- knife edges: one stream per point, frame 0 starts the track, frame 1 brings the person to be gated -------------------
GATE, IOU_THR = 0.31, 0.37


def _point_box(y, x):
    return (y, x, y, x)                                             # its centre is (x, y) exactly


def gate_sweep(n=192, seed=3):
    """Points whose squared distance to the track's keypoint 1 lies within a few ulps of r2.  The track's keypoint is at
    the origin, so dx and dy are the person's coordinates themselves; root boxes are disjoint (iou 0 < iou_thr = 1) and
    min_close is 1: the person continues the track (id 1) iff the gate holds, otherwise it starts track 2."""
    rng = np.random.default_rng(seed)
    K = 3
    root = np.array((100.0, 100.0, 137.3, 121.7), F)
    r2 = F(F(F(GATE) * F(GATE)) * R.area(root))
    images, pts = [], []
    for i in range(n):
        dy = F(rng.uniform(0.1, 0.95) * np.sqrt(float(r2)))
        dx = F(np.sqrt(float(r2) - float(dy) ** 2))
        for _ in range(int(rng.integers(0, 3))):                    # 0..2 ulps up, then 1 down: -1..+1 around the edge
            dx = np.nextafter(dx, F(np.inf))                        # (one ulp of dx moves dx * dx by about two of its own)
        dx = np.nextafter(dx, F(0))
        kp = np.array((1, 1, -1), np.int32)
        sc = np.full(K, 0.9, F)
        b0 = np.zeros((K, 4), F); b0[0] = root; b0[1] = _point_box(0, 0)
        b1 = np.zeros((K, 4), F); b1[0] = (300, 300, 340, 324); b1[1] = _point_box(dy, dx)
        images += [[(kp, b0, sc)], [(kp, b1, sc)]]
        pts.append((dx, dy))
    cfg = R.make_cfg(K=K, iou_thr=1.0, kp_gate=GATE, min_close=1)
    return _case(cfg, n, 2, 7, [pack(images, 7, K)]), np.array(pts, F), r2


def iou_sweep(n=192, seed=4):
    """People whose root box shares the track's rows and left edge and is 1 / thr times as wide, within a few ulps: the IoU
    lies at the threshold.  Only the root is present, so n_close is 0 and the IoU alone decides."""
    rng = np.random.default_rng(seed)
    K = 3
    images, boxes = [], []
    for i in range(n):
        h, w = F(rng.uniform(20, 60)), F(rng.uniform(10, 40))
        w2 = F(float(w) / IOU_THR)
        for _ in range(int(rng.integers(0, 5))):
            w2 = np.nextafter(w2, F(np.inf))
        w2 = np.nextafter(np.nextafter(w2, F(0)), F(0))
        kp = np.array((1, -1, -1), np.int32)
        sc = np.full(K, 0.9, F)
        b0 = np.zeros((K, 4), F); b0[0] = (0, 0, h, w)
        b1 = np.zeros((K, 4), F); b1[0] = (0, 0, h, w2)
        images += [[(kp, b0, sc)], [(kp, b1, sc)]]
        boxes.append((b0[0], b1[0]))
    cfg = R.make_cfg(K=K, iou_thr=IOU_THR, min_close=31)
    return _case(cfg, n, 2, 7, [pack(images, 7, K)]), boxes


# ---- one batch of edge conditions (GPU tests) --------------------------------------------------------------------------
def _grid_people(n, K, pitch=30.0, present=(0, 1, 2), per_row=20, h=20.0, w=12.0):
    """n well separated small people (root boxes do not touch), descending score."""
    return [person(20 + pitch * (i // per_row), 20 + pitch * (i % per_row), K, h=h, w=w, score=0.95 - 0.002 * i,
                   present=set(present)) for i in range(n)]


def edge_batch(M, K=18):
    """Five streams of three frames with n_frames = (3, 2, 0, 3, 1):
       stream 0   an empty image; 70 separated people into the empty tracker (at M >= 70: 64 tracked, SLOT_OVERFLOW); a
                  negative count
       stream 1   count == M (at M = 300: 300 > 256, DET_OVERFLOW, ids past 256 are -1); count > M; a frame not processed
       stream 2   idle
       stream 3   five people, one of them without a root, drifting over three frames
       stream 4   one frame processed, two not"""
    crowd70 = _grid_people(70, K)
    full = _grid_people(M, K)
    five = lambda t: [person(60 + 90 * i + t, 50 + 1.5 * t, K, score=0.9 - 0.1 * i,
                             present=None if i != 1 else set(range(1, K))) for i in range(5)]
    three = [person(60, 50 + 80 * i, K) for i in range(3)]
    images = [[], crowd70, three,
              full, full, three,
              three, three, three,
              five(0), five(1), five(2),
              three, three, three]
    counts = [None, None, -5,
              M, M + 100, None,
              None, None, None,
              None, None, None,
              None, None, None]
    call = pack(images, M, K, counts)
    call["n_frames"] = np.array((3, 2, 0, 3, 1), np.int32)
    return _case(R.make_cfg(K=K, max_age=2), 5, 3, M, [call])


_REF = {}


def run_ref(name, case, state=None):
    """The restatement's (outputs, flags, state copy) after every call of the case, computed once per `name`.  `state`: the
    tracker's state before the first call (default: fresh)."""
    if name not in _REF:
        st = R.fresh_state(case["streams"], case["cfg"]["K"]) if state is None else R.copy_state(state)
        steps = []
        out = R.fresh_outputs(case["streams"] * case["frames"], case["M"], case["cfg"]["K"])
        for c in case["calls"]:                                     # one set of output buffers, as a Tracker has: the rows
            R.track_update(case["cfg"], st, c["count"], c["kp_cell"], c["bbox"], c["score"], case["streams"],
                           case["frames"], c["n_frames"], out=out)  # of out_xy a call does not write keep the last call's
            steps.append(({k: v.copy() for k, v in out.items()}, R.copy_state(st)))
        _REF[name] = steps
    return _REF[name]


def chunking_views(M, run):
    """Per layout and sequence: ids, hits, xy, live of the 12 frames and the final state of its stream.  `run(name, case)`
    gives the steps of a case.  The rows of xy beyond an image's people are not written, so they are left out (zeroed)."""
    views = {}
    for layout in ("frames", "sequence", "streams"):
        cases = chunking(M, layout)
        for i in range(3):
            case = cases[0 if layout == "streams" else i]
            name = f"chunk/{layout}/{M}" if layout == "streams" else f"chunk/{layout}{i}/{M}"
            rows = [i * 4 + t for t in range(4)] if layout == "streams" else slice(None)
            steps, outs = run(name, case), []
            for (out, _), call in zip(steps, case["calls"]):
                o = {k: out[k][rows].copy() for k in ("ids", "hits", "xy", "live")}
                o["xy"][np.arange(M)[None, :] >= np.clip(call["count"][rows], 0, M)[:, None]] = 0
                outs.append(o)
            state = {k: v[i if layout == "streams" else 0] for k, v in steps[-1][1].items()}
            views[layout, i] = ({k: np.concatenate([o[k] for o in outs]) for k in outs[0]}, state)
    return views


def assert_chunking_invariant(views):
    for i in range(3):
        ref_out, ref_state = views["frames", i]
        assert ref_out["ids"].shape[0] == 12 and ref_out["ids"].max() >= 3 + i          # births beyond the first frame
        for layout in ("sequence", "streams"):
            out, state = views[layout, i]
            for k in ref_out:
                assert out[k].tobytes() == ref_out[k].tobytes(), (layout, i, k)
            for k in ref_state:
                assert np.asarray(state[k]).tobytes() == np.asarray(ref_state[k]).tobytes(), (layout, i, k)
