"""Shared cases of the re-identification tests: descriptors and track ids built directly, no network and no pixels involved
(the pixel side has its own cases in the test files).

A scenario is dict(cfg=reid_ref.make_cfg(..), seq=[frame, ..]) with a frame a list of (track id, descriptor or None) per
person, in the order of the people list.  `as_case` lays one scenario per stream out as calls of `frames` frames each
(dict(cfg, streams, frames, M, calls=[dict(count, ids, descr, valid, n_frames)])); `run_ref` runs a case through the NumPy
restatement and returns per call (outputs, state after it)."""
import numpy as np

import reid_ref as R

LEN = R.LEN


def flat(b0, b1=0, b2=0):
    """The descriptor of a rectangle of one colour: 1024 in one bin of each of the nine histograms."""
    d = np.zeros((3, 3, 8), np.uint16)
    for ch, q in enumerate((b0, b1, b2)):
        d[:, ch, q] = 1024
    return d.reshape(LEN)


def moved(d, out):
    """`d` with `out` samples in all moved from each histogram's fullest bin to the next bin, spread over the nine histograms:
    its intersection with a flat `d` is exactly 9216 - out."""
    d = d.reshape(9, 8).astype(np.int64)
    for i in range(9):
        k = out // 9 + (1 if i < out % 9 else 0)
        q = int(d[i].argmax())
        assert k <= d[i, q]
        d[i, q] -= k
        d[i, (q + 1) % 8] += k
    return d.reshape(LEN).astype(np.uint16)


A, B_, C_ = flat(0, 0, 0), flat(3, 3, 3), flat(6, 1, 5)             # three colours that intersect in 0
THR = 6452                                                           # ceil(0.7 * 9216)


def scenarios():
    cfg = R.make_cfg
    at = lambda sim: moved(A, R.SIM_MAX - sim)
    sc = {
        # id 5 leaves for one frame; a new track comes with a descriptor whose similarity is exactly thr / one below
        "relink_at_thr": dict(cfg=cfg(thr=THR, shift=0), seq=[[(5, A)], [], [(9, at(THR))]]),
        "born_below_thr": dict(cfg=cfg(thr=THR, shift=0), seq=[[(5, A)], [], [(9, at(THR - 1))]]),
        # tie-breaks: the larger similarity; at equal similarity the smaller lost; then the lower index
        "tie_similarity": dict(cfg=cfg(thr=1000), seq=[[(1, at(8000)), (2, at(9000))], [], [(7, A)]]),
        "tie_lost": dict(cfg=cfg(thr=1000), seq=[[(1, A), (2, A)], [(2, A)], [], [(7, A)]]),
        "tie_index": dict(cfg=cfg(thr=1000), seq=[[(1, A), (2, A)], [], [(7, A)]]),
        # two newcomers, one lost entry: the lower p relinks although the other is more similar, and that one is born
        "two_want_one": dict(cfg=cfg(thr=1000), seq=[[(1, A)], [], [(7, at(5000)), (8, A)]]),
        # min_lost 3: lost 2 is no candidate, lost 3 is
        "min_lost_short": dict(cfg=cfg(thr=0, min_lost=3), seq=[[(1, A)], [], [], [(7, A)]]),
        "min_lost_met": dict(cfg=cfg(thr=0, min_lost=3), seq=[[(1, A)], [], [], [], [(7, A)]]),
        # memory 2: lost == 2 relinks; one frame later the entry was freed the frame before
        "memory_last": dict(cfg=cfg(thr=0, memory=2), seq=[[(1, A)], [], [], [(7, A)]]),
        "memory_gone": dict(cfg=cfg(thr=0, memory=2), seq=[[(1, A)], [], [], [], [(7, A)]]),
        "memory_zero": dict(cfg=cfg(thr=0, memory=0), seq=[[(1, A)], [], [(7, A)]]),
        # an entry born without a descriptor is never a candidate, even at thr 0
        "no_descr_no_candidate": dict(cfg=cfg(thr=0), seq=[[(1, None)], [], [(7, A)]]),
        # a newcomer without a descriptor cannot relink
        "newcomer_without_descr": dict(cfg=cfg(thr=0), seq=[[(1, A)], [], [(7, None)]]),
        # the blend with its rounding term: shift 0 replaces, shift 2 moves a quarter of the way
        "blend_shift0": dict(cfg=cfg(shift=0), seq=[[(1, A)], [(1, moved(A, 1003))], [(1, B_)]]),
        "blend_shift2": dict(cfg=cfg(shift=2), seq=[[(1, A)], [(1, moved(A, 1003))], [(1, B_)], [(1, B_)]]),
        # a bound person without a descriptor keeps the entry's; one born without takes its first as it is
        "bound_without_descr": dict(cfg=cfg(shift=2), seq=[[(1, A)], [(1, None)], [(1, B_)]]),
        "first_descr_later": dict(cfg=cfg(shift=2), seq=[[(1, None)], [(1, B_)], [(1, A)]]),
        # a relinked entry forgets its old track id: when that id shows up again it is a newcomer
        "old_tid_forgotten": dict(cfg=cfg(thr=1000), seq=[[(1, A)], [], [(7, A)], [(7, A), (1, B_)]]),
        # ids <= 0 do not take part
        "non_participants": dict(cfg=cfg(), seq=[[(-1, A), (0, B_), (4, C_)], [(4, C_), (-1, A)]]),
        # three colours, all leave, all come back under new track ids in another order
        "three_return": dict(cfg=cfg(thr=THR), seq=[[(1, A), (2, B_), (3, C_)], [], [], [(9, C_), (8, A), (7, B_)]]),
    }
    return sc


def pack(images, M, Rr):
    """A list of B frames -> count, ids, descr, valid.  Rows beyond a frame's people hold values that must not matter."""
    Bn = len(images)
    count = np.zeros(Bn, np.int32)
    ids = np.full((Bn, M), 77, np.int32)
    descr = np.full((Bn, Rr, LEN), 9, np.uint16)
    valid = np.ones((Bn, Rr), np.int32)
    for b, people in enumerate(images):
        count[b] = len(people)
        for p, (tid, d) in enumerate(people[:M]):
            ids[b, p] = tid
            if p < Rr:
                valid[b, p] = 0 if d is None else 1
                descr[b, p] = 5 if d is None else d
    return dict(count=count, ids=ids, descr=descr, valid=valid, n_frames=None)


def as_case(seqs, cfg, frames, M, cuts=None):
    """One sequence per stream -> calls of `frames` frames; a stream whose sequence has run out gets n_frames 0 (its images
    are filled with people that must not be looked at).  `cuts`: per call the number of frames each stream takes (at most
    `frames`), default: as many as are left."""
    S = len(seqs)
    at = [0] * S
    calls = []
    junk = [(3, A), (4, B_)]
    while any(at[s] < len(seqs[s]) for s in range(S)):
        take = [min(frames, len(seqs[s]) - at[s]) for s in range(S)]
        if cuts is not None:
            take = [min(t, c) for t, c in zip(take, cuts[len(calls)])]
        images = []
        for s in range(S):
            images += seqs[s][at[s]:at[s] + take[s]] + [junk] * (frames - take[s])
            at[s] += take[s]
        call = pack(images, M, cfg["max_rois"])
        call["n_frames"] = None if all(t == frames for t in take) else np.array(take, np.int32)
        calls.append(call)
    return dict(cfg=cfg, streams=S, frames=frames, M=M, calls=calls)


def video(seed, T, n_people=5, p_here=0.7, p_rename=0.15, p_descr=0.9):
    """A seeded sequence: a few people in noisy flat colours who come and go and now and then change their track id."""
    rng = np.random.default_rng(seed)
    colours = [flat(*(int(v) for v in rng.integers(0, 8, 3))) for _ in range(n_people)]
    tids = list(range(1, n_people + 1))
    nxt = n_people + 1
    seq = []
    for _ in range(T):
        frame = []
        for i in rng.permutation(n_people):
            if rng.random() < p_rename:
                tids[i], nxt = nxt, nxt + 1
            if rng.random() < p_here:
                d = moved(colours[i], int(rng.integers(0, 3000))) if rng.random() < p_descr else None
                frame.append((tids[i], d))
        seq.append(frame)
    return seq


def crowd(n=130, M=136, Rr=4):
    """130 track ids in one frame: 128 entries are born, two people overflow; then half of them again."""
    cfg = R.make_cfg(max_rois=Rr, memory=1)
    first = [(1000 + i, A if i % 2 else None) for i in range(n)]
    second = [(1000 + i, B_) for i in range(0, n, 2)]
    return as_case([[first, second, second, first]], cfg, 1, M)


def run_case(case, update, state):
    """`update(case, call, state)` -> outputs; the state is carried by `update`'s side."""
    return [update(case, call, state) for call in case["calls"]]


def run_ref(case, state=None):
    """Per call (outputs, copy of the state after it); the invariant is asserted after every call."""
    st = R.fresh_state(case["streams"]) if state is None else R.copy_state(state)
    steps = []
    for call in case["calls"]:
        out = R.reid_update(case["cfg"], st, call["count"], call["ids"], call["descr"], call["valid"], case["streams"],
                            case["frames"], call["n_frames"])
        R.assert_invariant(st, case["cfg"])
        steps.append((out, R.copy_state(st)))
    return steps


def single(scn, M=7):
    """A scenario as one stream with one frame per call."""
    return as_case([scn["seq"]], scn["cfg"], 1, M)


# ---- three people walk across a small NV12 picture; one is away for longer than the tracker remembers ---------------------
WALK_HW, WALK_K, WALK_M, WALK_R, WALK_MAX_AGE = (144, 160), 4, 7, 5, 2
WALK_COLOURS = ((40, 90, 200), (200, 160, 100), (120, 70, 70))      # (Y, U, V) per person, in three different bins each


def walk():
    """dict(raw u8 [T, nbytes] NV12, calls=[the decode arrays of one frame], away=(first, last frame person 2 is absent),
    T).  Every person is painted in its own flat colour over the rectangle the ROI rules give it; person p of a frame is
    walker p while all three are there (the scores descend)."""
    import crops_ref as CR
    import track_cases as TC
    H, W = WALK_HW
    gap = WALK_MAX_AGE + 3
    T = 3 + gap + 3
    away = (3, 3 + gap - 1)
    nbytes, pitch, pc, uo, _ = R.layout("nv12", H, W)
    raw = np.full((T, nbytes), 128, np.uint8)
    calls, who = [], []
    for t in range(T):
        people, names = [], []
        for i in range(3):
            if i == 2 and away[0] <= t <= away[1]:
                continue
            cx = 20 + 2 * t if not (i == 2 and t > away[1]) else 120 + 2 * (t - away[1])
            people.append(TC.person(24 + 48 * i, cx, WALK_K, score=0.9 - 0.1 * i))
            names.append(i)
        call = TC.pack([people], WALK_M, WALK_K)
        roi, status = CR.people_rois(call["count"], call["kp_cell"], call["bbox"], WALK_HW, 1.0, 1.0, WALK_R, CR.MODE_PEOPLE,
                                     0.0, 0.0, CR.ALIGN["nv12"], 8)
        for p, i in enumerate(names):
            assert status[0, p] == CR.OK
            y0, x0, h, w = (int(v) for v in roi[0, p])
            yy, uu, vv = WALK_COLOURS[i]
            img = raw[t]
            img[:H * pitch].reshape(H, pitch)[y0:y0 + h, x0:x0 + w] = yy
            uv = img[uo:].reshape(H // 2, pc)
            uv[y0 // 2:(y0 + h) // 2, x0:x0 + w:2] = uu
            uv[y0 // 2:(y0 + h) // 2, x0 + 1:x0 + w:2] = vv
        calls.append(call)
        who.append(names)
    return dict(raw=raw, calls=calls, who=who, away=away, T=T)


_WALK = {}


def walk_ref():
    """The walk through the three restatements, once: per frame dict(ids, roi, status, descr, valid, out, state), plus the
    scenario itself under "walk"."""
    if _WALK:
        return _WALK
    import crops_ref as CR
    import track_ref as TR
    w = walk()
    H, W = WALK_HW
    tcfg = TR.make_cfg(K=WALK_K, max_age=WALK_MAX_AGE)
    rcfg = R.make_cfg(thr=THR, max_rois=WALK_R)
    tst, rst = TR.fresh_state(1, WALK_K), R.fresh_state(1)
    steps = []
    for t, call in enumerate(w["calls"]):
        tout = TR.track_update(tcfg, tst, call["count"], call["kp_cell"], call["bbox"], call["score"], 1, 1)
        roi, status = CR.people_rois(call["count"], call["kp_cell"], call["bbox"], WALK_HW, 1.0, 1.0, WALK_R, CR.MODE_PEOPLE,
                                     0.0, 0.0, CR.ALIGN["nv12"], 8)
        descr, valid = R.people_descr(w["raw"][t:t + 1], "nv12", H, W, roi, status)
        out = R.reid_update(rcfg, rst, call["count"], tout["ids"], descr, valid, 1, 1)
        R.assert_invariant(rst, rcfg)
        steps.append(dict(ids=tout["ids"].copy(), roi=roi, status=status, descr=descr, valid=valid, out=out,
                          state=R.copy_state(rst)))
    _WALK.update(walk=w, steps=steps, track_cfg=tcfg, reid_cfg=rcfg)
    return _WALK
