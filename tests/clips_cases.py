"""Seeded generators of clip cases: count / kp_cell / bbox / score / ids / xy arrays built directly, no network and no tracker
involved (the ids are planted; positive ids are distinct within an image, as the tracker's are).

A case is dict(cfg=clips_ref.make_cfg(..), streams, frames, M, calls=[dict(count, kp_cell, bbox, score, ids, xy, n_frames)]):
the calls run in order on one PoseClips, a gather after every call.  `run_ref` runs a case through the NumPy restatement
once and keeps the result, so the CPU tests and the GPU tests share one reference per case."""
import numpy as np

import clips_ref as R

F = np.float32
BIG = F(3.0e8)                         # finite garbage: it may reach `ref` through an absent root, where arithmetic happens


def blank(M, K):
    """One image whose every entry is garbage that must not matter: rows claim present keypoints and positive ids."""
    return dict(count=0, kp_cell=np.full((M, K), 7, np.int32), bbox=np.full((M, K, 4), 5.25, F),
                score=np.full((M, K), 0.99, F), ids=np.arange(1, M + 1, dtype=np.int32), xy=np.full((M, K, 2), 9.75, F))


def put(img, p, pid, coords, present=None):
    """Person `pid` into row p of the image: every keypoint in `present` (default: all) gets the box (y - 3, x - 3, y + 3,
    x + 3) around coords[k] = (x, y) and score 0.5 + k / 100; the others are absent and keep the image's garbage."""
    img["ids"][p] = pid
    for k in range(img["kp_cell"].shape[1]):
        if present is not None and k not in present:
            img["kp_cell"][p, k] = -1
            continue
        x, y = coords[k]
        img["kp_cell"][p, k], img["score"][p, k] = 100 + k, 0.5 + k / 100
        img["bbox"][p, k] = (y - 3, x - 3, y + 3, x + 3)
        img["xy"][p, k] = (x, y)
    return img


def random_image(rng, M, K, count):
    """M random people, none of whom takes part yet: ids 0 and below in the rows < count, positive ids past them (they must
    not matter).  Keypoints are present with probability 0.7 (the root: 0.97); coordinates are uniform doubles rounded to
    f32, so sums, differences and quotients of them are not representable in general; root boxes are proper boxes.  Garbage
    is planted at the absent keypoints -- NaN in xy, NaN or 123.5 in score, NaN in bbox -- and must not leak into the ring.
    The box of an absent ROOT is finite garbage: the rules copy it into `ref`, where arithmetic happens."""
    here = rng.random((M, K)) < 0.7
    here[:, 0] |= rng.random(M) < 0.9
    kp_cell = np.where(here, rng.integers(0, 500, (M, K)), rng.choice((-1, -7, -2 ** 31), (M, K))).astype(np.int32)
    bbox = rng.uniform(0.0, 384.0, (M, K, 4)).astype(F)
    lo = rng.uniform(0.0, 200.0, (M, 2))
    bbox[:, 0] = np.concatenate([lo, lo + rng.uniform(1.0, 180.0, (M, 2))], 1).astype(F)
    xy = rng.uniform(0.0, 384.0, (M, K, 2)).astype(F)
    score = rng.uniform(0.0, 1.0, (M, K)).astype(F)
    xy[~here], bbox[~here] = np.nan, np.nan
    score[~here] = np.where(rng.random(int((~here).sum())) < 0.5, np.nan, 123.5)
    bbox[~here[:, 0], 0] = (BIG, -BIG, F(17.3), BIG)
    ids = rng.choice((0, -1, -5), M).astype(np.int32)
    ids[max(count, 0):] = np.arange(1, M + 1)[max(count, 0):]
    return dict(count=count, kp_cell=kp_cell, bbox=bbox, score=score, ids=ids, xy=xy)


def pack(images, M, K, n_frames=None, with_xy=True):
    call = {k: np.stack([np.asarray(img[k]) for img in images]) for k in ("kp_cell", "bbox", "score", "ids", "xy")}
    call["count"] = np.array([img["count"] for img in images], np.int32)
    if not with_xy:
        call["xy"] = None
    call["n_frames"] = None if n_frames is None else np.asarray(n_frames, np.int32)
    return call


def _case(cfg, streams, frames, M, calls):
    return dict(cfg=cfg, streams=streams, frames=frames, M=M, calls=calls)


POOL = (1, 2, 3, 7, 2 ** 31 - 1, 64, 65, 1000)


def video(seed, n, M, K, p_here=0.6):
    """n images of one stream: up to min(M, 8) identities that come and go in runs (so that gaps both within and beyond a
    small max_gap occur), at random rows among people with ids 0 and below, with count anywhere up to M."""
    rng = np.random.default_rng(seed)
    pool = POOL[:min(M, len(POOL))]
    on = rng.random(len(pool)) < 0.7
    images = []
    for t in range(n):
        on = np.where(rng.random(len(pool)) < 0.35, rng.random(len(pool)) < p_here, on)
        on[0] = True                                                # one clip fills up and wraps
        if len(pool) > 1:
            on[1] = t % 5 != 3                                      # gaps of exactly one frame
        here = [pid for pid, o in zip(pool, on) if o]
        rng.shuffle(here)
        count = int(rng.integers(len(here), M + 1))
        rows = np.sort(rng.choice(count, len(here), replace=False)).astype(int)
        img = random_image(rng, M, K, count)
        img["ids"][rows] = here
        images.append(img)
    return images


def geometry(M, K, T, max_gap, norm=R.NORM_ROOT, with_xy=True):
    """Three streams of one frame per call with n_frames (1, 0, -2), 2T + 1 calls: every value of pos occurs at a gather,
    the rings wrap twice."""
    seed = 1000 * M + 100 * K + 10 * T + max_gap
    n = 2 * T + 1
    vids = [video(seed + s, n, M, K) for s in range(3)]
    calls = [pack([vids[s][t] for s in range(3)], M, K, (1, 0, -2), with_xy) for t in range(n)]
    return _case(R.make_cfg(K, T, max_gap, norm), 3, 1, M, calls)


def frames3(M, K=3, T=3, max_gap=1, with_xy=True, norm=R.NORM_ROOT):
    """Three streams of three frames per call, n_frames (3, 0, -1), (2, 3, 1) and (0, 1, 3): frames of one stream in one
    call, images that are not processed, a stream idle in one call and busy in the next; counts below 0 and above M."""
    vids = [video(50 + M + s, 9, M, K) for s in range(3)]
    over = vids[1][3]                                               # count > M: every row is listed; the upper half takes part
    over["ids"][M // 2:] = 2000 + np.arange(M // 2, M)              # distinct, and none of the video's
    vids[0][1]["count"], over["count"], vids[2][4]["count"] = -3, M + 100, 0
    nf = ((3, 0, -1), (2, 3, 1), (0, 1, 3))
    calls = [pack([vids[s][3 * c + t] for s in range(3) for t in range(3)], M, K, nf[c], with_xy) for c in range(3)]
    return _case(R.make_cfg(K, T, max_gap, norm), 3, 3, M, calls)


def ref_edges(norm=R.NORM_ROOT):
    """Root boxes under the normalisation: degenerate (a point), inverted on both axes, flat (h = 0 < w: s = w), upright
    (w < 0 < h: s = h), and a proper one; one person per stream, two frames, K = 3, T = 2."""
    K, M = 3, 7
    roots = ((50, 60, 50, 60), (90, 80, 40, 30), (20, 30, 20, 77.7), (10, 90, 33.3, 40), (10.1, 20.2, 70.7, 50.5))
    rng = np.random.default_rng(77)
    images = []
    for root in roots:
        for t in range(2):
            img = random_image(rng, M, K, 2)
            img["ids"][:2], img["bbox"][1, 0] = (0, 5), root
            img["kp_cell"][1, 1] = 3                                # at least one present keypoint besides the root
            img["xy"][1, 1] = (F(101.3), F(77.1))
            img["bbox"][1, 1] = (F(70.3), F(98.1), F(83.9), F(104.5))
            img["score"][1, 1] = 0.625
            images.append(img)
    return _case(R.make_cfg(K, 2, 0, norm), len(roots), 2, M, [pack(images, M, K)])


def crowd70(M=300, K=3, T=2):
    """70 distinct ids in one frame into empty clips: 64 births, 6 rows of -1 and the flag; the same 70 again (64 seen, no
    free slot for the 6); an empty frame with max_gap 0 frees everything; 5 of the 6 take slots 0..4."""
    rng = np.random.default_rng(70)
    def crowd(ids):
        img = random_image(rng, M, K, len(ids) + 3)
        for j, pid in enumerate(ids):
            img["ids"][j + (j > 10) + (j > 40)] = pid               # two non-participants in between
        return img
    ids = np.arange(501, 571)
    empty = blank(M, K)
    images = [crowd(ids), crowd(ids), empty, crowd(ids[65:])]
    return _case(R.make_cfg(K, T, 0), 1, 1, M, [pack([img], M, K) for img in images])


# ---- chunking: the same three videos cut three ways -------------------------------------------------------------------
N_CHUNK = 12
CUTS = ((5, 5, 2, 0), (3, 4, 5, 0), (0, 5, 5, 2))                   # per stream the frames it takes of each mixed call


def chunking(M, layout, K=3, T=5, max_gap=1):
    """`frames`: 12 calls of (1, 1) per video; `sequence`: one call of (1, 12) per video; `mixed`: four calls of (3, 5)
    with n_frames = CUTS[.][call], the images past n_frames holding other frames of the video (they must not matter)."""
    vids = [video(900 + M + s, N_CHUNK, M, K) for s in range(3)]
    cfg = R.make_cfg(K, T, max_gap)
    if layout == "frames":
        return [_case(cfg, 1, 1, M, [pack([img], M, K) for img in v]) for v in vids]
    if layout == "sequence":
        return [_case(cfg, 1, N_CHUNK, M, [pack(v, M, K)]) for v in vids]
    assert layout == "mixed"
    calls, done = [], [0, 0, 0]
    for c in range(4):
        images = []
        for s in range(3):
            images += [vids[s][(done[s] + t) % N_CHUNK] for t in range(5)]
            done[s] += CUTS[s][c]
        calls.append(pack(images, M, K, [CUTS[s][c] for s in range(3)]))
    return [_case(cfg, 3, 5, M, calls)]


_REF = {}


def run_case(case, push, gather, state):
    """Every call of the case: push(call), gather(), state() -> [(out_row, (x, ids, len), state copy)]."""
    steps = []
    for c in case["calls"]:
        row = push(c)
        steps.append((row, gather(), state()))
    return steps


def ref_steps(case, state=None):
    """The restatement's (out_row, gather outputs, state copy) after every call of the case.  `state`: the clips' state
    before the first call (default: fresh)."""
    cfg, S = case["cfg"], case["streams"]
    st = R.fresh_state(S, cfg["K"], cfg["length"]) if state is None else R.copy_state(state)
    return run_case(
        case,
        lambda c: R.clip_push(cfg, st, c["count"], c["kp_cell"], c["bbox"], c["score"], c["ids"], c["xy"], S,
                              case["frames"], c["n_frames"]),
        lambda: R.clip_gather(cfg, st, S), lambda: R.copy_state(st))


def run_ref(name, case):
    """ref_steps of the case from fresh clips, computed once per `name`."""
    if name not in _REF:
        _REF[name] = ref_steps(case)
    return _REF[name]


def chunking_views(M, run):
    """Per layout and video: the final state of its stream and its final gather outputs.  `run(name, case)` gives the steps
    of a case."""
    views = {}
    for layout in ("frames", "sequence", "mixed"):
        cases = chunking(M, layout)
        for i in range(3):
            mixed = layout == "mixed"
            steps = run(f"chunk/{layout}/{M}" if mixed else f"chunk/{layout}{i}/{M}", cases[0 if mixed else i])
            _, (x, ids, length), st = steps[-1]
            s = i if mixed else 0
            views[layout, i] = dict({k: v[s] for k, v in st.items()}, x=x[s], out_id=ids[s], out_len=length[s])
    return views


def assert_chunking_invariant(views):
    for i in range(3):
        ref = views["frames", i]
        assert ref["pos"] == N_CHUNK % 5 and (ref["id"] != 0).any() and ref["x"].any()
        for layout in ("sequence", "mixed"):
            for k, v in ref.items():
                assert np.asarray(views[layout, i][k]).tobytes() == np.asarray(v).tobytes(), (layout, i, k)
