"""GPU: ppn_pckh_match held bit for bit -- scores, labels, counts, flag word, untouched rows -- to its NumPy restatement
(tests/validate_ref.py, which tests/test_validate_cpu.py pins to evaluate.assign_gt_multi and the reference's AP values),
and validate.Validator end to end against the host route (to_humans() + evaluate.evaluation)."""
import os

import numpy as np
import pytest
import torch

import validate_ref as R
from validate_cases import pack_people, person_at, threshold_sweep
from pytorch_pose_proposal_network_amd import evaluate, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M = 7                                        # the golden seeds hold at most 6 people per image
SCORE_FILL, LABEL_FILL, COUNT_FILL = -7.0, 9, -3


def _mods():
    from pytorch_pose_proposal_network_amd import decode, validate
    return decode, validate


def _result(people, dev="cuda"):
    decode, _ = _mods()
    count, kp_cell, bbox, score = (torch.from_numpy(a).to(dev) for a in people)
    B, m = kp_cell.shape[:2]
    return decode.DecodeResult(count=count, kp_cell=kp_cell, limb_arg=torch.zeros(B, m, 17, dtype=torch.int32, device=dev),
                               bbox=bbox, score=score, max_humans=m)


def _fresh_records(validate, n, m):
    rec = validate.Records(n, m)
    rec.score.fill_(SCORE_FILL); rec.label.fill_(LABEL_FILL); rec.count.fill_(COUNT_FILL)
    return rec


def _run_both(people, tables, index, thresh=0.5):
    """(kernel outputs, restatement outputs) as (score, label, count, flags), both over sentinel-filled records."""
    _, validate = _mods()
    xy, head, counts = tables
    n, m = len(counts), people[1].shape[1]
    index = np.asarray(index, np.int32)
    gt = validate.GroundTruth.from_arrays(xy, head, counts)
    rec = _fresh_records(validate, n, m)
    validate.match_people(_result(people), gt, torch.from_numpy(index).cuda(), rec, thresh)
    got = rec.to_host()
    rs, rl, rc = np.full((n, m, 17), SCORE_FILL, np.float32), np.full((n, m, 17), LABEL_FILL, np.uint8), \
        np.full(n, COUNT_FILL, np.int32)
    flags = R.pckh_match(*people, xy, head, counts, index, rs, rl, rc, thresh)
    return got, (rs, rl, rc, flags)


def _assert_same(got, exp, tag=""):
    assert got[3] == exp[3], (tag, "flags", got[3], exp[3])
    assert np.array_equal(got[2], exp[2]), (tag, "count", got[2], exp[2])
    assert got[0].tobytes() == exp[0].tobytes(), (tag, "score", int((got[0] != exp[0]).sum()))
    assert np.array_equal(got[1], exp[1]), (tag, "label", int((got[1] != exp[1]).sum()))


def _same_ap(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def _tables(obj):
    counts = np.array([len(b) for b in obj[4]], np.int32)
    gmax = max(1, int(counts.max()))
    xy = np.zeros((len(counts), gmax, 17, 2), np.float32)
    head = np.zeros((len(counts), gmax), np.float32)
    for i, (kps, boxes) in enumerate(zip(obj[1], obj[4])):
        if len(boxes):
            xy[i, :len(boxes)] = np.asarray(kps, np.float32).reshape(-1, 17, 2)
            head[i, :len(boxes)] = evaluate._head_sizes(boxes)
    return xy, head, counts


def _golden():
    g = np.load(os.path.join(GOLDEN, "eval_cases.npz"), allow_pickle=False)
    return [(int(s), int(n), np.asarray(ap, np.float64)) for s, n, ap in zip(g["seeds"], g["sizes"], g["ap"])]


@pytest.mark.parametrize("seed,n,ap", _golden())
def test_golden_eval_cases(seed, n, ap):
    obj = synth.eval_case(seed, n)
    assert max(len(h) for h in obj[2]) <= M
    got, exp = _run_both(pack_people(obj[2], obj[3], M), _tables(obj), np.arange(n))
    _assert_same(got, exp, seed)
    vals = evaluate.metrics_from_records(got[0], got[1], got[2], _tables(obj)[2])
    assert np.allclose(vals, ap, rtol=0, atol=1e-9), (seed, vals, ap)


def _gt_person(rng, lo=40, hi=340):
    return rng.uniform(lo, hi, (17, 2)).astype(np.float32)


def test_edge_images_in_one_batch():
    """P = 0 with G > 0; G = 0 with P > 0; a padding image; P = 1 against G = Gmax = 64; P = M exactly; count > M; a head
    size of 0 -- one batch, image rows permuted, one row of the tables that no image addresses."""
    rng = np.random.default_rng(11)
    m, gmax, n = 5, 64, 8
    xy, head, counts = np.zeros((n, gmax, 17, 2), np.float32), np.zeros((n, gmax), np.float32), np.zeros(n, np.int32)
    humans, scores = [[] for _ in range(7)], [[] for _ in range(7)]
    index = np.array([5, 2, -1, 0, 6, 1, 3], np.int32)

    def add_gt(row, g, pts, hd):
        xy[row, g], head[row, g] = pts, hd
        counts[row] = max(counts[row], g + 1)

    def add_person(b, pts, **kw):
        hm, sm = person_at(pts, **kw)
        humans[b].append(hm); scores[b].append(sm)

    # batch image 0 -> row 5: no people, two ground-truth people
    add_gt(5, 0, _gt_person(rng), 20); add_gt(5, 1, _gt_person(rng), 25)
    # batch image 1 -> row 2: two people, no ground truth
    add_person(1, _gt_person(rng)); add_person(1, _gt_person(rng))
    # batch image 2: padding, three people; row 4 and row 7 are addressed by nobody
    for _ in range(3):
        add_person(2, _gt_person(rng))
    add_gt(4, 0, _gt_person(rng), 20)
    # batch image 3 -> row 0: one person near ground-truth person 37 of 64
    for g in range(gmax):
        add_gt(0, g, _gt_person(rng), 10 + g % 7)
    add_person(3, xy[0, 37] + np.float32(1.5), score=0.7)
    # batch image 4 -> row 6: exactly M people on three ground-truth people
    for g in range(3):
        add_gt(6, g, _gt_person(rng), 30)
    for p in range(m):
        add_person(4, xy[6, p % 3] + rng.uniform(-12, 12, (17, 2)).astype(np.float32), score=0.2 + 0.1 * p)
    # batch image 5 -> row 1: M + 3 people, only the first M are read; the LAST one sits exactly on ground truth 0
    add_gt(1, 0, _gt_person(rng), 30); add_gt(1, 1, _gt_person(rng), 30)
    for p in range(m + 2):
        add_person(5, xy[1, p % 2] + rng.uniform(-14, 14, (17, 2)).astype(np.float32))
    add_person(5, xy[1, 0])
    # batch image 6 -> row 3: head size 0 (0 / 0 for the person on it, x / 0 for the other) beside a proper one
    add_gt(3, 0, _gt_person(rng), 0); add_gt(3, 1, _gt_person(rng), 18)
    add_person(6, xy[3, 0]); add_person(6, xy[3, 0] + np.float32(3)); add_person(6, xy[3, 1] + np.float32(2))

    people = pack_people(humans, scores, m)
    assert people[0].tolist() == [0, 2, 3, 1, m, m + 3, 3]
    got, exp = _run_both(people, (xy, head, counts), index)
    _assert_same(got, exp)
    rs, rl, rc, flags = got
    assert flags == 0
    assert rc.tolist() == [1, m, 0, 3, COUNT_FILL, 0, m, COUNT_FILL]
    for row in (2, 4, 5, 7):                                              # dropped, unaddressed and empty rows keep the sentinel
        assert (rs[row] == SCORE_FILL).all() and (rl[row] == LABEL_FILL).all()
    assert rl[0, 0].sum() == 17 and (rs[0, 0] == np.float32(0.7)).all() and (rl[0, 1:] == LABEL_FILL).all()
    assert (rl[3, 0] == 0).all() and (rl[3, 1] == 0).all() and rl[3, 2].sum() == 17     # NaN and inf match nothing
    assert rl[1, :m].max() <= 1 and rl[6, :m].sum() > 0


def test_ties_and_empty_matches():
    rng = np.random.default_rng(12)
    m, gmax, n = 3, 2, 4
    xy, head, counts = np.zeros((n, gmax, 17, 2), np.float32), np.full((n, gmax), 20, np.float32), np.zeros(n, np.int32)
    humans, scores = [[] for _ in range(n)], [[] for _ in range(n)]

    def add_person(b, pts, **kw):
        hm, sm = person_at(pts, **kw)
        humans[b].append(hm); scores[b].append(sm)

    # image 0: two people identical in every joint -> the first claims the ground truth, the second gets zeros
    xy[0, 0], counts[0] = _gt_person(rng), 1
    add_person(0, xy[0, 0] + np.float32(2)); add_person(0, xy[0, 0] + np.float32(2))
    # image 1: one person equally close to two ground-truth people (8 joints each, different ones) -> the first g wins
    pts = _gt_person(rng)
    far = np.float32(500)
    xy[1, 0], xy[1, 1], counts[1] = pts + far, pts + far, 2
    xy[1, 0, :8], xy[1, 1, 8:16] = pts[:8], pts[8:16]
    add_person(1, pts)
    # image 2: a person whose best count is 0 -> nobody is claimed
    xy[2, 0], counts[2] = _gt_person(rng), 1
    add_person(2, xy[2, 0] + far, score=0.6)
    # image 3: only the root, and ground-truth joint 3 within the radius of (0, 0) -> label 1 with score 0
    xy[3, 0], counts[3] = _gt_person(rng), 1
    xy[3, 0, 3] = (6, -8)                                                  # distance 10 = 0.5 * head exactly
    add_person(3, np.zeros((17, 2)), joints=())
    got, exp = _run_both(pack_people(humans, scores, m), (xy, head, counts), np.arange(n))
    _assert_same(got, exp)
    rs, rl, rc, _ = got
    assert rc.tolist() == [2, 1, 1, 1]
    assert rl[0, 0].sum() == 17 and rl[0, 1].sum() == 0 and np.array_equal(rs[0, 0], rs[0, 1])
    assert rl[1, 0].tolist() == [1] * 8 + [0] * 9
    assert rl[2, 0].sum() == 0 and (rs[2, 0] == np.float32(0.6)).all()
    assert rl[3, 0].tolist() == [0, 0, 0, 1] + [0] * 13 and (rs[3, 0] == 0).all()


def test_threshold_sweep_is_bit_exact():
    """4 000 points within an ulp or two of the PCKh threshold (validate_cases.threshold_sweep), as 240 people x 17 joints:
    240 images of one person and one ground-truth person each, so that every person claims its ground truth and all its
    match bits reach the labels (where several people share one ground-truth person only the claiming one's bits do).
    Boxes of zero size keep the points' f32 values: (x + x) / 2 is exact."""
    gxy, ghead, pxy, counted = threshold_sweep()
    n = len(ghead)
    people = [person_at(pxy[i], half=0.0) for i in range(n)]
    packed = pack_people([[h] for h, _ in people], [[s] for _, s in people], 2)
    xy, head, counts = gxy.reshape(n, 1, 17, 2).copy(), ghead.reshape(n, 1).copy(), np.ones(n, np.int32)
    got, exp = _run_both(packed, (xy, head, counts), np.arange(n))
    miss = 1.0 - exp[1][:, 0][counted].mean()
    print(f"threshold sweep: {100 * miss:.2f} % of the 4000 points do not match")
    assert (exp[2] == 1).all() and 0.02 <= miss <= 0.20, miss
    assert int((got[1] != exp[1]).sum()) == 0
    _assert_same(got, exp)


def test_permuted_calls_fill_the_same_records_and_runs_repeat():
    _, validate = _mods()
    obj = synth.eval_case(5, 30)
    people, (xy, head, counts) = pack_people(obj[2], obj[3], M), _tables(obj)
    gt = validate.GroundTruth.from_arrays(xy, head, counts)
    natural, again, split = (_fresh_records(validate, 30, M) for _ in range(3))
    idx = torch.arange(30, dtype=torch.int32, device="cuda")
    validate.match_people(_result(people), gt, idx, natural)
    validate.match_people(_result(people), gt, idx, again)
    perm = np.random.default_rng(5).permutation(30)
    for part in (perm[:13], perm[13:]):                                     # two ragged calls, rows in any order
        validate.match_people(_result(tuple(a[part] for a in people)), gt, torch.from_numpy(part.astype(np.int32)).cuda(), split)
    a, b, c = natural.to_host(), again.to_host(), split.to_host()
    for other in (b, c):
        assert a[0].tobytes() == other[0].tobytes() and a[1].tobytes() == other[1].tobytes()
        assert a[2].tobytes() == other[2].tobytes() and a[3] == other[3] == 0


def test_flag_word_and_limits():
    decode, validate = _mods()
    from pytorch_pose_proposal_network_amd import lib as L
    obj = synth.eval_case(3, 8)
    people, (xy, head, counts) = pack_people(obj[2], obj[3], M), _tables(obj)
    got, exp = _run_both(people, (xy, head, counts), [0, 1, 2, 8, 4, -2, 6, 7])
    _assert_same(got, exp)
    assert got[3] == L.PPN_MATCH_FLAG_INDEX and got[2][3] == COUNT_FILL and got[2][5] == COUNT_FILL
    # a count beyond the table (a corrupted upload: from_arrays refuses to build one)
    gt = validate.GroundTruth.from_arrays(xy, head, counts)
    gt.gt_count[2] = gt.gmax + 1
    rec = _fresh_records(validate, 8, M)
    validate.match_people(_result(people), gt, torch.arange(8, dtype=torch.int32, device="cuda"), rec)
    assert rec.to_host()[3] == L.PPN_MATCH_FLAG_GT_COUNT and int(rec.count[2].cpu()) == COUNT_FILL
    # host-side limits: PPN_E_UNSUPPORTED before anything is launched
    lib = L.load()
    p = rec.score.data_ptr()
    assert lib.ppn_pckh_match(p, p, p, p, 1, 4, p, p, p, 1, L.PPN_MATCH_MAX_GT + 1, p, 0.5, p, p, p, p, None) == -3
    assert lib.ppn_pckh_match(p, p, p, p, 1, L.PPN_MATCH_MAX_PEOPLE + 1, p, p, p, 1, 4, p, 0.5, p, p, p, p, None) == -3
    assert lib.ppn_pckh_match(p, p, p, p, 1, 4, p, p, p, 1, 4, None, 0.5, p, p, p, p, None) == -1
    with pytest.raises(ValueError):
        validate.match_people(_result(people), gt, torch.arange(8, dtype=torch.int64, device="cuda"), rec)


def test_match_people_under_graph_capture():
    """The plan path of model.PoseProposalNet replays a graph of its own, so the matcher is captured alone: one replay
    fills the records as the direct call does."""
    _, validate = _mods()
    obj = synth.eval_case(1, 12)
    people, tables = pack_people(obj[2], obj[3], M), _tables(obj)
    gt = validate.GroundTruth.from_arrays(*tables)
    res = _result(people)
    idx = torch.arange(12, dtype=torch.int32, device="cuda")
    direct, replayed = _fresh_records(validate, 12, M), _fresh_records(validate, 12, M)
    validate.match_people(res, gt, idx, direct)                             # also loads the kernel before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        validate.match_people(res, gt, idx, replayed)
    replayed.score.fill_(SCORE_FILL); replayed.label.fill_(LABEL_FILL); replayed.count.fill_(COUNT_FILL)
    graph.replay()
    torch.cuda.synchronize()
    a, b = direct.to_host(), replayed.to_host()
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] == 0
    assert (b[2] != COUNT_FILL).all()


# ---- Validator end to end -----------------------------------------------------------------------------------------------
def _planted_gt(decoded, shift=(1.5, -1.0), spread=0.0):
    """Ground truth of one image from a compact decode: every second person's box centres, slightly shifted
    (tests/test_decode_gpu.py::test_device_decode_feeds_ap_evaluation).  spread > 0 moves joint j a further
    spread * j head sizes along x, so that the later joints of a person fall outside the PCKh radius of 0.5."""
    kps, boxes = [], []
    for p in range(0, int(decoded["n"]), 2):
        bb = decoded["bbox"][p]
        cy, cx = (bb[0, 0] + bb[0, 2]) / 2, (bb[0, 1] + bb[0, 3]) / 2
        box = (np.float32(cx), np.float32(cy), np.float32(bb[0, 3] - bb[0, 1]), np.float32(bb[0, 2] - bb[0, 0]))
        out = spread * np.arange(17) * float(evaluate._head_sizes([box])[0])
        kps.append(np.stack([(bb[1:, 1] + bb[1:, 3]) / 2 + shift[0] + out, (bb[1:, 0] + bb[1:, 2]) / 2 + shift[1]], 1).astype(np.float32))
        boxes.append(box)
    return (np.stack(kps) if kps else np.zeros((0, 17, 2), np.float32)), boxes


def _host_route(heads, gt_kps, gt_boxes, insize_hw, **kw):
    """The route of the parent commit: decode_heads -> to_humans() -> evaluate.evaluation."""
    decode, _ = _mods()
    obj = [[] for _ in range(7)]
    i = 0
    for head in heads:
        for hm, sc in decode.decode_heads(head, insize_hw=insize_hw, **kw).to_humans():
            obj[0].append(f"img_{i}.jpg"); obj[1].append(gt_kps[i]); obj[2].append(hm); obj[3].append(sc)
            obj[4].append(gt_boxes[i]); obj[5].append(None); obj[6].append(None)
            i += 1
    return evaluate.evaluation(obj), max(len(h) for h in obj[2])


@pytest.fixture(scope="module")
def d22_96():
    """D-22 at 96x96 with the weights of forward_d22_96.npz, two batches of 2 with targets (the set-up of
    tests/test_trainer_gpu.py::test_get_baseloss_matches_eval_oracle) and the forward_ref + loss_ref losses, computed once."""
    from pytorch_pose_proposal_network_amd import lib as L, prng
    from pytorch_pose_proposal_network_amd.trainer import PPNTrainer
    from oracle import decode_ref as D, forward_ref as Fr, loss_ref as Lr, targets_ref as Tg
    g = np.load(os.path.join(GOLDEN, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    sd = synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats)
    tr = PPNTrainer("drn_d_22", sd, compute_dtype=L.PPN_F32, insize=(96, 96))
    w = np.array([1.2, 0.8, 1.0, 0.9, 1.1], np.float32)
    tr.task.w.copy_(torch.from_numpy(w))
    batches, ref, gt_kps, gt_boxes = [], np.zeros(5), [], []
    for i in range(2):
        x = Fr.normalize_u8(prng.u8_frames(40 + i, 2, (96, 96)))
        tg = Tg.synthetic_batch(60 + 2 * i, 2, insize=(96, 96), outsize=(6, 6))
        head = Fr.forward_ref(sd, x, "drn_d_22")
        ref += np.array([float(v) for v in Lr.ppn_loss_ref(head, {k: torch.from_numpy(v) for k, v in tg.items()},
                                                          insize=(96, 96))])
        for b in range(2):
            kps, boxes = _planted_gt(D.decode_ref(head[b].numpy(), insize=(96, 96)), shift=(0.0, 0.0), spread=0.09)
            gt_kps.append(kps); gt_boxes.append(boxes)
        batches.append((torch.as_tensor(x).cuda(), {k: torch.from_numpy(v).cuda() for k, v in tg.items()}))
    return dict(trainer=tr, w=w, batches=batches, loss_ref=float((w.astype(np.float64) * (ref / 2)).sum() / 5),
                gt_kps=gt_kps, gt_boxes=gt_boxes)


def test_validator_end_to_end_d22_96(d22_96):
    _, validate = _mods()
    s = d22_96
    tr = s["trainer"]
    assert sum(len(b) for b in s["gt_boxes"]) > 0
    gt = validate.GroundTruth(s["gt_kps"], s["gt_boxes"])
    net = tr._eval_net()
    heads = [net(x).clone() for x, _ in s["batches"]]
    ap_host, most = _host_route(heads, s["gt_kps"], s["gt_boxes"], (96, 96))
    print("AP by the host route:", np.round(ap_host, 3).tolist(), "most people in an image:", most)

    v = validate.Validator(net, gt, 2, tr.criterion, tr.task.w, max_humans=36)
    v.reset()
    for i, (x, tg) in enumerate(s["batches"]):
        v.step(x, [2 * i, 2 * i + 1], tg)
    loss_avg, ap = v.finish()
    assert _same_ap(ap, ap_host), (ap, ap_host)
    assert np.isfinite(ap[-1]) and 0.0 < ap[-1] < 100.0                   # joints 6.. of the planted people are out of reach
    print("loss_avg", loss_avg, "forward_ref + loss_ref", s["loss_ref"])
    assert np.allclose(loss_avg, s["loss_ref"], rtol=2e-4), (loss_avg, s["loss_ref"])

    # a third batch of padding images changes neither; nor does feeding the last batch as two ragged ones
    v.step(s["batches"][0][0], [-1, -1])
    loss2, ap2 = v.finish()
    assert loss2 == loss_avg and _same_ap(ap2, ap)
    v.reset()
    x0, t0 = s["batches"][0]
    x1, t1 = s["batches"][1]
    v.step(x0, torch.tensor([0, 1], dtype=torch.int32), t0)
    for b in range(2):
        v.step(x1[b:b + 1], [2 + b], {k: t[b:b + 1] for k, t in t1.items()})
    loss3, ap3 = v.finish()
    assert _same_ap(ap3, ap) and np.allclose(loss3, s["loss_ref"], rtol=2e-4), (loss3, s["loss_ref"])

    # the trainer's convenience: the same epoch from (x, image_index, targets) triples
    loss4, ap4 = tr.validate([(x, [2 * i, 2 * i + 1], tg) for i, (x, tg) in enumerate(s["batches"])], gt, max_humans=36)
    assert _same_ap(ap4, ap) and np.allclose(loss4, loss_avg, rtol=1e-6)


class _CrowdNet:
    """Stands in for the network: hands back planted-crowd heads (24x24 cells), whatever the frames."""
    training = False
    insize, outsize, local_grid_size = (384, 384), (24, 24), (21, 21)

    def __init__(self, heads):
        self.heads, self.calls = heads, 0

    def __call__(self, x):
        self.calls += 1
        return self.heads[self.calls - 1]


def test_validator_on_planted_crowds_and_overflow():
    from oracle import decode_ref as D
    _, validate = _mods()
    heads_np = [np.stack([synth.planted_crowd_head(40 + 2 * i + b) for b in range(2)]) for i in range(2)]
    gt_kps, gt_boxes = zip(*[_planted_gt(D.decode_ref(h)) for hb in heads_np for h in hb])
    heads = [torch.from_numpy(h).cuda() for h in heads_np]
    ap_host, most = _host_route(heads, gt_kps, gt_boxes, (384, 384))
    assert most > 1
    gt = validate.GroundTruth(gt_kps, gt_boxes)
    x = torch.zeros(2, 3, 384, 384, device="cuda")

    def epoch(max_humans):
        v = validate.Validator(_CrowdNet(heads), gt, 2, max_humans=max_humans)
        v.reset()
        for i in range(2):
            v.step(x, [2 * i, 2 * i + 1])
        return v.finish()

    loss_avg, ap = epoch(most)                                              # exactly as many slots as the fullest image needs
    assert loss_avg is None
    print("AP on the planted crowds:", np.round(ap, 3).tolist(), "most people in an image:", most)
    assert _same_ap(ap, ap_host), (ap, ap_host)
    assert 0.0 < ap[-1] <= 100.0
    with pytest.raises(RuntimeError, match="max_humans"):
        epoch(1)
    with pytest.raises(RuntimeError, match="max_humans"):
        epoch(most - 1)
    # an index beyond the tables raises at the end of the epoch
    v = validate.Validator(_CrowdNet(heads), gt, 2, max_humans=most)
    v.reset()
    v.step(x, [0, 4])
    with pytest.raises(RuntimeError, match="index"):
        v.finish()
