"""CPU: the NumPy restatement of ppn_pckh_match (tests/validate_ref.py) and evaluate.metrics_from_records against
evaluate.assign_gt_multi / evaluation and the AP values the imported reference produced (tests/golden/eval_cases.npz), and
the packing of validate.GroundTruth."""
import os

import numpy as np
import pytest
import torch

import validate_ref as R
from validate_cases import pack_people
from pytorch_pose_proposal_network_amd import evaluate, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M = 7                                        # the golden seeds hold at most 6 people per image


def _golden():
    g = np.load(os.path.join(GOLDEN, "eval_cases.npz"), allow_pickle=False)
    return [(int(s), int(n), np.asarray(ap, np.float64)) for s, n, ap in zip(g["seeds"], g["sizes"], g["ap"])]


def _pack_gt(obj):
    """NumPy tables in GroundTruth's layout, built independently of it."""
    counts = np.array([len(b) for b in obj[4]], np.int32)
    gmax = max(1, int(counts.max()))
    xy = np.zeros((len(counts), gmax, 17, 2), np.float32)
    head = np.zeros((len(counts), gmax), np.float32)
    for i, (kps, boxes) in enumerate(zip(obj[1], obj[4])):
        if len(boxes):
            xy[i, :len(boxes)] = np.asarray(kps, np.float32).reshape(-1, 17, 2)
            head[i, :len(boxes)] = evaluate._head_sizes(boxes)
    return xy, head, counts


def _records(obj, m=M):
    count, kp_cell, bbox, score = pack_people(obj[2], obj[3], m)
    xy, head, counts = _pack_gt(obj)
    n = len(counts)
    rs, rl, rc = np.full((n, m, 17), -7, np.float32), np.full((n, m, 17), 9, np.uint8), np.full(n, -3, np.int32)
    flags = R.pckh_match(count, kp_cell, bbox, score, xy, head, counts, np.arange(n, dtype=np.int32), rs, rl, rc)
    assert flags == 0
    return rs, rl, rc, counts


@pytest.mark.parametrize("seed,n,ap", _golden())
def test_ref_equals_assign_gt_multi_and_golden_ap(seed, n, ap):
    obj = synth.eval_case(seed, n)
    assert max(len(h) for h in obj[2]) <= M
    rs, rl, rc, counts = _records(obj)
    # the frames `evaluation` keeps, through the array matcher that is pinned to the reference
    kept = [i for i in range(n) if len(obj[4][i])]
    frames = []
    for i in kept:
        pxy, psc = evaluate._pred_arrays(obj[2][i], obj[3][i])
        frames.append((pxy, psc, np.asarray(obj[1][i], np.float32).reshape(-1, 17, 2), evaluate._head_sizes(obj[4][i])))
    scores_all, labels_all, n_gt = evaluate.assign_gt_multi(frames)
    for f, i in enumerate(kept):
        P = len(obj[2][i])
        assert rc[i] == P
        for j in range(17):
            assert np.array_equal(rs[i, :P, j], np.asarray(scores_all[j][f], np.float32)), (i, j)
            assert np.array_equal(rl[i, :P, j], np.asarray(labels_all[j][f]).astype(np.uint8)), (i, j)
        assert (rs[i, P:] == -7).all() and (rl[i, P:] == 9).all()          # rows beyond the count are not written
        assert n_gt[0, f] == counts[i]
    for i in set(range(n)) - set(kept):
        assert rc[i] == 0 and (rs[i] == -7).all()
    got = evaluate.metrics_from_records(rs, rl, rc, counts)
    assert np.allclose(got, ap, rtol=0, atol=1e-9), (seed, got, ap)
    assert np.array_equal(np.asarray(got), np.asarray(evaluate.evaluation(obj)), equal_nan=True)


def test_golden_holds_a_case_without_ground_truth():
    """One golden case has no frame with ground truth: every image is dropped and the metric is that of an empty set."""
    empty = [(s, n) for s, n, _ in _golden() if all(len(b) == 0 for b in synth.eval_case(s, n)[4])]
    assert empty
    for s, n in empty:
        rs, rl, rc, counts = _records(synth.eval_case(s, n))
        assert (rc == 0).all() and (counts == 0).all()


def test_metrics_from_records_rejects_bad_shapes():
    rs, rl = np.zeros((2, 3, 17), np.float32), np.zeros((2, 3, 17), np.uint8)
    with pytest.raises(ValueError):
        evaluate.metrics_from_records(rs, rl[:, :2], np.zeros(2, np.int32), np.ones(2, np.int32))
    with pytest.raises(ValueError):
        evaluate.metrics_from_records(rs, rl, np.array([0, 4], np.int32), np.ones(2, np.int32))
    with pytest.raises(ValueError):
        evaluate.metrics_from_records(rs, rl, np.zeros(3, np.int32), np.ones(3, np.int32))


def test_ground_truth_packing():
    from pytorch_pose_proposal_network_amd import validate
    obj = synth.eval_case(3, 8)
    assert any(len(b) == 0 for b in obj[4]) and any(len(b) > 1 for b in obj[4])
    gt = validate.GroundTruth(obj[1], obj[4], device="cpu")
    xy, head, counts = _pack_gt(obj)
    assert gt.n_images == 8 and gt.gmax == xy.shape[1]
    assert gt.gt_count.dtype == torch.int32 and np.array_equal(gt.gt_count.numpy(), counts)
    assert np.array_equal(gt.gt_xy.numpy(), xy) and np.array_equal(gt.gt_head.numpy(), head)
    for i, boxes in enumerate(obj[4]):
        assert gt.gt_count[i] == len(boxes)
        assert np.array_equal(gt.gt_head.numpy()[i, :len(boxes)], evaluate._head_sizes(boxes))
        assert (gt.gt_head.numpy()[i, len(boxes):] == 0).all()
    # the flat [G, 34] layout main.py reshapes from is taken too; a wider table on request
    flat = [np.asarray(k, np.float32).reshape(len(b), 34) for k, b in zip(obj[1], obj[4])]
    wide = validate.GroundTruth(flat, obj[4], device="cpu", gmax=5)
    assert wide.gmax == 5 and np.array_equal(wide.gt_xy.numpy()[:, :gt.gmax], xy) and (wide.gt_xy.numpy()[:, gt.gmax:] == 0).all()
    # limits
    crowd_boxes = [[(np.float32(50), np.float32(50), np.float32(20), np.float32(30))] * (validate.MAX_GT + 1)]
    crowd_kps = [np.zeros((validate.MAX_GT + 1, 17, 2), np.float32)]
    with pytest.raises(ValueError, match="at most 64"):
        validate.GroundTruth(crowd_kps, crowd_boxes, device="cpu")
    at_limit = validate.GroundTruth([crowd_kps[0][:-1]], [crowd_boxes[0][:-1]], device="cpu")
    assert at_limit.gmax == validate.MAX_GT
    with pytest.raises(ValueError):
        validate.GroundTruth(obj[1], obj[4], device="cpu", gmax=1)         # below the set's largest image
    with pytest.raises(ValueError):
        validate.GroundTruth(obj[1][:3], obj[4], device="cpu")
    with pytest.raises(ValueError):
        validate.GroundTruth([np.zeros((1, 16, 2), np.float32)], [crowd_boxes[0][:1]], device="cpu")
    same = validate.GroundTruth.from_arrays(xy, head, counts, device="cpu")
    assert same.gmax == gt.gmax and np.array_equal(same.gt_head.numpy(), head) and np.array_equal(same.counts, counts)
    with pytest.raises(ValueError):
        validate.GroundTruth.from_arrays(xy, head, counts + xy.shape[1], device="cpu")
    with pytest.raises(ValueError):
        validate.GroundTruth.from_arrays(np.zeros((1, 65, 17, 2), np.float32), np.zeros((1, 65)), np.zeros(1), device="cpu")


def test_ref_flags_and_padding():
    """Indices outside [-1, N) and counts beyond the table set the flag word and write nothing; -1 writes nothing."""
    obj = synth.eval_case(3, 8)
    count, kp_cell, bbox, score = pack_people(obj[2], obj[3], M)
    xy, head, counts = _pack_gt(obj)
    n = len(counts)

    def run(index, cnts=counts):
        rs, rl, rc = np.full((n, M, 17), -7, np.float32), np.full((n, M, 17), 9, np.uint8), np.full(n, -3, np.int32)
        return R.pckh_match(count, kp_cell, bbox, score, xy, head, cnts, np.asarray(index, np.int32), rs, rl, rc), rs, rl, rc

    f, rs, rl, rc = run([-1] * n)
    assert f == 0 and (rc == -3).all() and (rs == -7).all() and (rl == 9).all()
    f, rs, rl, rc = run([0, 1, 2, 3, 4, 5, 6, n])
    assert f == 1 and rc[7] == -3
    f, rs, rl, rc = run([0, 1, 2, 3, 4, 5, 6, -2])
    assert f == 1
    big = counts.copy()
    big[2] = xy.shape[1] + 1
    f, rs, rl, rc = run(np.arange(n), big)
    assert f == 2 and rc[2] == -3 and rc[3] != -3
