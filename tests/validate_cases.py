"""Shared by test_validate_cpu.py and test_validate_gpu.py: people dicts packed into DecodeResult-shaped arrays (the inverse
of DecodeResult.to_humans()), hand-made people, and the threshold sweep of the PCKh knife edge."""
import numpy as np

K, J = 18, 17


def pack_people(humans_list, scores_list, M):
    """Per-image lists of {kp: f32[4]} / {kp: f32} dicts -> count i32[B], kp_cell i32[B,M,18], bbox f32[B,M,18,4],
    score f32[B,M,18].  `count` keeps the full number of people; slots beyond M are dropped as the decoder drops them."""
    B = len(humans_list)
    count = np.zeros(B, np.int32)
    kp_cell = np.full((B, M, K), -1, np.int32)
    bbox = np.zeros((B, M, K, 4), np.float32)
    score = np.zeros((B, M, K), np.float32)
    for b, (humans, scores) in enumerate(zip(humans_list, scores_list)):
        count[b] = len(humans)
        for p, (hm, sm) in enumerate(zip(humans[:M], scores[:M])):
            for k, box in hm.items():
                kp_cell[b, p, k] = 7 + k                            # any cell index: only its sign is read
                bbox[b, p, k] = np.asarray(box, np.float32)
                score[b, p, k] = np.float32(sm[k])
    return count, kp_cell, bbox, score


def person_at(xy, half=4.0, score=0.5, joints=range(J)):
    """(human dict, score dict) with the root and the chosen joints as boxes of half-width `half` centred on xy f32[17,2]."""
    xy = np.asarray(xy, np.float32)
    hm, sm = {0: np.array([0, 0, 10, 10], np.float32)}, {0: np.float32(0.9)}
    for j in joints:
        x, y = xy[j]
        hm[j + 1] = np.array([y - half, x - half, y + half, x + half], np.float32)
        sm[j + 1] = np.float32(score)
    return hm, sm


def threshold_sweep(n_people=240, seed=7):
    """The PCKh knife edge: 4 000 points at 0.5 * head from their ground-truth joint, which sits at the origin --
    default_rng(7), head uniform in [8, 60), a random angle, everything rounded to f32 -- ordered as n_people x 17 joints,
    each person against the one ground-truth person of its image.  A ground-truth person has ONE head size: of the 4 000
    drawn it takes the one drawn for its first joint, and all its 17 points lie on that head's circle.  240 x 17 = 4 080: the
    last 80 joints are filler that sits on its ground truth (they always match and are left out of the counted 4 000).
    All counted points are within an ulp or two of the threshold: contracting dx*dx + dy*dy into an FMA or multiplying by
    1 / head flips dozens of them.
    Returns (gt_xy f32[n_people,17,2], head f32[n_people], pred_xy f32[n_people,17,2], counted bool[n_people,17])."""
    rng = np.random.default_rng(seed)
    n, total = 4000, n_people * J
    assert total >= n
    head = rng.uniform(8, 60, n).astype(np.float32)
    ang = rng.uniform(0, 2 * np.pi, n)
    head = np.concatenate([head, np.full(total - n, 20, np.float32)]).reshape(n_people, J)[:, 0].copy()
    ang = np.concatenate([ang, np.zeros(total - n)])
    counted = np.arange(total) < n
    r = 0.5 * np.repeat(head, J).astype(np.float64) * counted
    pred = np.stack([r * np.cos(ang), r * np.sin(ang)], 1).astype(np.float32)
    return np.zeros((n_people, J, 2), np.float32), head, pred.reshape(n_people, J, 2), counted.reshape(n_people, J)
