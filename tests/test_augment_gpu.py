"""Train-time augmentation on the device (csrc/augment.hip, pytorch_pose_proposal_network_amd/augment.py) against the NumPy
restatement tests/augment_ref.py, BIT FOR BIT: the arithmetic is fully specified (include/ppn.h), both sides get the same
f32 fwd / inv matrices, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import augment_ref as R

pytestmark = pytest.mark.gpu

K = 18
ROW = 5 + 2 * (K - 1)
HW = np.array([[40, 56], [33, 47], [17, 23]], np.int32)          # valid sizes inside the 40 x 56 padding
OUT = (32, 48)


def _mods():
    from pytorch_pose_proposal_network_amd import augment, targets
    return augment, targets


def _f32(m):
    return np.ascontiguousarray(m[:, :2, :], np.float32)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope="module")
def pictures():
    """u8 [3,40,56,3]; everything outside a picture's valid size is 255, so a read out there shows up."""
    rng = np.random.default_rng(2024)
    src = np.full((3, 40, 56, 3), 255, np.uint8)
    for b, (h, w) in enumerate(HW):
        src[b, :h, :w] = rng.integers(0, 255, (h, w, 3), dtype=np.uint8)
    return src


def _inv_case(name, out_hw=OUT):
    A, _ = _mods()
    if name.startswith("train"):
        return A.sample_params(17, int(name[5:]), HW, out_hw, "train")["inv"]
    if name == "identity":
        return np.tile(np.array([[1, 0, 0], [0, 1, 0]], np.float32), (3, 1, 1))
    if name == "rot180":
        return _f32(A.affine_matrices(180.0, 1.0, (0, 0, 0, 0), HW, out_hw)[1])
    if name == "rot180_same_size":                                   # source size = output size: taps on integers
        return _f32(np.stack([A.affine_matrices(180.0, 1.0, (0, 0, 0, 0), hw, hw)[1][0] for hw in HW]))
    if name == "s035":
        return _f32(A.affine_matrices(25.0, 0.35, (0, 0, 0, 0), HW, out_hw)[1])
    if name == "s250":
        return _f32(A.affine_matrices(-31.0, 2.5, (1, 2, 3, 4), HW, out_hw)[1])
    if name == "straddle":      # sx in [-0.75, 22.75], sy in [-0.75, 17.85]: taps on both sides of every edge of 17 x 23
        return np.tile(np.array([[0.5, 0, -0.75], [0, 0.6, -0.75]], np.float32), (3, 1, 1))
    raise KeyError(name)


IMAGE_CASES = ["train0", "train1", "train2", "train3", "train4", "identity", "rot180", "rot180_same_size", "s035", "s250",
               "straddle"]


@pytest.mark.parametrize("name", IMAGE_CASES)
def test_images_bit_exact(pictures, name):
    A, _ = _mods()
    inv = _inv_case(name)
    ref_u8, ref_x = R.augment_images_ref(pictures, HW, inv, OUT)
    if name == "straddle":
        assert (ref_u8[2, :, 0] < 255).all() and not ref_u8[2, -1].any()      # the case does reach the edges
    if name == "s035":
        assert (ref_u8 == 0).mean() > 0.5                                       # most of the output is border
    u8, x = A.augment_images(torch.from_numpy(pictures).cuda(), HW, inv, OUT, want_u8=True)
    assert _same(u8, ref_u8), np.argwhere(u8.cpu().numpy() != ref_u8)[:5]
    assert _same(x, ref_x)
    # either output alone, into buffers the caller owns (sentinels: every element is written)
    only_u8 = torch.full((3, *OUT, 3), 7, dtype=torch.uint8, device="cuda")
    got = A.augment_images(torch.from_numpy(pictures).cuda(), torch.from_numpy(HW).cuda(), torch.from_numpy(inv).cuda(),
                           OUT, out_u8=only_u8, want_f32=False)
    assert got[0] is only_u8 and got[1] is None and _same(only_u8, ref_u8)
    only_x = torch.full((3, 3, *OUT), float("nan"), device="cuda")
    got = A.augment_images(pictures, HW, inv, OUT, out_f32=only_x)
    assert got[0] is None and got[1] is only_x and _same(only_x, ref_x)


@pytest.mark.parametrize("name", ["train1", "straddle", "s250"])
def test_images_bit_exact_scalar_store_path(pictures, name):
    """outW % 4 != 0: the one-pixel-per-thread instantiation."""
    A, _ = _mods()
    out_hw = (31, 45)
    inv = _inv_case(name, out_hw)
    ref_u8, ref_x = R.augment_images_ref(pictures, HW, inv, out_hw)
    u8, x = A.augment_images(pictures, HW, inv, out_hw, want_u8=True)
    assert _same(u8, ref_u8) and _same(x, ref_x)


def test_image_full_size_from_200x300():
    A, _ = _mods()
    hw = np.array([[200, 300]], np.int32)
    src = np.random.default_rng(5).integers(0, 256, (1, 200, 300, 3), dtype=np.uint8)
    p = A.sample_params(23, 1, hw, (384, 384), "train")
    ref_u8, ref_x = R.augment_images_ref(src, hw, p["inv"], (384, 384))
    assert ref_u8.any()
    u8, x = A.augment_images(src, hw, p["inv"], (384, 384), want_u8=True)
    assert _same(u8, ref_u8) and _same(x, ref_x)


def test_images_reject_bad_arguments(pictures):
    A, _ = _mods()
    from pytorch_pose_proposal_network_amd.lib import PPNError
    inv = _inv_case("identity")
    with pytest.raises(ValueError):
        A.augment_images(pictures, np.array([[41, 56], [33, 47], [17, 23]]), inv, OUT)      # taller than the padding
    with pytest.raises(PPNError):
        A.augment_images(pictures, HW, inv, OUT, want_f32=False)                             # no output asked for


# -------------------------------------------------------------------------------------------------------------- labels

def _random_people(rng, n, w, h, far=()):
    """n rows of packed people inside a w x h picture; rows listed in `far` have every keypoint far outside any frame."""
    P = np.zeros((n, ROW), np.float32)
    V = np.zeros(n, np.int32)
    for i in range(n):
        P[i, 0:2] = rng.uniform(0, [w, h])
        P[i, 2:4] = rng.integers(0, 30, 2)
        P[i, 4] = 8 + i
        pts = rng.uniform(0, [w - 1, h - 1], (K - 1, 2)).astype(np.float32)
        pts[rng.random(K - 1) < 0.2] = 0                              # absent keypoints
        if i in far:
            pts = pts + np.float32(5000)
        P[i, 5:] = pts.reshape(-1)
        V[i] = int(rng.integers(0, 1 << (K - 1)))                     # hidden-but-present and labeled-but-absent mixes
    return P, V


def _label_batch(pmax, seed):
    """Five images: count 0 (rows hold stale data that must be zeroed), 1, pmax with people dropped first / last / in the
    middle, pmax with nobody dropped, pmax with everybody dropped."""
    rng = np.random.default_rng(seed)
    people, visible = np.zeros((5, pmax, ROW), np.float32), np.zeros((5, pmax), np.int32)
    count = np.array([0, 1, pmax, pmax, pmax], np.int32)
    mid = set(range(2, pmax - 1, 3))
    for b, far in enumerate(((), (), {0, pmax - 1} | mid, (), set(range(pmax)))):
        people[b], visible[b] = _random_people(rng, pmax, 56, 40, far)
    return people, visible, count


@pytest.mark.parametrize("pmax", [3, 70, 300])
def test_people_bit_exact(pmax):
    """pmax 3 and 70 (more people than a wavefront has lanes) and 300 (more than the kernel's 256-person chunk)."""
    A, _ = _mods()
    people, visible, count = _label_batch(pmax, 100 + pmax)
    hw = np.tile(np.array([[40, 56]], np.int32), (5, 1))
    for name, fwd in (("train", A.sample_params(29, 2, hw, OUT, "train")["fwd"]),
                      ("val", A.sample_params(0, 0, hw, OUT, "val")["fwd"]),
                      ("half", _f32(A.affine_matrices(33.0, 0.5, (2, 0, 1, 3), hw, OUT)[0]))):
        rp, rv, rc = R.augment_people_ref(people, visible, count, fwd, OUT)
        assert rc[0] == 0 and rc[1] <= 1 and rc[4] == 0
        if name == "val":                                             # the resize keeps everyone who was not moved away
            assert rc.tolist() == [0, 1, pmax - len({0, pmax - 1} | set(range(2, pmax - 1, 3))), pmax, 0]
        po, vo, co = A.augment_people((people, visible, count), fwd, OUT)
        assert _same(co, rc), (co, rc)
        assert _same(vo, rv)
        assert _same(po, rp)                                          # the zeroed tail included
        # device tensors in, caller-owned (dirty) outputs
        out = (torch.full((5, pmax, ROW), 3.0, device="cuda"), torch.full((5, pmax), -1, dtype=torch.int32, device="cuda"),
               torch.full((5,), -1, dtype=torch.int32, device="cuda"))
        got = A.augment_people(tuple(torch.from_numpy(a).cuda() for a in (people, visible, count)),
                               torch.from_numpy(fwd).cuda(), OUT, out=out)
        assert got[0] is out[0] and _same(out[0], rp) and _same(out[1], rv) and _same(out[2], rc)


def test_people_edges_of_the_frame_and_of_the_boxes():
    """Identity F on a 32 x 48 frame, so the inputs ARE the knife edges: a keypoint exactly on x' = 0, one just below outW,
    one exactly on outW; boxes partly outside, wholly outside and of zero width."""
    A, _ = _mods()
    below = np.nextafter(np.float32(48), np.float32(0))
    below_h = np.nextafter(np.float32(32), np.float32(0))
    rows = [
        dict(box=(10, 10, 8, 6), pts=[(0.0, 5.0), (below, 7.0), (48.0, 7.0), (5.0, below_h), (5.0, 32.0), (-0.5, 3.0)]),
        dict(box=(46, 30, 9, 9), pts=[(1.0, 1.0)]),                   # partly outside (right / bottom)
        dict(box=(-20, -20, 10, 10), pts=[(2.0, 2.0)]),               # wholly outside: clips to an empty box at (0, 0)
        dict(box=(100, 10, 10, 4), pts=[(3.0, 3.0)]),                 # wholly outside on the right: empty box at x = 48
        dict(box=(20, 20, 1, 7), pts=[(4.0, 4.0)]),                   # floor(1 / 2) = 0: zero width
        dict(box=(20, 20, 0, 0), pts=[(5.0, 0.0)]),                   # no box at all; keypoint on y' = 0
        dict(box=(20, 20, 4, 4), pts=[(48.0, 1.0), (1.0, 32.0)]),     # every keypoint on the far edges: dropped
    ]
    pmax = len(rows)
    people, visible = np.zeros((1, pmax, ROW), np.float32), np.full((1, pmax), (1 << (K - 1)) - 1, np.int32)
    for i, r in enumerate(rows):
        people[0, i, 0:4] = r["box"]
        people[0, i, 4] = i + 1
        people[0, i, 5:5 + 2 * len(r["pts"])] = np.asarray(r["pts"], np.float32).reshape(-1)
    count = np.array([pmax], np.int32)
    fwd = np.array([[[1, 0, 0], [0, 1, 0]]], np.float32)
    rp, rv, rc = R.augment_people_ref(people, visible, count, fwd, OUT)
    # the restatement does what the contract says on these rows
    assert rc[0] == pmax - 1 and rp[0, :, 4].tolist() == [1, 2, 3, 4, 5, 6, 0]
    assert rp[0, 0, 5:17].tolist() == [0, 5, below, 7, 0, 0, 5, below_h, 0, 0, 0, 0] and rv[0, 0] == 0b001011
    assert rp[0, 1, :4].tolist() == [(42 + 48) / 2, (26 + 32) / 2, 6, 6]
    assert rp[0, 2, :4].tolist() == [0, 0, 0, 0] and rp[0, 3, :4].tolist() == [48, 10, 0, 4]
    assert rp[0, 4, :4].tolist() == [20, 20, 0, 6] and rp[0, 5, :4].tolist() == [20, 20, 0, 0]
    po, vo, co = A.augment_people((people, visible, count), fwd, OUT)
    assert _same(co, rc) and _same(vo, rv) and _same(po, rp)


# ------------------------------------------------------------------------------------------------------------- handoff

def _handoff_inputs():
    from pytorch_pose_proposal_network_amd import synth
    _, T = _mods()
    hw = np.array([[80, 100], [64, 70]], np.int32)
    src = np.full((2, 80, 100, 3), 255, np.uint8)
    rng = np.random.default_rng(77)
    for b, (h, w) in enumerate(hw):
        src[b, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    lists = [synth.synthetic_people(300 + b, insize=(int(w), int(h))) for b, (h, w) in enumerate(hw)]
    return src, hw, T.pack_people(lists, pmax=6)


def test_train_augmenter_equals_reference_pipeline():
    A, T = _mods()
    src, hw, packed = _handoff_inputs()
    aug = A.TrainAugmenter(insize=(96, 96), seed=3, mode="train")
    x, tg = aug(torch.from_numpy(src).cuda(), hw, packed, step=5)
    p = aug.params
    assert _same(p["fwd"], A.sample_params(3, 5, hw, (96, 96), "train")["fwd"])
    _, ref_x = R.augment_images_ref(src, hw, p["inv"], (96, 96))
    rp, rv, rc = R.augment_people_ref(*packed, p["fwd"], (96, 96))
    assert rc.sum() > 0
    want = T.encode_targets(T.pack_people(R.unpack_people(rp, rv, rc)), (96, 96), (6, 6))
    assert _same(x, ref_x)
    assert sorted(tg) == sorted(want) and "limb_c" in tg
    for k in want:
        assert _same(tg[k], want[k]), k
    assert tg["delta"].sum() > 0
    # a second step reuses every buffer, device-tensor annotations give the same batch, and step 5 comes back identical
    first = {k: v.clone() for k, v in tg.items()}
    ptrs = (x.data_ptr(), {k: v.data_ptr() for k, v in tg.items()})
    x6, tg6 = aug(torch.from_numpy(src).cuda(), hw, packed, step=6)
    assert not _same(aug.params["fwd"], p["fwd"]) and (x6.data_ptr(), {k: v.data_ptr() for k, v in tg6.items()}) == ptrs
    x5, tg5 = aug(torch.from_numpy(src).cuda(), torch.from_numpy(hw).cuda(),
                  tuple(torch.from_numpy(a).cuda() for a in packed), step=5)
    assert _same(x5, ref_x) and all(_same(tg5[k], first[k]) for k in first)
    # val mode: the resize alone
    xv, _ = A.TrainAugmenter(insize=(96, 96), mode="val")(src, hw, packed, step=0)
    assert _same(xv, R.augment_images_ref(src, hw, A.sample_params(0, 0, hw, (96, 96), "val")["inv"], (96, 96))[1])


def test_trainer_takes_the_augmented_batch():
    """One PPNTrainer.train_step (DRN-D-22, first-order) on what TrainAugmenter returns, unchanged."""
    A, _ = _mods()
    from pytorch_pose_proposal_network_amd import lib as L, synth
    from pytorch_pose_proposal_network_amd.trainer import PPNTrainer
    src, hw, packed = _handoff_inputs()
    x, tg = A.TrainAugmenter(insize=(96, 96), seed=3)(src, hw, packed, step=5)
    tr = PPNTrainer("drn_d_22", synth.make_state_dict("drn_d_22", 0), compute_dtype=L.PPN_F32, insize=(96, 96),
                    second_order=False)
    losses, w = tr.train_step(x, tg)
    torch.cuda.synchronize()
    losses, w = losses.cpu().numpy(), w.cpu().numpy()
    assert losses.shape == (5,) and np.isfinite(losses).all() and (losses > 0).all() and np.isfinite(w).all()


def test_encode_targets_takes_device_tensors():
    _, T = _mods()
    _, _, packed = _handoff_inputs()
    a = T.encode_targets(packed, (96, 96), (6, 6))
    dev = tuple(torch.from_numpy(v).cuda() for v in packed)
    b = T.encode_targets(dev, (96, 96), (6, 6))
    assert sorted(a) == sorted(b)
    for k in a:
        assert _same(a[k], b[k]), k
    c = T.encode_targets(dev, (96, 96), (6, 6), out=b)               # written in place
    assert all(c[k] is b[k] for k in b) and all(_same(c[k], a[k]) for k in a)
    with pytest.raises(ValueError):
        T.encode_targets((dev[0].double(), dev[1], dev[2]), (96, 96), (6, 6))
