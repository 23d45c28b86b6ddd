"""The augmentation stage's options on the device (csrc/augment.hip: ppn_augment_images_color, ppn_augment_people_mirror;
augment.TrainAugmenter(mirror_p, color)) against the NumPy restatement tests/augment_jitter_ref.py, BIT FOR BIT: the
arithmetic is fully specified (include/ppn.h) and both sides get the same matrices and parameter rows, so there is no
tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest
import torch

import augment_jitter_ref as J
import augment_ref as R
import tta_ref

pytestmark = pytest.mark.gpu

K = 18
ROW = 5 + 2 * (K - 1)
KP = tta_ref.KP_MIRROR
HW = np.array([[37, 53], [40, 56], [21, 30]], np.int32)            # valid sizes inside the 40 x 56 padding
VEC, SCALAR = (32, 48), (32, 30)


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


def _key(n):
    from pytorch_pose_proposal_network_amd import prng
    return [int(x) for x in np.array([prng.stream_seed(77, n)], np.uint64).view(np.int32)]


@pytest.fixture(scope="module")
def pictures():
    """u8 [3,40,56,3]; everything outside a picture's valid size is 255, so a read out there shows up."""
    rng = np.random.default_rng(2025)
    src = np.full((3, 40, 56, 3), 255, np.uint8)
    for b, (h, w) in enumerate(HW):
        src[b, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return src


def _rows(name):
    """i32 [3,10]: the parameter rows of one batch, different per image."""
    rng = np.random.default_rng(len(name))
    if name == "identity_and_clamps":       # identity; gain 1024 with offset -255; gain 0 with offset 255
        return np.array([list(J.IDENTITY), [256, 1024, 1024, 1024, -255, -255, -255, 0, 0, 0],
                         [256, 0, 0, 0, 255, 255, 255, 0, 0, 0]], np.int32)
    if name == "saturation_and_noise":      # sat 0; sat 512; noise_q 4096 on an otherwise plain picture
        return np.array([[0, 256, 256, 256, 0, 0, 0, 0] + _key(0), [512, 256, 256, 256, 0, 0, 0, 300] + _key(1),
                         [256, 256, 256, 256, 0, 0, 0, 4096] + _key(2)], np.int32)
    if name == "random":                    # inside the ranges
        return np.stack([np.concatenate([[rng.integers(0, 513)], rng.integers(0, 1025, 3), rng.integers(-255, 256, 3),
                                         [rng.integers(0, 4097)], _key(10 + b)]) for b in range(3)]).astype(np.int32)
    if name == "beyond_the_ranges":         # the kernel clamps: sat 9999 / -3, gains 5000 / -7, offsets +-999, noise_q 99999 / -5
        return np.array([[9999, 5000, -7, 300, 999, -999, 10, 99999] + _key(20), [-3, 256, 256, 2000, -999, 0, 999, -5] + _key(21),
                         [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, 256, -2 ** 31, 2 ** 31 - 1, 0, 2 ** 31 - 1] + _key(22)], np.int32)
    if name == "sampled":                   # what the sampler folds a default ColorJitter into
        A, _ = _mods()
        return A.sample_params(5, 1, HW, VEC, "train", color=A.ColorJitter())["color"]
    raise KeyError(name)


def _inv(name, out_hw):
    """f32 [3,2,3]; every batch holds mirrored and unmirrored images."""
    A, _ = _mods()
    flags = {"identity_and_clamps": [1, 0, 1], "saturation_and_noise": [0, 1, 0], "random": [1, 1, 0],
             "beyond_the_ranges": [0, 0, 1], "sampled": [1, 0, 0]}[name]
    if name == "saturation_and_noise":      # taps on both sides of every edge of the smallest picture, mirrored or not
        return _f32(A.affine_matrices(0.0, 0.6, (0, 0, 0, 0), HW, out_hw, mirror=flags)[1])
    p = A.sample_params(17, len(name), HW, out_hw, "train")
    return _f32(A.affine_matrices(p["theta"], p["scale"], p["crop"], HW, out_hw, mirror=flags)[1])


ROW_SETS = ["identity_and_clamps", "saturation_and_noise", "random", "beyond_the_ranges", "sampled"]


@pytest.mark.parametrize("out_hw", [VEC, SCALAR], ids=["vec32x48", "scalar32x30"])
@pytest.mark.parametrize("name", ROW_SETS)
def test_colour_images_bit_exact(pictures, name, out_hw):
    A, _ = _mods()
    rows, inv = _rows(name), _inv(name, out_hw)
    ref_u8, ref_x = J.augment_images_color_ref(pictures, HW, inv, rows, out_hw)
    plain_u8, _ = R.augment_images_ref(pictures, HW, inv, out_hw)
    assert not np.array_equal(ref_u8[1:], plain_u8[1:])              # the rows do something
    src = torch.from_numpy(pictures).cuda()
    u8, x = A.augment_images(src, HW, inv, out_hw, want_u8=True, color=rows)
    assert _same(u8, ref_u8), np.argwhere(u8.cpu().numpy() != ref_u8)[:5]
    assert _same(x, ref_x)
    # a second run writes the same bytes (the noise is a function of the key and the pixel index alone)
    u8b, xb = A.augment_images(src, HW, inv, out_hw, want_u8=True, color=torch.from_numpy(rows).cuda())
    assert _same(u8b, u8) and _same(xb, x)
    # either output alone, into buffers the caller owns (sentinels: every element is written)
    only_u8 = torch.full((3, *out_hw, 3), 7, dtype=torch.uint8, device="cuda")
    got = A.augment_images(src, HW, inv, out_hw, out_u8=only_u8, want_f32=False, color=rows)
    assert got[0] is only_u8 and got[1] is None and _same(only_u8, ref_u8)
    only_x = torch.full((3, 3, *out_hw), float("nan"), device="cuda")
    got = A.augment_images(src, HW, inv, out_hw, out_f32=only_x, color=rows)
    assert got[0] is None and got[1] is only_x and _same(only_x, ref_x)
    if name == "identity_and_clamps":       # the identity row: ppn_augment_images' bytes from the same call arguments
        pu8, px = A.augment_images(src, HW, inv, out_hw, want_u8=True)
        assert _same(u8[0], pu8[0]) and _same(x[0], px[0]) and _same(pu8, plain_u8)
        assert (ref_u8[2] == 255).all()


@pytest.mark.parametrize("name", ["random", "saturation_and_noise"])
def test_colour_images_misaligned_planes_take_the_scalar_path(pictures, name):
    """out_w % 4 == 0 but dst_f32 starts 4 bytes off a 16-byte boundary (dst_u8 one byte off 4): scalar stores, same bits,
    and nothing written in front of or behind the views."""
    A, _ = _mods()
    rows, inv = _rows(name), _inv(name, VEC)
    ref_u8, ref_x = J.augment_images_color_ref(pictures, HW, inv, rows, VEC)
    n = 3 * 3 * VEC[0] * VEC[1]
    base_x = torch.full((n + 2,), -5.0, device="cuda")
    base_u8 = torch.full((n + 2,), 9, dtype=torch.uint8, device="cuda")
    assert base_x.data_ptr() % 16 == 0 and base_u8.data_ptr() % 4 == 0
    x, u8 = base_x[1:n + 1].view(3, 3, *VEC), base_u8[1:n + 1].view(3, *VEC, 3)
    A.augment_images(pictures, HW, inv, VEC, out_u8=u8, out_f32=x, color=rows)
    assert _same(x, ref_x) and _same(u8, ref_u8)
    assert base_x[0].item() == -5.0 and base_x[-1].item() == -5.0 and base_u8[0].item() == 9 and base_u8[-1].item() == 9
    A.augment_images(pictures, HW, inv, VEC, out_f32=x)             # the plain kernel on the same view
    assert _same(x, R.augment_images_ref(pictures, HW, inv, VEC)[1])


def test_mirrored_identity_size_is_the_flipped_picture(pictures):
    A, _ = _mods()
    hw = HW[1:2]
    inv = _f32(A.affine_matrices(0.0, 1.0, (0, 0, 0, 0), hw, (40, 56), mirror=True)[1])
    for color in (None, np.array([J.IDENTITY])):
        u8, x = A.augment_images(pictures[1:2], hw, inv, (40, 56), want_u8=True, color=color)
        assert _same(u8, np.ascontiguousarray(pictures[1:2, :, ::-1]))
        assert _same(x, J.normalise(np.ascontiguousarray(pictures[1:2, :, ::-1])))


def test_colour_image_full_size_from_200x300():
    """The training geometry: 384 x 384 from one 200 x 300 picture, mirrored, with a sampled row (147 456 noise draws)."""
    A, _ = _mods()
    hw = np.array([[200, 300]], np.int32)
    src = np.random.default_rng(5).integers(0, 256, (1, 200, 300, 3), dtype=np.uint8)
    p = A.sample_params(23, 1, hw, (384, 384), "train", mirror_p=1.0, color=A.ColorJitter(noise=(6.0, 6.0)))
    assert p["mirror"].all() and p["color"][0, 7] == 768
    ref_u8, ref_x = J.augment_images_color_ref(src, hw, p["inv"], p["color"], (384, 384))
    assert ref_u8.any()
    u8, x = A.augment_images(src, hw, p["inv"], (384, 384), want_u8=True, color=p["color"])
    assert _same(u8, ref_u8) and _same(x, ref_x)


def test_colour_rejects_bad_arguments(pictures):
    A, _ = _mods()
    from pytorch_pose_proposal_network_amd.lib import PPNError
    inv = _inv("random", VEC)
    with pytest.raises(ValueError):
        A.augment_images(pictures, HW, inv, VEC, color=np.zeros((2, 10), np.int32))
    with pytest.raises(PPNError):
        A.augment_images(pictures, HW, inv, VEC, want_f32=False, color=_rows("random"))      # no output asked for


# -------------------------------------------------------------------------------------------------------------- labels

def _people(rng, n, w, h, nk, far=(), corner=()):
    """n packed rows inside a w x h picture: absent keypoints, asymmetric visible masks with hidden in-frame keypoints and
    labeled absent ones; rows in `far` have every keypoint far outside any frame, rows in `corner` only two keypoints, in
    the top-left corner (a zoom about the centre empties them, mirrored or not; a resize keeps them)."""
    P = np.zeros((n, 5 + 2 * nk), np.float32)
    V = np.zeros(n, np.int32)
    for i in range(n):
        P[i, 0:2] = rng.uniform(0, [w, h])
        P[i, 2:4] = rng.integers(0, 30, 2)
        P[i, 4] = 8 + i
        pts = rng.uniform(0, [w - 1, h - 1], (nk, 2)).astype(np.float32)
        pts[rng.random(nk) < 0.2] = 0
        if i in far:
            pts = pts + np.float32(5000)
        if i in corner:
            pts[:] = 0
            pts[[0, nk - 1]] = [[1.5, 1.0], [3.0, 2.25]]
        P[i, 5:] = pts.reshape(-1)
        V[i] = int(rng.integers(0, 1 << nk))
    return P, V


def _label_batch(pmax, counts, seed, nk=K - 1):
    """Three images; image 0 loses people first / last / in the middle.  Rows beyond `count` hold stale people."""
    rng = np.random.default_rng(seed)
    people, visible = np.zeros((3, pmax, 5 + 2 * nk), np.float32), np.zeros((3, pmax), np.int32)
    for b, (far, corner) in enumerate((({0, pmax - 1} | set(range(2, pmax - 1, 3)), ()), ((), {0, 2}), ({1}, {0}))):
        people[b], visible[b] = _people(rng, pmax, 56, 40, nk, far, corner)
    return people, visible, np.asarray(counts, np.int32)


def _entry(packed, fwd, mirror, table, out_hw):
    """ppn_augment_people_mirror itself (mirror None -> NULL), into dirty outputs."""
    from pytorch_pose_proposal_network_amd import lib as L
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (*packed, fwd)]
    md = torch.tensor(mirror, dtype=torch.int32, device="cuda") if mirror is not None else None
    B, pmax, row = packed[0].shape
    out = (torch.full((B, pmax, row), 3.0, device="cuda"), torch.full((B, pmax), -1, dtype=torch.int32, device="cuda"),
           torch.full((B,), -1, dtype=torch.int32, device="cuda"))
    L.check(L.load().ppn_augment_people_mirror(*[t.data_ptr() for t in dev], md.data_ptr() if md is not None else None,
                                               (C.c_int32 * len(table))(*table), B, pmax, len(table), out_hw[0], out_hw[1],
                                               *[t.data_ptr() for t in out], L.current_stream_ptr()),
            "ppn_augment_people_mirror")
    return out


@pytest.mark.parametrize("pmax", [3, 70, 300])
def test_people_bit_exact(pmax):
    """pmax 3, 70 (more people than a wavefront has lanes) and 300 (more than the kernel's 256-person chunk); flags [1, 0, 1];
    counts of 0 and beyond pmax in mirrored and unmirrored images."""
    A, _ = _mods()
    hw = np.tile(np.array([[40, 56]], np.int32), (3, 1))
    flags = [1, 0, 1]
    p = A.sample_params(29, 2, hw, VEC, "train")
    fwds = (("train", _f32(A.affine_matrices(p["theta"], p["scale"], p["crop"], hw, VEC, mirror=flags)[0])),
            ("resize", _f32(A.affine_matrices(0.0, 1.0, (0, 0, 0, 0), hw, VEC, mirror=flags)[0])),
            ("crop", _f32(A.affine_matrices(33.0, 1.6, (3, 2, 1, 4), hw, VEC, mirror=flags)[0])))
    for counts in ([pmax, pmax + 5, max(pmax - 1, 1)], [0, pmax, pmax + 7]):
        packed = _label_batch(pmax, counts, 100 + pmax + counts[0])
        for name, fwd in fwds:
            rp, rv, rc = J.augment_people_mirror_ref(*packed, fwd, flags, KP, VEC)
            plain = R.augment_people_ref(*packed, fwd, VEC)
            if counts[0]:
                assert not _same(rp[0], plain[0][0]) and not _same(rv[0], plain[1][0])       # the swap does something
                assert _same(rp[1], plain[0][1]) and _same(rc, plain[2])
            if name == "resize":
                assert rc[0] == min(counts[0], pmax) - (len({0, pmax - 1} | set(range(2, pmax - 1, 3))) if counts[0] else 0)
            if name == "resize":
                assert rc[1] == pmax
            if name == "crop":                                        # the corner people are emptied by the crop itself
                assert rc[1] <= pmax - 2 and rc[2] <= min(counts[2], pmax) - 2
            po, vo, co = A.augment_people(packed, fwd, VEC, mirror=np.array(flags, bool), kp_mirror=KP)
            assert _same(co, rc), (co, rc)
            assert _same(vo, rv)
            assert _same(po, rp)                                      # the zeroed tail included
            # device tensors in, caller-owned (dirty) outputs, the default table
            out = (torch.full((3, pmax, ROW), 3.0, device="cuda"), torch.full((3, pmax), -1, dtype=torch.int32, device="cuda"),
                   torch.full((3,), -1, dtype=torch.int32, device="cuda"))
            got = A.augment_people(tuple(torch.from_numpy(a).cuda() for a in packed), torch.from_numpy(fwd).cuda(), VEC,
                                   out=out, mirror=torch.tensor(flags, dtype=torch.int32, device="cuda"))
            assert got[0] is out[0] and _same(out[0], rp) and _same(out[1], rv) and _same(out[2], rc)
            # mirror NULL and all-zero flags: ppn_augment_people's bytes
            old = A.augment_people(packed, fwd, VEC)
            assert all(_same(a, b) for a, b in zip(old, plain))
            for none in (None, [0, 0, 0]):
                assert all(_same(a, b) for a, b in zip(_entry(packed, fwd, none, KP, VEC), old)), none


def test_people_with_a_hand_made_table():
    """K = 3: (instance, left, right) with the table [0, 2, 1]; and K = 1, where there is nothing to swap."""
    A, _ = _mods()
    flags = [1, 0, 1]
    hw = np.tile(np.array([[40, 56]], np.int32), (3, 1))
    fwd = _f32(A.affine_matrices(10.0, 1.2, (0, 1, 2, 0), hw, VEC, mirror=flags)[0])
    packed = _label_batch(5, [5, 5, 4], 9, nk=2)
    packed[1][:] |= 0b100                                             # a bit without a slot is copied
    rp, rv, rc = J.augment_people_mirror_ref(*packed, fwd, flags, [0, 2, 1], VEC)
    assert rc.sum() > 3 and (rv & 0b100).any()
    po, vo, co = A.augment_people(packed, fwd, VEC, mirror=flags, kp_mirror=[0, 2, 1])
    assert _same(co, rc) and _same(vo, rv) and _same(po, rp)
    assert all(_same(a, b) for a, b in zip(_entry(packed, fwd, flags, [0, 2, 1], VEC), (rp, rv, rc)))
    with pytest.raises(ValueError):
        A.augment_people(packed, fwd, VEC, mirror=flags)              # rows of K = 3 against the project's 18-entry table
    from pytorch_pose_proposal_network_amd.lib import PPNError
    with pytest.raises(PPNError):
        A.augment_people(packed, fwd, VEC, mirror=flags, kp_mirror=[0, 1, 1])
    lone = (np.zeros((3, 2, 5), np.float32), np.zeros((3, 2), np.int32), np.array([2, 1, 0], np.int32))
    got = _entry(lone, fwd, flags, [0], VEC)
    assert not got[0].any() and not got[1].any() and not got[2].any()      # nobody has a keypoint: everybody is dropped


# ------------------------------------------------------------------------------------------------------------- handoff

SEED, STEP = 3, 5


@pytest.fixture(scope="module")
def handoff():
    from pytorch_pose_proposal_network_amd import synth
    A, T = _mods()
    hw = np.array([[80, 100], [64, 70], [96, 96], [50, 90]], np.int32)
    src = np.full((4, 96, 100, 3), 255, np.uint8)
    rng = np.random.default_rng(78)
    for b, (h, w) in enumerate(hw):
        src[b, :h, :w] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    lists = [synth.synthetic_people(300 + b, insize=(int(w), int(h))) for b, (h, w) in enumerate(hw)]
    return src, hw, T.pack_people(lists, pmax=6)


def test_train_augmenter_with_both_options_equals_the_restatement(handoff):
    from oracle import targets_ref
    A, T = _mods()
    src, hw, packed = handoff
    cj = A.ColorJitter()
    aug = A.TrainAugmenter(insize=(96, 96), seed=SEED, mode="train", mirror_p=0.5, color=cj)
    dev_in = (torch.from_numpy(src).cuda(), tuple(torch.from_numpy(a).cuda() for a in packed))
    x, tg = aug(dev_in[0], hw, dev_in[1], step=STEP)
    p = aug.params
    want = A.sample_params(SEED, STEP, hw, (96, 96), "train", mirror_p=0.5, color=cj)
    assert all(_same(p[k], want[k]) for k in want)
    assert 0 < p["mirror"].sum() < 4 and (p["color"][:, 7] > 0).any()     # mirrored and unmirrored images in one batch
    ref_x, ref_t, (rp, rv, rc) = J.pipeline_ref(src, hw, packed, p, (96, 96), KP, targets_ref)
    assert rc[p["mirror"]].sum() > 0 and rc[~p["mirror"]].sum() > 0
    assert _same(x, ref_x)
    assert sorted(ref_t) == sorted(T.TARGET_KEYS)
    for k in T.TARGET_KEYS:
        assert _same(tg[k], ref_t[k]), k
    assert tg["delta"].sum() > 0 and "limb_c" in tg
    first_x, first = x.clone(), {k: v.clone() for k, v in tg.items()}
    # the second and third calls of this geometry allocate nothing, reuse every buffer, and step 5 comes back identical
    ptrs = (x.data_ptr(), {k: v.data_ptr() for k, v in tg.items()})
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    x6, tg6 = aug(dev_in[0], hw, dev_in[1], step=STEP + 1)
    assert not _same(aug.params["color"], p["color"])
    x5, tg5 = aug(dev_in[0], hw, dev_in[1], step=STEP)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert (x5.data_ptr(), {k: v.data_ptr() for k, v in tg5.items()}) == ptrs
    assert _same(x5, first_x) and all(_same(tg5[k], first[k]) for k in first)
    # each option alone
    for kw in (dict(mirror_p=1.0), dict(color=cj)):
        a1 = A.TrainAugmenter(insize=(96, 96), seed=SEED, **kw)
        x1, t1 = a1(src, hw, packed, step=STEP)
        rx, rt, _ = J.pipeline_ref(src, hw, packed, a1.params, (96, 96), KP, targets_ref)
        assert _same(x1, rx) and all(_same(t1[k], rt[k]) for k in T.TARGET_KEYS), kw


def test_train_augmenter_defaults_and_val_mode_are_unchanged(handoff):
    A, T = _mods()
    src, hw, packed = handoff
    dev_in = (torch.from_numpy(src).cuda(), tuple(torch.from_numpy(a).cuda() for a in packed))
    aug = A.TrainAugmenter(insize=(96, 96), seed=SEED)
    x, tg = aug(dev_in[0], hw, dev_in[1], step=STEP)
    p = A.sample_params(SEED, STEP, hw, (96, 96), "train")
    assert sorted(aug.params) == sorted(p) and all(_same(aug.params[k], p[k]) for k in p)
    # the calls as they were before the options existed
    _, px = A.augment_images(dev_in[0], hw, p["inv"], (96, 96))
    people = A.augment_people(dev_in[1], p["fwd"], (96, 96))
    pt = T.encode_targets(people, (96, 96), (6, 6))
    assert _same(x, px) and sorted(tg) == sorted(pt) and all(_same(tg[k], pt[k]) for k in pt)
    assert _same(x, R.augment_images_ref(src, hw, p["inv"], (96, 96))[1])
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    aug(dev_in[0], hw, dev_in[1], step=STEP + 1)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    # val mode ignores both options
    plain = A.TrainAugmenter(insize=(96, 96), seed=SEED, mode="val")
    xv, tv = plain(src, hw, packed, step=STEP)
    xv, tv = xv.clone(), {k: v.clone() for k, v in tv.items()}
    opt = A.TrainAugmenter(insize=(96, 96), seed=SEED, mode="val", mirror_p=1.0, color=A.ColorJitter())
    xo, to = opt(src, hw, packed, step=STEP)
    assert _same(xo, xv) and all(_same(to[k], tv[k]) for k in tv)
    assert _same(xv, R.augment_images_ref(src, hw, A.sample_params(0, 0, hw, (96, 96), "val")["inv"], (96, 96))[1])


def test_trainer_takes_the_jittered_mirrored_batch(handoff):
    """One PPNTrainer.train_step (DRN-D-22, first-order) on what TrainAugmenter(mirror_p, color) returns, unchanged."""
    A, _ = _mods()
    from pytorch_pose_proposal_network_amd import lib as L, synth
    from pytorch_pose_proposal_network_amd.trainer import PPNTrainer
    src, hw, packed = handoff
    aug = A.TrainAugmenter(insize=(96, 96), seed=SEED, mirror_p=0.5, color=A.ColorJitter())
    x, tg = aug(src, hw, packed, step=STEP)
    assert aug.params["mirror"].any() and x.shape == (4, 3, 96, 96)
    tr = PPNTrainer("drn_d_22", synth.make_state_dict("drn_d_22", 0), compute_dtype=L.PPN_F32, insize=(96, 96),
                    second_order=False)
    losses, w = tr.train_step(x, tg)
    torch.cuda.synchronize()
    losses, w = losses.cpu().numpy(), w.cpu().numpy()
    assert losses.shape == (5,) and np.isfinite(losses).all() and (losses > 0).all() and np.isfinite(w).all()
