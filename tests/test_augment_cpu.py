"""Train-time augmentation, host side (no GPU): the parameter sampler of pytorch_pose_proposal_network_amd/augment.py and
the properties of the NumPy restatement tests/augment_ref.py that tests/test_augment_gpu.py holds the kernels to."""
import numpy as np
import pytest

import augment_ref as R

K = 18
ROW = 5 + 2 * (K - 1)


def _aug():
    from pytorch_pose_proposal_network_amd import augment
    return augment


def _f32(m):
    return np.ascontiguousarray(m[:, :2, :], np.float32)


def _person(points, bbox=(20.0, 20.0, 10.0, 10.0), size=12.0, vis=None):
    pts = np.zeros((K - 1, 2), np.float32)
    pts[:len(points)] = points
    return dict(bbox=bbox, size=size, points=pts, visible=[True] * (K - 1) if vis is None else vis)


def _pack(lists, pmax=0):
    from pytorch_pose_proposal_network_amd import config, targets
    assert config.K == K
    return targets.pack_people(lists, pmax)


# ------------------------------------------------------------------------------------------------------------- sampler

def test_sampler_is_deterministic_and_step_keyed():
    A = _aug()
    hw = np.array([[200, 300], [480, 640], [17, 23]], np.int32)
    a, b = A.sample_params(7, 3, hw, (384, 384), "train"), A.sample_params(7, 3, hw, (384, 384), "train")
    assert sorted(a) == ["crop", "fwd", "inv", "scale", "theta"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["fwd"].dtype == np.float32 and a["fwd"].shape == (3, 2, 3) and a["inv"].shape == (3, 2, 3)
    assert a["crop"].dtype == np.int32 and a["crop"].shape == (3, 4)
    c = A.sample_params(7, 4, hw, (384, 384), "train")
    d = A.sample_params(8, 3, hw, (384, 384), "train")
    for other in (c, d):
        assert not np.array_equal(a["theta"], other["theta"]) and not np.array_equal(a["fwd"], other["fwd"])
    assert len(set(a["theta"].tolist())) == 3                       # images of one batch draw from their own streams


def test_sampler_ranges_over_1000_draws():
    A = _aug()
    hw = np.tile(np.array([[211, 317]], np.int32), (1000, 1))
    p = A.sample_params(1, 0, hw, (384, 384), "train")
    assert p["theta"].min() >= -40 and p["theta"].max() <= 40 and p["theta"].min() < -35 and p["theta"].max() > 35
    assert p["scale"].min() >= 0.35 and p["scale"].max() <= 2.5 and p["scale"].min() < 0.5 and p["scale"].max() > 2.3
    top, right, bottom, left = p["crop"].T
    assert top.min() >= 0 and bottom.min() >= 0 and max(top.max(), bottom.max()) <= int(0.1 * 211)
    assert left.min() >= 0 and right.min() >= 0 and max(left.max(), right.max()) <= int(0.1 * 317)
    assert top.max() >= 19 and left.max() >= 29                     # the whole range is used
    assert not np.array_equal(top, bottom) and not np.array_equal(left, right)     # one uniform per side


def test_val_mode_is_a_pure_resize():
    A = _aug()
    hw = np.array([[200, 300], [48, 64]], np.int32)
    p = A.sample_params(5, 9, hw, (96, 128), "val")
    assert not p["theta"].any() and (p["scale"] == 1).all() and not p["crop"].any()
    for b, (h, w) in enumerate(hw):
        kx, ky = 128 / w, 96 / h
        want = np.array([[kx, 0, 0.5 * kx - 0.5], [0, ky, 0.5 * ky - 0.5]], np.float32)
        assert np.array_equal(p["fwd"][b], want)
    assert np.array_equal(p["fwd"], A.sample_params(6, 1, hw, (96, 128), "val")["fwd"])      # no randomness at all
    with pytest.raises(ValueError):
        A.sample_params(0, 0, hw, (96, 128), "test")


def test_forward_times_inverse_is_identity_in_float64():
    A = _aug()
    hw = np.tile(np.array([[200, 300], [97, 61]], np.int32), (50, 1))
    p = A.sample_params(3, 1, hw, (384, 384), "train")
    fwd, inv = A.affine_matrices(p["theta"], p["scale"], p["crop"], hw, (384, 384))
    assert fwd.dtype == np.float64 and inv.dtype == np.float64
    eye = np.eye(3)
    # entries reach |translation| ~ 1e3 x |scale| ~ 1e1; float64 rounding of a few products of that size
    assert np.abs(fwd @ inv - eye).max() < 1e-10 and np.abs(inv @ fwd - eye).max() < 1e-10
    assert np.array_equal(p["fwd"], _f32(fwd)) and np.array_equal(p["inv"], _f32(inv))
    assert np.array_equal(fwd[:, 2], np.tile([0, 0, 1.0], (100, 1)))


# --------------------------------------------------------------------------------------------------- oracle properties

def test_identity_copies_picture_and_labels():
    A = _aug()
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (1, 24, 40, 3), dtype=np.uint8)
    fwd, inv = A.affine_matrices(0.0, 1.0, (0, 0, 0, 0), (24, 40), (24, 40))
    assert np.array_equal(fwd[0], np.eye(3)) and np.array_equal(inv[0], np.eye(3))
    u8, x = R.augment_images_ref(src, [(24, 40)], _f32(inv), (24, 40))
    assert np.array_equal(u8, src)
    want = (src.astype(np.float32) - R.MEAN) / R.STD
    assert x.dtype == np.float32 and np.array_equal(x, want.transpose(0, 3, 1, 2))
    # labels: keypoints unchanged (hidden ones too), absent ones stay absent; the box goes through floor(w / 2) and the clip
    vis = [True] * (K - 1)
    vis[1] = False
    a = _person([(3.5, 4.25), (10.0, 20.0), (0.0, 0.0), (39.5, 23.5)], bbox=(20.0, 12.0, 11.0, 7.0), vis=vis)
    b = _person([(5.0, 5.0)], bbox=(38.0, 2.0, 10.0, 8.0))
    pk = _pack([[a, b]])
    po, vo, co = R.augment_people_ref(*pk, _f32(fwd), (24, 40))
    assert co.tolist() == [2]
    assert np.array_equal(po[0, :, 4:], pk[0][0, :, 4:])                                  # size and every keypoint
    assert vo[0, 0] == 0b1001 and vo[0, 1] == 0b1                                         # only labeled-and-present bits stay
    assert po[0, 0, :4].tolist() == [20.0, 12.0, 10.0, 6.0]                               # 11 // 2 = 5, 7 // 2 = 3
    assert po[0, 1, :4].tolist() == [(33 + 40) / 2, (0 + 6) / 2, 7.0, 6.0]                # [33, 43] x [-2, 6] clipped


def test_rotation_by_180_degrees_flips_both_axes():
    A = _aug()
    rng = np.random.default_rng(1)
    src = rng.integers(0, 256, (1, 17, 23, 3), dtype=np.uint8)
    fwd, inv = A.affine_matrices(180.0, 1.0, (0, 0, 0, 0), (17, 23), (17, 23))
    u8, _ = R.augment_images_ref(src, [(17, 23)], _f32(inv), (17, 23))
    assert np.array_equal(u8[0], src[0, ::-1, ::-1])                 # its taps fall on integers
    pk = _pack([[_person([(2.0, 3.0)], bbox=(5.0, 6.0, 4.0, 2.0))]])
    po, _, _ = R.augment_people_ref(*pk, _f32(fwd), (17, 23))
    assert po[0, 0, 5:7].tolist() == [20.0, 13.0] and po[0, 0, :4].tolist() == [17.0, 10.0, 4.0, 2.0]


def test_pixels_and_labels_agree():
    """A bright 3x3 blob centred on a keypoint lands, after a sampled transform with s >= 1, with its intensity centroid
    within 1 pixel of the transformed keypoint."""
    A = _aug()
    hw, out_hw = np.array([[120, 160]], np.int32), (96, 128)
    done = 0
    for step in range(200):
        p = A.sample_params(11, step, hw, out_hw, "train")
        if p["scale"][0] < 1.0:
            continue
        kp = np.array([80.0 + (step % 5) - 2, 60.0 + (step % 3) - 1], np.float32)       # near the centre: stays in frame
        src = np.zeros((1, 120, 160, 3), np.uint8)
        src[0, int(kp[1]) - 1:int(kp[1]) + 2, int(kp[0]) - 1:int(kp[0]) + 2] = 255
        po, vo, co = R.augment_people_ref(*_pack([[_person([tuple(kp)])]]), p["fwd"], out_hw)
        if co[0] == 0:
            continue
        u8, _ = R.augment_images_ref(src, hw, p["inv"], out_hw)
        wgt = u8[0, :, :, 0].astype(np.float64)
        if wgt[0].any() or wgt[-1].any() or wgt[:, 0].any() or wgt[:, -1].any():
            continue                                                 # blob cut by the frame: its centroid is biased
        ys, xs = np.mgrid[0:out_hw[0], 0:out_hw[1]]
        cx, cy = (wgt * xs).sum() / wgt.sum(), (wgt * ys).sum() / wgt.sum()
        assert abs(cx - po[0, 0, 5]) < 1 and abs(cy - po[0, 0, 6]) < 1, (step, cx, cy, po[0, 0, 5:7])
        done += 1
    assert done >= 20


def test_person_leaving_the_frame_is_dropped_and_order_kept():
    A = _aug()
    # magnify 2.5x about the centre of a 40x40 picture: only what lies near the centre stays inside
    fwd, _ = A.affine_matrices(0.0, 2.5, (0, 0, 0, 0), (40, 40), (40, 40))
    f = _f32(fwd)
    near = lambda dx: _person([(19.5 + dx, 19.5), (20.5 + dx, 21.0)], bbox=(20.0, 20.0, 6.0, 6.0), size=10.0 + dx)
    far = _person([(2.0, 3.0), (38.0, 37.0)], bbox=(3.0, 3.0, 4.0, 4.0), size=99.0)
    half = _person([(1.0, 1.0), (21.0, 20.0)], size=50.0)          # one keypoint leaves, one stays: the person stays
    for lists, sizes in (([far, near(0), near(1)], [10, 11]), ([near(0), far, near(1)], [10, 11]),
                         ([near(0), near(1), far], [10, 11]), ([far, half, far, near(2)], [50, 12]), ([far, far], [])):
        pk = _pack([lists], pmax=5)
        po, vo, co = R.augment_people_ref(*pk, f, (40, 40))
        assert co.tolist() == [len(sizes)] and po[0, :len(sizes), 4].tolist() == sizes
        assert not po[0, len(sizes):].any() and not vo[0, len(sizes):].any()
    po, vo, _ = R.augment_people_ref(*_pack([[half]]), f, (40, 40))
    assert po[0, 0, 5:7].tolist() == [0.0, 0.0] and vo[0, 0] == 0b10 and po[0, 0, 7] > 0
    assert R.unpack_people(po, vo, np.array([1]))[0][0]["visible"][:3] == [False, True, False]
