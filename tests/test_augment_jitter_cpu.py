"""The augmentation stage's options, host side (no GPU): the mirror factor of F, the sampler's new streams, the properties of
the NumPy restatement tests/augment_jitter_ref.py that tests/test_augment_jitter_gpu.py holds the kernels to, its agreement
with the target encoder, and the library's argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import augment_jitter_ref as J
import augment_ref as R
import tta_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 18
ROW = 5 + 2 * (K - 1)
KP = tta_ref.KP_MIRROR


def _aug():
    from pytorch_pose_proposal_network_amd import augment
    return augment


def _f32(m):
    return np.ascontiguousarray(m[:, :2, :], np.float32)


def _slot(name):
    from pytorch_pose_proposal_network_amd import config as cfg
    return cfg.KEYPOINT_NAMES.index(name) - 1


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------ geometry

def _parent_cases():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_augment_parent", os.path.join(ROOT, "tests", "golden",
                                                                                      "make_augment_parent.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SAMPLED, mod.DIRECT, np.load(os.path.join(ROOT, "tests", "golden", "augment_parent.npz"))


def test_matrices_without_mirror_are_the_parents_bit_for_bit():
    """tests/golden/augment_parent.npz holds what the code in front of the options returned on test_augment_cpu.py's
    parameter sets: mirror None and mirror all False give those float64 bits."""
    A = _aug()
    sampled, direct, g = _parent_cases()
    for name, seed, step, hw, out_hw, mode in sampled:
        hw = np.asarray(hw, np.int32)
        th, sc, cr = g[f"{name}/theta"], g[f"{name}/scale"], g[f"{name}/crop"]
        for mirror in (None, np.zeros(len(hw), bool), False):
            fwd, inv = A.affine_matrices(th, sc, cr, hw, out_hw, mirror=mirror)
            assert _same(fwd, g[f"{name}/fwd64"]) and _same(inv, g[f"{name}/inv64"]), name
        assert _same(A.affine_matrices(th, sc, cr, hw, out_hw)[0], g[f"{name}/fwd64"])         # the old positional call
    for name, theta, scale, crop, hw, out_hw in direct:
        for mirror in (None, [False]):
            fwd, inv = A.affine_matrices(theta, scale, crop, hw, out_hw, mirror=mirror)
            assert _same(fwd, g[f"{name}/fwd64"]) and _same(inv, g[f"{name}/inv64"]), name


def test_mirror_geometry():
    A = _aug()
    hw = np.tile(np.array([[200, 300], [97, 61]], np.int32), (50, 1))
    p = A.sample_params(3, 1, hw, (384, 384), "train")
    flags = np.arange(100) % 3 != 0
    fwd, inv = A.affine_matrices(p["theta"], p["scale"], p["crop"], hw, (384, 384), mirror=flags)
    plain_f, plain_i = A.affine_matrices(p["theta"], p["scale"], p["crop"], hw, (384, 384))
    eye = np.eye(3)
    assert np.abs(fwd @ inv - eye).max() < 1e-9 and np.abs(inv @ fwd - eye).max() < 1e-9
    assert _same(fwd[~flags], plain_f[~flags]) and _same(inv[~flags], plain_i[~flags])       # per image
    assert np.array_equal(fwd[:, 2], np.tile([0, 0, 1.0], (100, 1)))
    for b in np.where(flags)[0][:10]:                                 # F_mirrored(x, y) = F(w - 1 - x, y): before the rotation
        w = float(hw[b, 1])
        for x, y in ((0.0, 0.0), (17.0, 5.5), (w - 1, 40.0)):
            assert np.allclose(fwd[b] @ [x, y, 1.0], plain_f[b] @ [w - 1 - x, y, 1.0], rtol=0, atol=1e-9)
    # identity size: column i goes to column w - 1 - i exactly, rows stay
    for h, w in ((24, 40), (17, 23)):
        f, i = A.affine_matrices(0.0, 1.0, (0, 0, 0, 0), (h, w), (h, w), mirror=True)
        want = np.array([[-1.0, 0, w - 1], [0, 1, 0], [0, 0, 1]])
        assert np.array_equal(f[0], want) and np.array_equal(i[0], want)
        for col in range(w):
            assert (f[0] @ [col, 3.0, 1.0]).tolist() == [w - 1 - col, 3.0, 1.0]
        src = np.random.default_rng(h).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
        u8, _ = R.augment_images_ref(src, [(h, w)], _f32(i), (h, w))
        assert np.array_equal(u8[0], src[0, :, ::-1])
    # one flag for every image
    f_all, _ = A.affine_matrices(p["theta"], p["scale"], p["crop"], hw, (384, 384), mirror=True)
    assert _same(f_all[flags], fwd[flags])


# ------------------------------------------------------------------------------------------------------------- sampler

def test_sampler_options():
    A = _aug()
    sampled, _, g = _parent_cases()
    cj = A.ColorJitter()
    assert (cj.brightness, cj.contrast, cj.saturation, cj.cast, cj.noise, cj.gray_p) == \
        (32, (0.6, 1.4), (0.5, 1.5), 0.1, (0.0, 8.0), 0.1)
    for name, seed, step, hw, out_hw, mode in sampled[:6]:
        hw = np.asarray(hw, np.int32)
        plain = A.sample_params(seed, step, hw, out_hw, mode)
        assert sorted(plain) == ["crop", "fwd", "inv", "scale", "theta"]            # a call without options: as before
        for k in plain:
            assert _same(plain[k], g[f"{name}/{k}"]), (name, k)
        a = A.sample_params(seed, step, hw, out_hw, mode, mirror_p=0.5, color=cj)
        b = A.sample_params(seed, step, hw, out_hw, mode, mirror_p=0.5, color=cj)
        assert sorted(a) == ["color", "crop", "fwd", "inv", "mirror", "scale", "theta"]
        for k in ("theta", "scale", "crop"):                                          # the geometry's stream did not move
            assert _same(a[k], g[f"{name}/{k}"]), (name, k)
        for k in a:
            assert (a[k] is None and b[k] is None) or _same(a[k], b[k]), k
        assert a["mirror"].dtype == np.bool_ and a["mirror"].shape == (len(hw),)
        if mode == "val":
            assert not a["mirror"].any() and a["color"] is None and _same(a["fwd"], plain["fwd"])
            continue
        assert a["color"].dtype == np.int32 and a["color"].shape == (len(hw), 10)
        m = a["mirror"]
        assert _same(a["fwd"][~m], plain["fwd"][~m]) and _same(a["inv"][~m], plain["inv"][~m])
        f64, i64 = A.affine_matrices(a["theta"], a["scale"], a["crop"], hw, out_hw, mirror=m)
        assert _same(a["fwd"], _f32(f64)) and _same(a["inv"], _f32(i64))
        # the mirror draw does not depend on the colour option, nor the colour rows on mirror_p
        assert _same(A.sample_params(seed, step, hw, out_hw, mode, mirror_p=0.5)["mirror"], m)
        assert A.sample_params(seed, step, hw, out_hw, mode, mirror_p=0.5)["color"] is None
        assert _same(A.sample_params(seed, step, hw, out_hw, mode, color=cj)["color"], a["color"])
        none, every = (A.sample_params(seed, step, hw, out_hw, mode, mirror_p=q, color=cj)["mirror"] for q in (0.0, 1.0))
        assert not none.any() and every.all()
    with pytest.raises(ValueError):
        A.sample_params(0, 0, [[20, 20]], (16, 16), "train", mirror_p=1.5)


def test_option_streams_are_the_documented_ones():
    """mirror: u[0] of stream_seed(stream_seed(key, b), 1); noise key: stream_seed(stream_seed(key, b), 2) -- through prng's
    scalar functions, which the sampler's batched helpers must equal."""
    from pytorch_pose_proposal_network_amd import prng
    A = _aug()
    seeds = [prng.stream_seed(9, i) for i in range(7)] + [0, 2 ** 64 - 1]
    assert [int(v) for v in prng.stream_seeds(seeds, 2)] == [prng.stream_seed(s, 2) for s in seeds]
    assert _same(prng.uniform01_rows(seeds, 9), np.stack([prng.uniform01(s, 9) for s in seeds]))
    hw = np.tile(np.array([[120, 160]], np.int32), (5, 1))
    p = A.sample_params(21, 4, hw, (96, 128), "train", mirror_p=0.3, color=A.ColorJitter(noise=(4.0, 4.0)))
    key = prng.stream_seed(21, 4)
    for b in range(5):
        kb = prng.stream_seed(key, b)
        u = prng.uniform01(prng.stream_seed(kb, 1), 9)
        assert p["mirror"][b] == (u[0] < 0.3)
        nk = prng.stream_seed(kb, 2)
        assert (int(p["color"][b, 8]) & 0xFFFFFFFF) | ((int(p["color"][b, 9]) & 0xFFFFFFFF) << 32) == nk
        assert p["color"][b, 7] == 512
        sat = 0 if u[1] < 0.1 else round(256 * (0.5 + float(u[2])))
        assert p["color"][b, 0] == sat


def test_sampler_ranges_over_1000_draws():
    A = _aug()
    hw = np.tile(np.array([[211, 317]], np.int32), (1000, 1))
    cj = A.ColorJitter()
    p = A.sample_params(1, 0, hw, (384, 384), "train", mirror_p=0.5, color=cj)
    assert 400 < p["mirror"].sum() < 600
    c = p["color"]
    for col, (lo, hi) in enumerate(J.CLAMPS):
        assert c[:, col].min() >= lo and c[:, col].max() <= hi
    grey = c[:, 0] == 0
    assert 50 < grey.sum() < 160                                      # gray_p = 0.1
    assert c[~grey, 0].min() >= 128 and c[~grey, 0].max() <= 384 and c[~grey, 0].min() < 140 and c[~grey, 0].max() > 372
    # gain = round(256 * contrast * cast): contrast in [0.6, 1.4], cast in [0.9, 1.1]
    assert c[:, 1:4].min() >= round(256 * 0.6 * 0.9) and c[:, 1:4].max() <= round(256 * 1.4 * 1.1)
    assert len({tuple(r) for r in c[:, 1:4]}) > 900 and (c[:, 1] != c[:, 2]).any()
    # off = round(128 - 128 * contrast + brightness), one value for the three channels
    assert (c[:, 4] == c[:, 5]).all() and (c[:, 4] == c[:, 6]).all()
    assert c[:, 4].min() >= round(128 - 128 * 1.4 - 32) and c[:, 4].max() <= round(128 - 128 * 0.6 + 32)
    assert c[:, 7].min() >= 0 and c[:, 7].max() <= 1024 and c[:, 7].max() > 1000 and c[:, 7].min() < 24
    assert len({(int(r[8]), int(r[9])) for r in c}) == 1000           # every image has its own noise key
    # folding, on a degenerate jitter: contrast 1.25, brightness exactly +16 / -16 at u = 1 / 0 is not reachable, so pin the
    # formulas through ranges of zero width
    q = A.sample_params(1, 0, hw[:4], (384, 384), "train",
                        color=A.ColorJitter(brightness=0, contrast=(1.25, 1.25), saturation=(0.75, 0.75), cast=0.0,
                                            noise=(2.0, 2.0), gray_p=0.0))["color"]
    assert (q[:, :8] == [192, 320, 320, 320, -32, -32, -32, 256]).all()
    q = A.sample_params(1, 0, hw[:4], (384, 384), "train", color=A.ColorJitter(gray_p=1.0))["color"]
    assert (q[:, 0] == 0).all()


# ---------------------------------------------------------------------------------------------------- restatement: colour

def _picture(seed=0, shape=(1, 24, 40, 3)):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def test_colour_identity_is_the_plain_image():
    A = _aug()
    assert tuple(J.IDENTITY) == A.COLOR_IDENTITY
    hw = np.array([[24, 40], [19, 33]], np.int32)
    src = _picture(1, (2, 24, 40, 3))
    inv = A.sample_params(9, 2, hw, (32, 48), "train")["inv"]
    u8, x = R.augment_images_ref(src, hw, inv, (32, 48))
    rows = np.tile(J.IDENTITY, (2, 1))
    rows[1, 8:] = [12345, -6789]                                      # the key does not matter at noise_q 0
    cu8, cx = J.augment_images_color_ref(src, hw, inv, rows, (32, 48))
    assert _same(cu8, u8) and _same(cx, x)
    # all 256 values and every (y, c) pair
    c, y = np.meshgrid(np.arange(256), np.arange(256))
    assert np.array_equal(y + (((c - y) * 256 + 128) >> 8), c) and np.array_equal((c * 256 + 128) >> 8, c)


def test_colour_rules():
    v = _picture(2)
    # sat 0: three equal channels, the integer luma
    row = J.IDENTITY.copy()
    row[0] = 0
    g = J.color_step(v, row[None])
    px = v.astype(np.int64)
    y = (77 * px[..., 0] + 150 * px[..., 1] + 29 * px[..., 2] + 128) >> 8
    assert all(np.array_equal(g[..., c], y) for c in range(3)) and y.max() <= 255
    # both clamp ends: gain 1024 (4x) with offset -255, gain 0 with offset 255
    hi = J.color_step(v, np.array([[256, 1024, 1024, 1024, -255, -255, -255, 0, 0, 0]]))
    assert np.array_equal(hi, np.clip(4 * px - 255, 0, 255)) and (hi == 0).any() and (hi == 255).any()
    lo = J.color_step(v, np.array([[256, 0, 0, 0, 255, 255, 255, 0, 0, 0]]))
    assert (lo == 255).all()
    assert (J.color_step(v, np.array([[256, 0, 0, 0, -255, -255, -255, 0, 0, 0]])) == 0).all()
    # parameters beyond the ranges are clamped to them
    wild = J.color_step(v, np.array([[9999, 5000, -7, 1024, 999, -999, 0, 0, 0, 0]]))
    tame = J.color_step(v, np.array([[512, 1024, 0, 1024, 255, -255, 0, 0, 0, 0]]))
    assert np.array_equal(wild, tame)
    # by hand, c < y: (r, g, b) = (10, 200, 30): y = (770 + 30000 + 870 + 128) >> 8 = 31768 >> 8 = 124;  sat 300:
    #   r: (10 - 124) * 300 + 128 = -34072;  -34072 >> 8 = floor(-133.09) = -134 (truncation would give -133);  124 - 134 -> 0
    #   b: (30 - 124) * 300 + 128 = -28072;  floor(-109.66) = -110;  124 - 110 = 14
    #   g: (200 - 124) * 300 + 128 = 22928;  22928 >> 8 = 89;  124 + 89 = 213
    # and sat 77 for r: -114 * 77 + 128 = -8650;  floor(-33.79) = -34;  124 - 34 = 90 (truncation: 91)
    one = np.array([[[[10, 200, 30]]]], np.uint8)
    assert J.color_step(one, np.array([[300, 256, 256, 256, 0, 0, 0, 0, 0, 0]]))[0, 0, 0].tolist() == [0, 213, 14]
    assert J.color_step(one, np.array([[77, 256, 256, 256, 0, 0, 0, 0, 0, 0]]))[0, 0, 0, 0] == 90
    # gain then offset: c1 = 90, gain 300: (27000 + 128) >> 8 = 105, offset -7 -> 98
    assert J.color_step(one, np.array([[77, 300, 256, 256, -7, 0, 0, 0, 0, 0]]))[0, 0, 0, 0] == 98


def test_noise():
    from pytorch_pose_proposal_network_amd import prng
    key = prng.stream_seed(2024, 7)
    lo, hi = (int(x) for x in np.array([key], np.uint64).view(np.int32))
    grey = np.full((1, 64, 64, 3), 128, np.uint8)
    row = J.IDENTITY.copy()
    row[8:] = [lo, hi]
    assert np.array_equal(J.color_step(grey, row[None]), grey)        # noise_q 0 adds nothing, whatever the key
    assert not J.noise_field(lo, hi, 0, (64, 64)).any()
    row[7] = 1024
    d = J.color_step(grey, row[None]).astype(np.int64) - 128          # 128 +- 24 never clamps: this is d itself
    assert np.array_equal(d[0], J.noise_field(lo, hi, 1024, (64, 64)))
    for c in range(3):
        assert abs(d[..., c].mean()) <= 0.5 and 7.5 <= d[..., c].std() <= 8.5, (c, d[..., c].mean(), d[..., c].std())
    assert np.abs(d).max() <= 24                                      # |s| <= 381: (381 * 1024 + 8192) >> 14 = 24
    assert abs(np.corrcoef(d[..., 0].ravel(), d[..., 1].ravel())[0, 1]) < 0.05      # the channels use disjoint bits
    # the stream is prng.raw_u64's, element idx = oy * out_w + ox: pixel (oy, ox) = (3, 5) of a 64-wide image by hand
    z = int(prng.raw_u64(key, 64 * 64)[3 * 64 + 5])
    for c in range(3):
        t = (z >> (21 * c)) & 0x1FFFFF
        s = 2 * ((t & 127) + ((t >> 7) & 127) + ((t >> 14) & 127)) - 381
        assert d[0, 3, 5, c] == (s * 1024 + 8192) >> 14
    # another out_w indexes the same stream differently; another key gives another field
    assert not np.array_equal(J.noise_field(lo, hi, 1024, (64, 32))[:, :, 0], d[0, :, :32, 0])
    assert np.array_equal(J.noise_field(lo, hi, 1024, (128, 32)).reshape(-1, 3), d[0].reshape(-1, 3))
    assert not np.array_equal(J.noise_field(lo + 1, hi, 1024, (64, 64)), d[0])
    # the clamp at 4096, and saturation at the ends of the u8 range
    row[7] = 99999
    big = J.color_step(grey, row[None]).astype(np.int64) - 128
    assert np.array_equal(big[0], J.noise_field(lo, hi, 4096, (64, 64))) and 31 <= big.std() <= 33
    dark = J.color_step(np.zeros((1, 64, 64, 3), np.uint8), row[None])
    assert (dark == 0).mean() > 0.45 and dark.max() > 60


# ---------------------------------------------------------------------------------------------------- restatement: labels

def _person(points, bbox=(20.0, 12.0, 10.0, 8.0), size=12.0, vis=None):
    pts = np.zeros((K - 1, 2), np.float32)
    for slot, xy in points.items():
        pts[slot] = xy
    return dict(bbox=bbox, size=size, points=pts, visible=[True] * (K - 1) if vis is None else vis)


def _pack(lists, pmax=0):
    from pytorch_pose_proposal_network_amd import targets
    return targets.pack_people(lists, pmax)


def test_mirror_tables_are_the_projects():
    from pytorch_pose_proposal_network_amd import tta
    assert tta.mirror_tables()[0] == KP and _slot("left_wrist") != _slot("right_wrist")
    assert KP[_slot("left_wrist") + 1] - 1 == _slot("right_wrist")


def test_mirroring_twice_returns_the_labels():
    A = _aug()
    h, w = 40, 56
    rng = np.random.default_rng(3)
    people = np.zeros((2, 4, ROW), np.float32)
    people[:, :, 0:2] = rng.integers(10, 30, (2, 4, 2))
    people[:, :, 2:4] = 2 * rng.integers(1, 5, (2, 4, 2))             # even sizes: floor(w / 2) loses nothing
    people[:, :, 4] = rng.integers(8, 20, (2, 4))
    pts = rng.integers(1, [w - 1, h - 1], (2, 4, K - 1, 2)).astype(np.float32)
    pts[rng.random((2, 4, K - 1)) < 0.2] = 0                          # absent keypoints
    people[:, :, 5:] = pts.reshape(2, 4, -1)
    present = (pts != 0).any(-1)
    bits = (rng.random((2, 4, K - 1)) < 0.6) & present                # asymmetric masks; only present keypoints are labeled
    visible = (bits * (1 << np.arange(K - 1))).sum(-1).astype(np.int32)
    count = np.array([4, 3], np.int32)
    people[1, 3], visible[1, 3] = 0, 0
    fwd = _f32(A.affine_matrices(0.0, 1.0, (0, 0, 0, 0), (h, w), (h, w), mirror=True)[0])
    fwd = np.tile(fwd, (2, 1, 1))
    once = J.augment_people_mirror_ref(people, visible, count, fwd, [1, 1], KP, (h, w))
    assert not np.array_equal(once[0], people) and not np.array_equal(once[1], visible) and once[2].tolist() == [4, 3]
    twice = J.augment_people_mirror_ref(*once, fwd, [1, 1], KP, (h, w))
    assert _same(twice[0], people) and _same(twice[1], visible) and _same(twice[2], count)
    # flags [1, 0]: the second image sees only F; no flags / None: augment_ref itself
    mixed = J.augment_people_mirror_ref(people, visible, count, fwd, [1, 0], KP, (h, w))
    plain = R.augment_people_ref(people, visible, count, fwd, (h, w))
    assert _same(mixed[0][0], once[0][0]) and _same(mixed[0][1], plain[0][1]) and _same(mixed[1][1], plain[1][1])
    for flags in (None, [0, 0]):
        got = J.augment_people_mirror_ref(people, visible, count, fwd, flags, KP, (h, w))
        assert all(_same(a, b) for a, b in zip(got, plain))


def test_left_wrist_alone_comes_out_as_right_wrist():
    A = _aug()
    h, w = 40, 56
    lw, rw = _slot("left_wrist"), _slot("right_wrist")
    vis = [False] * (K - 1)
    vis[lw] = True
    vis[rw] = True                                                    # labeled but out of frame: its bit must not survive
    lone = _person({lw: (10.0, 7.0), rw: (500.0, 7.0)}, vis=vis)
    gone = _person({rw: (500.0, 7.0)}, size=99.0)                     # nothing in frame: dropped, mirrored or not
    pk = _pack([[gone, lone]], pmax=3)
    fwd = _f32(A.affine_matrices(0.0, 1.0, (0, 0, 0, 0), (h, w), (h, w), mirror=True)[0])
    po, vo, co = J.augment_people_mirror_ref(*pk, fwd, [1], KP, (h, w))
    assert co.tolist() == [1] and po[0, 0, 4] == 12.0
    want = np.zeros(2 * (K - 1), np.float32)
    want[2 * rw:2 * rw + 2] = [w - 1 - 10.0, 7.0]
    assert np.array_equal(po[0, 0, 5:], want) and vo[0, 0] == 1 << rw
    assert po[0, 0, :4].tolist() == [w - 1 - 20.0, 12.0, 10.0, 8.0]  # the box is mirrored by F, not permuted
    assert not po[0, 1:].any() and not vo[0, 1:].any()
    # a hidden left wrist: the person survives, in the right slot, with no bit
    vis[lw] = False
    po, vo, co = J.augment_people_mirror_ref(*_pack([[_person({lw: (10.0, 7.0)}, vis=vis)]]), fwd, [1], KP, (h, w))
    assert co.tolist() == [1] and np.array_equal(po[0, 0, 5:], want) and vo[0, 0] == 0


def test_small_hand_made_table():
    """K = 3: keypoints (instance, left, right)."""
    people = np.array([[[10, 10, 4, 4, 7, 1, 2, 3, 4], [10, 10, 4, 4, 8, 5, 6, 0, 0]]], np.float32)
    visible = np.array([[0b01, 0b01]], np.int32)
    fwd = np.array([[[1, 0, 0], [0, 1, 0]]], np.float32)
    po, vo, co = J.augment_people_mirror_ref(people, visible, [2], fwd, [1], [0, 2, 1], (20, 20))
    assert po[0, :, 5:].tolist() == [[3, 4, 1, 2], [0, 0, 5, 6]] and vo[0].tolist() == [0b10, 0b10] and co.tolist() == [2]


# --------------------------------------------------------------------------------------------------- encoder consistency

def _planted_people(seed=5):
    """Three people whose keypoints of one kind never share a cell, every coordinate 16 c + f with an integer f in 2..13: at
    least 2 px from a cell border, before and after x -> 383 - x (f -> 15 - f)."""
    rng = np.random.default_rng(seed)
    people = []
    for n, (ccx, ccy) in enumerate(((6, 6), (12, 16), (17, 8))):
        def point(dx, dy):
            return np.array([16 * (ccx + dx) + int(rng.integers(2, 14)), 16 * (ccy + dy) + int(rng.integers(2, 14))],
                            np.float32)
        root = point(0, 0)
        pts = np.stack([point(int(rng.integers(-3, 4)), int(rng.integers(-3, 4))) for _ in range(K - 1)])
        vis = np.ones(K - 1, bool)
        vis[_slot("left_wrist") if n == 0 else _slot("right_knee")] = n == 2      # one-sided hidden joints on two people
        people.append(dict(bbox=(root[0], root[1], np.float32(96), np.float32(128)), points=pts, visible=vis,
                           size=np.float32(16)))
    return people


def test_mirrored_labels_encode_to_the_mirrored_targets():
    """Val-mode resize at identity size, mirrored, then oracle/targets_ref.encode_targets.  The mirror here is the augmenter's
    pixel-index convention, x -> w - 1 - x on pixel centres at integers (a point at 16 c + f lands at 16 (23 - c) + 15 - f),
    NOT the 1 - x that tta.py applies to cell-relative offsets; so only the supports are compared, not tx."""
    from oracle import targets_ref as T
    A = _aug()
    people = _planted_people()
    pk = _pack([people])
    hw = np.array([[384, 384]], np.int32)
    p = A.sample_params(0, 0, hw, (384, 384), "val")
    assert np.array_equal(p["fwd"][0], [[1, 0, 0], [0, 1, 0]])
    fwd = _f32(A.affine_matrices(p["theta"], p["scale"], p["crop"], hw, (384, 384), mirror=[True])[0])
    po, vo, co = J.augment_people_mirror_ref(*pk, fwd, [1], KP, (384, 384))
    assert co.tolist() == [3]
    a = T.encode_targets(people)
    m = T.encode_targets(R.unpack_people(po, vo, co)[0])
    assert int(a["delta"].sum()) == 3 * K - 2 and int(a["te"].sum()) > 30
    assert np.array_equal(m["delta"], a["delta"][KP][:, :, ::-1])     # grid column j -> W - 1 - j, channels through kp_mirror
    assert not np.array_equal(m["delta"], a["delta"][:, :, ::-1])     # ... and the channel swap matters
    for k in ("tw", "th", "ty", "weight"):
        assert np.array_equal(m[k], a[k][KP][:, :, ::-1]), k
    te = a["te"][tta_ref.EDGE_MIRROR][:, :, ::-1][..., ::-1]          # edges through edge_mirror, lx -> sW - 1 - lx, j -> W - 1 - j
    assert np.array_equal(m["te"], te)
    assert np.array_equal(m["weight_ij"], a["weight_ij"][tta_ref.EDGE_MIRROR][:, :, ::-1][..., ::-1])
    on = a["delta"][KP][:, :, ::-1] != 0                              # tx: f / 16 -> (15 - f) / 16, the pixel-index mirror
    assert np.array_equal(m["tx"][on], (np.float32(15 / 16) - a["tx"][KP][:, :, ::-1][on]))


# ------------------------------------------------------------------------------------------------------------- library

def _lib():
    from pytorch_pose_proposal_network_amd import build, lib
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lib


def test_library_without_a_gpu():
    lib = _lib()
    l = lib.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    for name in ("ppn_augment_images_color", "ppn_augment_people_mirror"):
        assert f" T {name}" in out and name in lib.EXPORTS
    bad = -1                                                          # PPN_E_INVALID
    # addresses that are never dereferenced: every rejection happens before anything is launched
    S, HW, INV, COL, U8, X = (0x10000000 * (i + 1) for i in range(6))
    img = lambda *p: l.ppn_augment_images_color(*p[:4], 2, 40, 56, 32, 48, p[4], p[5], None)
    for args in ((None, HW, INV, COL, U8, X), (S, None, INV, COL, U8, X), (S, HW, None, COL, U8, X),
                 (S, HW, INV, None, U8, X), (S, HW, INV, COL, None, None)):
        assert img(*args) == bad and b"NULL" in l.ppn_last_error(), args
    for args in ((S, HW, INV, COL, S, X), (S, HW, INV, COL, COL, X), (S, HW, INV, COL, U8, INV)):
        assert img(*args) == bad and b"alias" in l.ppn_last_error(), args
    assert l.ppn_augment_images_color(S, HW, INV, COL, 0, 40, 56, 32, 48, U8, X, None) == bad
    assert l.ppn_augment_images_color(S, HW, INV, COL, 2, 40, 56, 32, 0, U8, X, None) == bad

    P, V, CN, F, M, PO, VO, CO = (0x10000000 * (i + 1) for i in range(8))
    table = lambda t: (C.c_int32 * len(t))(*t)
    good = table(tta_ref.KP_MIRROR)
    ppl = lambda p, kp=good, k=18: l.ppn_augment_people_mirror(p[0], p[1], p[2], p[3], p[4], kp, 3, 8, k, 32, 48, p[5], p[6],
                                                               p[7], None)
    ok = [P, V, CN, F, M, PO, VO, CO]
    for i in (0, 1, 2, 3, 5, 6, 7):                                  # every pointer but `mirror`, which may be NULL
        args = list(ok)
        args[i] = None
        assert ppl(args) == bad and b"NULL" in l.ppn_last_error(), i
    assert ppl(ok, kp=None) == bad and b"NULL" in l.ppn_last_error()
    for args in ([P, V, CN, F, M, P, VO, CO], [P, V, CN, F, M, PO, V, CO], [P, V, CN, F, M, PO, VO, CN],
                 [P, V, CN, F, M, PO, M, CO], [P, V, CN, F, M, PO, VO, M]):
        assert ppl(args) == bad and b"alias" in l.ppn_last_error(), args
    chain = list(tta_ref.KP_MIRROR)
    chain[1], chain[2] = 2, 3                                         # 1 -> 2 -> 3: not an involution
    assert ppl(ok, kp=table(chain)) == bad and b"involution" in l.ppn_last_error()
    assert ppl(ok, kp=table([1, 0] + list(range(2, 18)))) == bad and b"kp_mirror[0]" in l.ppn_last_error()
    assert ppl(ok, kp=table([0, 18] + list(range(2, 18)))) == bad and b"involution" in l.ppn_last_error()
    assert ppl(ok, kp=table([0, -1] + list(range(2, 18)))) == bad
    assert ppl(ok, k=0) == bad and ppl(ok, k=lib.PPN_MAX_KP + 1) == bad
    assert l.ppn_augment_people_mirror(P, V, CN, F, M, good, 0, 8, 18, 32, 48, PO, VO, CO, None) == bad
    # the old entry points are what they were
    assert l.ppn_augment_people(None, V, CN, F, 3, 8, 18, 32, 48, PO, VO, CO, None) == bad
    assert l.ppn_augment_images(None, HW, INV, 2, 40, 56, 32, 48, U8, X, None) == bad


def test_wrappers_take_the_new_arguments():
    import inspect
    A = _aug()
    sig = inspect.signature
    assert sig(A.affine_matrices).parameters["mirror"].default is None
    assert sig(A.sample_params).parameters["mirror_p"].default == 0.0 and sig(A.sample_params).parameters["color"].default is None
    assert sig(A.augment_images).parameters["color"].default is None
    assert sig(A.augment_people).parameters["mirror"].default is None
    assert sig(A.augment_people).parameters["kp_mirror"].default is None
    p = sig(A.TrainAugmenter.__init__).parameters
    assert p["mirror_p"].default == 0.0 and p["color"].default is None
