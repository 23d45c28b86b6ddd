"""The cases of tests/backward_cases.py are what they claim (CPU only), and their f64 reference is right: every table entry
meets the preconditions that make tests/test_backward_edges_gpu.py reach the path it is for, the autograd reference equals
the two sums written out tap by tap, and the oracle of the off-square training iteration has its grid the right way round."""
import numpy as np
import pytest
import torch

import backward_cases as BC


def test_reference_equals_the_sums_written_out_per_tap():
    """F.conv2d + .backward in f64 against an explicit loop over taps and output pixels: off-square, strided, dilated, a
    remainder on one axis ((H + 2 pad - eff) % s == 1 for H, 0 for W), batch > 1, cin != cout."""
    c = BC.Conv(2, 3, 5, 10, 7, 3, 2, 2, 1)
    assert (c.H + 2 * c.pad - BC.eff(c)) % c.s == 1 and (c.W + 2 * c.pad - BC.eff(c)) % c.s == 0
    Ho, Wo = BC.out_hw(c)
    assert (Ho, Wo) == (4, 3)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(c.B, c.H, c.W, c.ci, generator=g, dtype=torch.float64)
    w = torch.randn(c.co, c.ci, c.k, c.k, generator=g, dtype=torch.float64)
    dy = torch.randn(c.B, Ho, Wo, c.co, generator=g, dtype=torch.float64)
    dW, _ = BC.grads_ref(c, dy, x=x)
    _, dX = BC.grads_ref(c, dy, w=w)
    dW2, dX2 = BC.conv_grads_by_taps(c, x.numpy(), w.numpy(), dy.numpy())
    assert np.abs(dW.numpy() - dW2).max() <= 1e-13 * np.abs(dW2).max()
    assert np.abs(dX.numpy() - dX2).max() <= 1e-13 * np.abs(dX2).max()
    assert np.abs(dW2).min() > 0                     # every tap meets the image somewhere
    # the pixels no output reads are the ones with a zero gradient, and there are some (stride 2 and dilation 2 from an
    # odd offset: every even row and column)
    t = BC.touched(c)
    assert not t[0::2].any() and not t[:, 0::2].any() and t[1::2, 1::2].all()
    assert ((dX2 != 0).any(axis=(0, 3)) == t).all()


@pytest.mark.parametrize("name,dtype", BC.wgrad_runs())
def test_wgrad_cases_meet_their_preconditions(name, dtype):
    c, why = BC.WGRAD_CASES[name]
    Ho, Wo = BC.out_hw(c)
    assert c.H != c.W and Ho != Wo and Ho % 2 == 1 and Wo % 2 == 1 and Ho >= 1 and Wo >= 1
    nsplit = BC.partials(c, dtype)
    assert BC.check_wgrad_purpose(name, dtype, nsplit) is None
    if why[dtype] in ("split23", "tail"):
        assert c.ci == c.co == 64 or BC.wgrad_tile(c) == 256
    if name.startswith("big"):
        assert BC.wgrad_tile(c) == 256
    if name == "big3x3d2":
        assert c.dil == 2 and c.ci % 256 and c.co % 256                      # ragged channel tiles
    if name.startswith("s2/"):
        rem = ((c.H + 2 * c.pad - c.k) % 2, (c.W + 2 * c.pad - c.k) % 2)
        assert c.s == 2 and sorted(rem) == [0, 1] and (c.H % 2 or c.W % 2)
    if name == "wo1":
        assert Wo == 1 and Ho > 1
    if name == "ho1":
        assert Ho == 1 and Wo > 1
    assert BC.pixels(c) < 1 << 24


def test_wgrad_cases_cover_the_list():
    runs = BC.wgrad_runs()
    kinds = {(BC.WGRAD_CASES[n][1][d], d) for n, d in runs}
    for d in ("f32", "bf16"):
        assert ("split23", d) in kinds and ("tail", d) in kinds
    assert ("ldscap", "bf16") in kinds
    # idle work-groups behind the XCD remap, in both dtypes and on both tiles
    idle = [(n, d) for n, d in runs if n in BC.WGRAD_IDLE and BC.WGRAD_CASES[n][1][d] != "any"]
    assert {d for _, d in idle} == {"f32", "bf16"} and {BC.wgrad_tile(BC.WGRAD_CASES[n][0]) for n, _ in idle} == {128, 256}
    for n, d in idle:
        assert BC.wgrad_items(BC.WGRAD_CASES[n][0], BC.partials(BC.WGRAD_CASES[n][0], d)) % 8
    # strided 3x3 and strided 1x1, the remainder once on each axis
    s2 = [BC.WGRAD_CASES[n][0] for n in BC.WGRAD_CASES if n.startswith("s2/")]
    assert {c.k for c in s2} == {1, 3}
    assert {(c.H + 2 * c.pad - c.k) % 2 for c in s2} == {0, 1}


@pytest.mark.parametrize("name", list(BC.STEM_CASES))
def test_stem_cases_meet_their_preconditions(name):
    c = BC.STEM_CASES[name]
    Ho, Wo = BC.out_hw(c)
    tiles, cap = BC.stem_tiles(c), BC.stem_cap(c)
    assert c.H != c.W and Ho != Wo and Ho % BC.stem_rows(c) and Wo % 64
    grid = BC.partials(c, "bf16")
    if name.endswith("/persistent"):
        assert cap < tiles < 2 * cap and grid == cap
    else:
        assert tiles < cap and grid == tiles and c.H > c.W and tiles > 1
    # these shapes are the ones the dedicated kernels take (anything else would be the generic kernel with pixel splits)
    assert (c.k, c.s, c.ci, c.co) in {(7, 1, 8, 16), (7, 1, 4, 16), (3, 1, 16, 16), (3, 2, 16, 32)} and c.dil == 1 and c.pad == c.k // 2


def test_stem_cases_cover_every_kernel_in_both_orientations():
    kinds = {(n.split("/")[1], c.k, c.s, c.ci) for n, c in BC.STEM_CASES.items()}
    assert kinds == {(v, k, s, ci) for v in ("persistent", "small") for (k, s, ci) in ((7, 1, 8), (7, 1, 4), (3, 1, 16), (3, 2, 16))}
    assert {BC.stem_cap(c) for c in BC.STEM_CASES.values()} == {512, 1024}
    assert BC.stem_rows(BC.STEM_CASES["l2/small"]) == 4 and BC.stem_rows(BC.STEM_CASES["l1/small"]) == 8


@pytest.mark.parametrize("name", list(BC.DGRAD_CASES))
def test_dgrad_cases_meet_their_preconditions(name):
    c = BC.DGRAD_CASES[name]
    Ho, Wo = BC.out_hw(c)
    assert c.H != c.W and Ho >= 1 and Wo >= 1
    assert c.ci % 8 == 0 and c.co % 8 == 0             # what the convolution kernels accept in both dtypes
    t = BC.touched(c)
    if c.s == 2:
        rem = ((c.H + 2 * c.pad - c.k) % 2, (c.W + 2 * c.pad - c.k) % 2)
        assert sorted(rem) == [0, 1]
        # the zero-upsampled dy is larger than stride * (Ho - 1) + 1 on the axis with the remainder
        up = (c.H + 2 * c.pad - c.k + 1, c.W + 2 * c.pad - c.k + 1)
        assert [u != 2 * (o - 1) + 1 for u, o in zip(up, (Ho, Wo))] == [r == 1 for r in rem]
        if c.pad == 0:
            assert not t.all() and (not t[-1].any() or not t[:, -1].any())
    else:
        assert t.all()
    if name.startswith("big/"):
        assert min(c.ci, c.co) >= 256 and c.dil == 2
    if name == "ragged/d4":
        assert c.ci % 64 and c.co % 64 and c.dil == 4
    if name == "w1":
        assert c.W == 1 and c.k == 3 and c.pad == 1


def test_dgrad_cases_cover_the_stride2_paths():
    s2 = [BC.DGRAD_CASES[n] for n in BC.DGRAD_S2]
    for k in (1, 3):
        assert any(c.k == k and c.ci <= 16 and c.pad == k // 2 for c in s2)
        assert any(c.k == k and c.ci > 16 and c.pad == k // 2 for c in s2)
    # the remainder sits on H in one case and on W in another
    assert {(c.H + 2 * c.pad - c.k) % 2 for c in s2} == {0, 1}
    # rows / columns without any gradient exist in the 1x1 cases (every odd one) and in the pad-0 case (the last row)
    for n in ("s2/1x1/ci64", "s2/1x1/ci8", "s2/3x3/pad0"):
        assert not BC.touched(BC.DGRAD_CASES[n]).all()


def test_training_case_and_its_oracle_are_oriented_rows_by_columns():
    from oracle import forward_ref as Fr
    from oracle import loss_ref as Lr
    sd, x, tg = BC.train_inputs()
    assert (BC.TRAIN_H, BC.TRAIN_W) == (112, 80) and BC.TRAIN_INSIZE == (80, 112) and BC.TRAIN_OUTSIZE == (5, 7)
    assert BC.TRAIN_H % 16 == 0 and BC.TRAIN_W % 16 == 0
    assert x.shape == (BC.TRAIN_BATCH, 3, 112, 80)
    head = Fr.forward_ref(sd, x, BC.TRAIN_ARCH)
    assert tuple(head.shape) == (BC.TRAIN_BATCH, 6 * Lr.K + 441 * Lr.E, 7, 5)
    assert tg["delta"].shape == (BC.TRAIN_BATCH, Lr.K, 7, 5) and tg["te"].shape[-2:] == (7, 5)
    # there is something to learn from in both images, and not only in a square corner of the grid
    on = tg["delta"].sum(axis=1) > 0
    assert on.reshape(BC.TRAIN_BATCH, -1).any(axis=1).all() and on[:, 5:].any()
