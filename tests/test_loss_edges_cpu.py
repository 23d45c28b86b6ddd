"""The edge cases of tests/loss_cases.py are what they claim (CPU only): the oracle is finite on all of them in f32 and in
f64, the ties / touching / disjoint boxes hold exactly in both precisions, and the perfectly fitted case really cancels the
IoU gradient with respect to w and h -- which is what makes tests/test_loss_edges_gpu.py sensitive to the tie rule."""
import numpy as np
import pytest
import torch

import loss_cases as LC

K = LC.K


def _group_max(a, C):
    return {g: float(np.abs(a[:, sl]).max()) for g, sl in LC.group_slices(C)}


@pytest.mark.parametrize("name", LC.CASES)
def test_oracle_is_finite_in_both_precisions(name):
    r = LC.first_order(name, "mix")
    assert np.isfinite(r["l64"]).all() and np.isfinite(r["l32"]).all(), (r["l64"], r["l32"])
    assert np.isfinite(r["g64"]).all() and r["finite32"]
    assert all(np.isfinite(v) for v in r["e32"].values())
    assert r["g64"].shape == LC.build(name)[0].shape
    # the f32 oracle agrees with the f64 one to f32 accuracy: e32 is rounding, not a second answer
    for g, m in _group_max(r["g64"], r["g64"].shape[1]).items():
        assert r["e32"][g] <= 1e-5 * max(m, 1.0) or r["e32"][g] <= 2e-2 * m, (g, r["e32"][g], m)


@pytest.mark.parametrize("name", ["g35/plain", "g35/sat", "g35/fit", "g35/edge_ties", "g35/zero_area", "g60/fit",
                                  "g60/edge_ties", "g60/zero_area", "g30s/sat"])
def test_double_backward_is_finite_in_both_precisions(name):
    for ckey in ("mix", "unary"):
        r = LC.second_order(name, ckey)
        assert np.isfinite(r["zbar64"]).all() and np.isfinite(r["tzbar64"]).all()
        assert all(np.isfinite(v) for v in list(r["e32_zbar"].values()) + list(r["e32_tzbar"].values()))


def test_geometries_reach_what_they_are_for():
    hw = {g: o[0] * o[1] for g, (_, o, _) in LC.GEOMS.items()}
    assert hw["g35"] % 4 and hw["g135"] % 4                                     # the scalar limb kernels
    assert hw["g60"] % 4 == 0 and LC.GEOMS["g60"][1][0] % 4                     # vector loss on scalar-encoded targets
    assert hw["g140"] % 4 == 0 and hw["g140"] % 64 and hw["g140"] > 128         # vector path, ragged third block
    assert hw["g135"] > 128 and hw["g135"] % 64
    (inW, inH), (W, H), _ = LC.GEOMS["g30s"]
    assert inW // W != inH // H
    for g, (insize, outsize, win) in LC.GEOMS.items():
        assert insize[0] % outsize[0] == 0 and insize[1] % outsize[1] == 0 and win[0] == win[1] and outsize[0] != outsize[1]
    assert LC.channels(LC.GEOMS["g35"][2]) == 533 and LC.channels(LC.GEOMS["g135"][2]) == 7605
    assert (5 * K * hw["g35"]) % 256 != 0 and -(-5 * K * hw["g35"] // 256) == 13    # batch 5: 3150 threads over 13 blocks


@pytest.mark.parametrize("geom", ["g35", "g60"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sat_and_zero_area_inputs(geom, dtype):
    head = LC.build(f"{geom}/sat")[0]
    assert set(np.unique(head)) == {0.0, 1.0}
    head, tg = LC.build(f"{geom}/zero_area")[:2]
    on = tg["delta"] > 0
    for g in (4, 5):
        assert (head[:, g * K:(g + 1) * K][on] == 0).all()
    assert (tg["tw"][on] == 0).all() and (tg["th"][on] == 0).all()
    e = LC.iou_edges(f"{geom}/zero_area", dtype)
    ont = torch.from_numpy(on)
    assert (e["wr"][ont] <= 0).all() and (e["hr"][ont] <= 0).all()              # I = 0 and both areas 0: U = eps


@pytest.mark.parametrize("geom", ["g35", "g60"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_fit_is_a_four_way_tie(geom, dtype):
    name = f"{geom}/fit"
    head, tg = LC.build(name)[:2]
    on = tg["delta"] > 0
    for g, key in ((2, "tx"), (3, "ty"), (4, "tw"), (5, "th")):
        assert np.array_equal(head[:, g * K:(g + 1) * K][on], tg[key][on])
    e = LC.iou_edges(name, dtype)
    ont = torch.from_numpy(on)
    for p, q in (("a1", "c1"), ("b1", "d1"), ("a2", "c2"), ("b2", "d2")):
        assert torch.equal(e[p][ont], e[q][ont]), (p, q)
    assert (e["wr"][ont] > 0).all() and (e["hr"][ont] > 0).all()


@pytest.mark.parametrize("geom", ["g35", "g60"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_edge_ties_hold_exactly(geom, dtype):
    name = f"{geom}/edge_ties"
    head, tg, insize, outsize, _ = LC.build(name)
    e = LC.iou_edges(name, dtype)
    pairs = (("a1", "c1"), ("b1", "d1"), ("a2", "c2"), ("b2", "d2"))
    for i, (rel, (ix, iy), (tx, ty, tw, th), _) in enumerate(LC.TIE_CELLS):
        assert tg["delta"][0, 0, iy, ix] == 1.0
        assert (tg["tx"][0, 0, iy, ix], tg["ty"][0, 0, iy, ix], tg["tw"][0, 0, iy, ix], tg["th"][0, 0, iy, ix]) == \
            (tx / 64, ty / 64, tw / 64, th / 64), rel
        assert tuple(head[0, g * K, iy, ix] for g in (2, 3, 4, 5)) == LC.tie_prediction(i, outsize)
        v = {k: float(t[0, 0, iy, ix]) for k, t in e.items()}
        equal = {f"{p}=={q}" for p, q in pairs if v[p] == v[q]}
        if "==" in rel and rel != "wr==0":                                     # exactly the named pair of edges, no other
            assert equal == {rel}, (rel, equal, v)
            assert v["wr"] > 0 and v["hr"] > 0
        elif rel == "wr==0":                                                   # the ReLU kink: touching, not overlapping
            assert v["wr"] == 0.0 and v["hr"] > 0 and not equal, (rel, v, equal)
            assert v["b1"] == v["c1"]
        else:
            assert v["wr"] < 0 and v["hr"] > 0 and not equal, (rel, v, equal)
    # every edge value of the six cells is the same number in f32 and f64
    if dtype == torch.float32:
        e64 = LC.iou_edges(name, torch.float64)
        for _, (ix, iy), _, _ in LC.TIE_CELLS:
            for k in e:
                assert float(e[k][0, 0, iy, ix]) == float(e64[k][0, 0, iy, ix]), k


@pytest.mark.parametrize("geom", ["g35", "g60"])
def test_fit_cancels_the_size_gradient(geom):
    """At a fitted cell the IoU gradient w.r.t. w and h is g_iou * rh * (eps / 2) / U^2 under the half-gradient tie rule and
    of order g_iou * rh / A * inW under any other: the w / h groups of `fit` are >= 100x smaller than `plain`'s."""
    C = LC.build(f"{geom}/fit")[0].shape[1]
    for ckey in ("mix", "e1"):
        fit = _group_max(LC.first_order(f"{geom}/fit", ckey)["g64"], C)
        plain = _group_max(LC.first_order(f"{geom}/plain", ckey)["g64"], C)
        for g in ("w", "h"):
            assert fit[g] * 100 <= plain[g], (ckey, g, fit[g], plain[g])
    # the same for the double-backward quantity: tzbar = (d loss / ds) s (1 - s)
    fit = _group_max(LC.second_order(f"{geom}/fit", "mix")["tzbar64"], C)
    plain = _group_max(LC.second_order(f"{geom}/plain", "mix")["tzbar64"], C)
    for g in ("w", "h"):
        assert fit[g] * 100 <= plain[g], (g, fit[g], plain[g])


def test_e32_is_per_case_and_group():
    r = LC.first_order("g35/plain", "mix")
    assert set(r["e32"]) == set(LC.GROUPS) == set(r["e32_dz"]) == set(r["e32_db"])
    assert LC.first_order("g35/plain", "mix") is r                             # computed once, shared
    assert not r["g64"].flags.writeable
    assert LC.tol(1.0, 0.0) == 2e-5 and LC.tol(0.0, 1e-6) == 4e-6
