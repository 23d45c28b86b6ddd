"""CPU: the head arg-max cases (tests/head_cases.py) are what they claim and their checker sees the faults it is for.  No GPU.

* every case reaches the branch it is recorded for: the slot split pq / pr, tail rows, tiles per workgroup, empty slots and images
  per tile, computed by head_cases.schedule() (the tile walk of conv_head.hip restated) for the 256 compute units of an MI355X;
* the exact cases meet the exactness condition in every type and are arranged as the module says (ties, saturation, no logit
  in 14 .. 19);
* the reference alone leaves at most 1 % of the windows of every random case undecided;
* a torch f32 emulation (f32 logits, f32 sigmoid, first maximum of the values) passes the checker at ratio <= 1 on every case;
* planted faults are all caught."""
import numpy as np
import pytest
import torch

import head_cases as HC

DT = HC.DTYPE_NAMES
N_CU = 256
RANDOM = [n for n, c in HC.CASES.items() if c.kind in ("random", "negative")]
EXACT = [n for n, c in HC.CASES.items() if c.kind in ("ties", "saturated")]


def _sched(name, n_cu=N_CU):
    c = HC.CASES[name]
    return HC.schedule(HC.pixels(c), c.E, n_cu)


def test_cases_reach_the_branches_they_are_for():
    want = {"slots/9_exact": (9, 1, 1, 0), "slots/9_tail": (9, 1, 1, 59), "slots/23": (23, 2, 7, 64), "slots/7": (7, 0, 7, 114),
            "slots/1_partial": (1, 0, 1, 63), "walk17": (41, 5, 1, 64)}
    for name, (n_ptiles, pq, pr, tail) in want.items():
        s = _sched(name)
        assert (s["n_ptiles"], s["pq"], s["pr"], s["tail"]) == (n_ptiles, pq, pr, tail), (name, s)
    assert HC.pixels(HC.CASES["slots/9_exact"]) == 1152 and HC.pixels(HC.CASES["slots/9_tail"]) == 19 * 19 * 3
    # mixed slots (pq >= 1 and pr >= 1): slots below pr divide by pq + 1, the rest by pq; the grid is cut to the largest slot, so
    # the workgroups of the smaller slots past their tiles return at once
    for name in ("slots/9_exact", "slots/9_tail", "slots/7"):
        assert _sched(name)["empty"] > 0, name
    # the walk: >= 3 tiles per workgroup with an edge change at every step, on 256 compute units and on 64
    for n_cu in (256, 64):
        s = _sched("walk17", n_cu)
        assert s["max_tiles"] >= 3 and s["edge_changes"] >= 2, s
    c = HC.CASES["walk17"]
    assert (c.E, HC.pixels(c), c.K) == (17, 5184, 128)
    # windows: every listed one, both paddings, two pixel tiles with a 7-row second one
    for w in HC.EDGE_WINDOWS + HC.SMALL_WINDOWS:
        h, p = HC.CASES["win%d/hostile" % w], HC.CASES["win%d/production" % w]
        assert (h.win, h.pad, h.kind, p.win, p.pad, p.kind) == (w, "hostile", "random", w, "zero", "negative")
        assert _sched("win%d/hostile" % w)["n_ptiles"] == 2 and _sched("win%d/hostile" % w)["tail"] == 7
    assert HC.EDGE_WINDOWS == (385, 420, 431, 432, 433, 441, 447, 448)
    # pixel ranges: disjoint, their union the whole tensor, every inner cut off the multiples of 128
    for name in ("ranges/2", "ranges/3", "ranges/3_of4"):
        c = HC.CASES[name]
        end = 0
        for lo, n in c.ranges:
            assert lo == end and n > 0
            end = lo + n
            assert end == HC.pixels(c) or end % HC.BP != 0
            if (c.H * c.W) % 4 == 0:
                assert lo % 4 == 0 and (end % 4 == 0 or end == HC.pixels(c))
        assert end == HC.pixels(c)
    assert (HC.CASES["ranges/3_of4"].H * HC.CASES["ranges/3_of4"].W) % 4 == 0 and (19 * 19) % 4 != 0
    assert len(HC.CASES["ranges/2"].ranges) == 2 and len(HC.CASES["ranges/3"].ranges) == 3
    # depth: two and four K steps in every type, and 512
    assert [HC.depth(HC.CASES["depth/2steps"], d) for d in DT] == [64, 128, 128]
    assert [HC.depth(HC.CASES["depth/4steps"], d) for d in DT] == [128, 256, 256]
    assert [HC.depth(HC.CASES["depth/512"], d) for d in DT] == [512, 512, 512]
    assert HC.ODD_DEPTH_STEPS % 2 == 1
    # small images
    c = HC.CASES["howo6"]
    assert c.H * c.W == 6 and HC.BP // 6 == 21 and HC.pixels(c) > HC.BP
    c = HC.CASES["howo1"]
    assert c.H * c.W == 1 and HC.pixels(c) > HC.BP
    assert HC.CASES["null_bias"].bias is False and HC.operands("null_bias", "f32")[2] is None
    # the atomic path: a window wider than a 448-row tile, one that a 32-channel run crosses twice, the three unary counts
    a = {n: c for n, c in HC.CASES.items() if "atomic" in c.paths}
    assert {81, 420, 441, 529, 20} <= {c.win for c in a.values()}
    assert {0, 108, 64} <= {c.uch for c in a.values()} and 64 % 32 == 0
    assert HC.CASES["atomic/win20"].win + 2 <= 32 and HC.CASES["atomic/win529"].win > HC.EDGE_PAD
    assert set(HC.ATOMIC_TILES) == {None, (192, 128), (256, 256)}


@pytest.mark.parametrize("name", EXACT)
def test_exact_cases_are_exact_and_arranged_as_stated(name):
    c = HC.CASES[name]
    amb = list(HC.AMBIGUOUS[name])
    M = HC.pixels(c)
    if c.paths[0] == "edge":
        # tile 0 holds exactly one ambiguous pixel; tile 1's are its last valid rows before the tail
        assert sum(1 for m in amb if m < HC.BP) == 1 and [m for m in amb if m >= HC.BP] == [M - 2, M - 1] and M % HC.BP != 0
    for d in DT:
        x, w, b = HC.operands(name, d)
        assert HC.exact_condition(x, w, b)
        assert float(x.abs().max()) <= 2 and float(w.abs().max()) <= 40 and torch.equal(HC.q(w, d), w)
        ref = HC.reference_of(c, x, w, b)
        t = ref.t
        assert not bool(((t > 13.0) & (t < 20.0)).any())                     # nothing near the band 14 .. 19
        flag0 = torch.zeros(M, dtype=torch.bool)
        flag0[amb] = True
        i1, i2, i3 = HC.tie_rows(c)
        assert 0 <= i1 < i2 < i3 == c.win - 1
        want, bits = HC.expected_exact(c, ref)
        if c.kind == "ties":
            three = t[:, :, [i1, i2, i3]]
            rest = t.clone()
            rest[:, :, [i1, i2, i3]] = float("-inf")
            assert bool((three.max(dim=2).values - rest.max(dim=2).values >= 2.0).all())
            assert bool((three[flag0][:, :, 0] == three[flag0][:, :, 1]).all() and (three[flag0][:, :, 0] == three[flag0][:, :, 2]).all())
            assert bool((want[flag0] == i1).all()) and bool((want[~flag0] == i2).all()) and bits is None
            assert bool((three[~flag0][:, :, 1] - three[~flag0][:, :, [0, 2]].max(dim=2).values == 1.0).all())
        else:
            sat = t >= 20.0
            assert bool((t[~sat] <= 10.0).all())
            assert bool((sat.sum(dim=2)[flag0] == 3).all()) and bool((sat.sum(dim=2)[~flag0] == 2).all())
            assert bool((want[flag0] == i1).all()) and bool((want[~flag0] == i2).all())
            # the lowest saturated index is NOT the largest logit where the flag is 1: an arg-max of the logits would be wrong
            assert bool((ref.first[~flag0] != i2).any())
            assert np.float32(1.0) + np.exp(np.float32(-20.0)) == np.float32(1.0) and int(bits[0, 0]) == 0x3F800000


@pytest.mark.parametrize("name", RANDOM)
def test_reference_leaves_at_most_one_percent_undecided(name):
    c = HC.CASES[name]
    for d in DT:
        ref = HC.reference(name, d)
        share = 1.0 - float(ref.decided.double().mean())
        print("HEAD_EDGE_CPU %s %s: undecided by the reference alone %.4f, max |logit| %.1f" % (name, d, share, float(ref.t.abs().max())))
        assert share <= HC.UNDECIDED_CAP, (name, d, share)
        assert float(ref.t.abs().max()) <= 40.0                               # e^-v neither overflows nor goes subnormal
        if c.kind == "negative":                                              # every limb score below 0.5: a zero pad row would win
            assert float(ref.tmax.max()) < -1.0


@pytest.mark.parametrize("name", list(HC.CASES))
def test_f32_emulation_passes_the_checker(name):
    c = HC.CASES[name]
    for d in DT:
        x, w, b = HC.operands(name, d)
        ref = HC.reference(name, d)
        keys = HC.emulate(c, x, w, b)
        v = HC.check(c, ref, keys)
        assert v.ok and v.ratio <= 1.0, (name, d, v)
        if c.kind in ("ties", "saturated"):
            assert HC.check_exact(c, ref, keys) is None
        val, idx = HC.split_keys(keys)
        assert torch.equal(HC.make_keys(val, idx, c), keys)


# ---- planted faults ---------------------------------------------------------------------------------------------------------------

def _pad_rows_compete(name, d):
    """conv_head.hip masks the rows past the window in the last 16-row channel tile only: the pad rows window .. 431 of a
    window below 432 are not masked.  model.py packs them with zero weights and bias, so their value is sigmoid(0) = 0.5."""
    c = HC.CASES[name]
    x, w, b = HC.operands(name, d)
    n = HC.EDGE_PAD - 16 - c.win
    assert n > 0
    return HC.emulate(c, x, w, b, win_rows=lambda v: torch.cat([v, torch.full(v.shape[:2] + (n,), 0.5)], dim=2))


def _bias_row_of_the_wrong_edge(name, d):
    c = HC.CASES[name]
    x, w, b = HC.operands(name, d)
    b2 = b.clone()
    b2[c.uch:] = torch.roll(b[c.uch:].view(c.E, c.win), 1, dims=0).reshape(-1)
    return HC.emulate(c, x, w, b2)


def _last_index_wins_a_tie(name, d):
    c = HC.CASES[name]
    x, w, b = HC.operands(name, d)
    val, idx = HC.split_keys(HC.emulate(c, x, w, b, win_rows=lambda v: v.flip(2)))
    return HC.make_keys(val, c.win - 1 - idx, c)


def _pixel_tile_of_the_neighbouring_slot(name, d):
    """Pixel tile 1 (slot 0 owns tiles 0 and 1 of the nine) computed from the rows of tile 2, the first of slot 1."""
    c = HC.CASES[name]
    x, w, b = HC.operands(name, d)
    X = x.permute(0, 2, 3, 1).reshape(HC.pixels(c), -1).clone()
    X[HC.BP: 2 * HC.BP] = X[2 * HC.BP: 3 * HC.BP]
    return HC.emulate(c, X.view(c.B, c.H, c.W, -1).permute(0, 3, 1, 2), w, b)


def _key_one_pixel_off(name, d):
    c = HC.CASES[name]
    val, idx = HC.split_keys(HC.emulate(c, *HC.operands(name, d)))
    return HC.make_keys(torch.roll(val, 1, dims=0), torch.roll(idx, 1, dims=0), c)


FAULTS = {
    "pad rows compete (window 420, production padding)": ("win420/production", _pad_rows_compete),
    "pad rows compete (window 385, production padding)": ("win385/production", _pad_rows_compete),
    "the bias row of the wrong edge": ("win441/hostile", _bias_row_of_the_wrong_edge),
    "a pixel tile taken from the neighbouring slot": ("slots/9_tail", _pixel_tile_of_the_neighbouring_slot),
    "a key written one pixel off": ("slots/9_tail", _key_one_pixel_off),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_checker_sees_the_planted_fault(fault):
    name, plant = FAULTS[fault]
    c = HC.CASES[name]
    for d in DT:
        ref = HC.reference(name, d)
        clean = HC.check(c, ref, HC.emulate(c, *HC.operands(name, d)))
        v = HC.check(c, ref, plant(name, d))
        print("HEAD_EDGE_CPU fault '%s' %s: indices out of range %d, not near-maximal %d, decided windows wrong %d, ratio %.3g"
              % (fault, d, v.bad_index, v.not_near, v.wrong_decided, v.ratio))
        assert clean.ok and not v.ok, (fault, d, v)
        if plant is _pad_rows_compete:
            # every cell: all real limb scores are below 0.5, the key is 0.5 at an index past the window
            assert v.bad_index == HC.pixels(c) * c.E
        elif plant is not _bias_row_of_the_wrong_edge:                      # (a bias of scale 0.1 moves the value, rarely the index)
            assert v.wrong_decided > 0


def test_pad_rows_that_compete_hide_behind_positive_maxima():
    """Why no test noticed: with the biases as drawn, the maximum of a window's ~400 random logits is almost never negative, and a
    zero pad row (value 0.5) never wins."""
    c = HC.CASES["win420/hostile"]
    x, w, b = HC.operands("win420/hostile", "bf16")
    keys = HC.emulate(c, x, w, b, win_rows=lambda v: torch.cat([v, torch.full(v.shape[:2] + (12,), 0.5)], dim=2))
    assert HC.check(c, HC.reference("win420/hostile", "bf16"), keys).ok


@pytest.mark.parametrize("name", ["ties", "atomic/ties"])
def test_last_index_winning_a_tie_is_caught_by_the_exact_check(name):
    c = HC.CASES[name]
    for d in DT:
        ref = HC.reference(name, d)
        keys = _last_index_wins_a_tie(name, d)
        why = HC.check_exact(c, ref, keys)
        assert why is not None and "wanted index %d" % HC.tie_rows(c)[0] in why
        # the near-maximal rule alone cannot see it: the tied logits are equal
        assert HC.check(c, ref, keys).ok
        assert HC.check_exact(c, ref, HC.emulate(c, *HC.operands(name, d))) is None


def test_saturated_lowest_index_rule_is_caught_by_the_exact_check():
    """An arg-max of the LOGITS picks the largest saturated logit, not the lowest saturated index."""
    c = HC.CASES["saturated"]
    for d in DT:
        ref = HC.reference("saturated", d)
        keys = HC.make_keys(torch.ones(ref.first.shape), ref.first, c)
        assert HC.check_exact(c, ref, keys) is not None
        keys = HC.make_keys(torch.full(ref.first.shape, float(np.nextafter(np.float32(1.0), np.float32(0.0)))),
                            HC.expected_exact(c, ref)[0], c)
        assert HC.check_exact(c, ref, keys) is not None                       # one f32 step below 1.0f


def test_a_value_one_f32_step_beyond_the_bound_is_caught():
    name = "win441/hostile"
    c = HC.CASES[name]
    for d in DT:
        ref = HC.reference(name, d)
        val, idx = HC.split_keys(HC.emulate(c, *HC.operands(name, d)))
        for (m, e, sign) in ((0, 0, 1.0), (HC.pixels(c) - 1, c.E - 1, -1.0)):
            k = int(idx[m, e])
            t, A = ref.t[m, e, k], ref.A[m, e, k]
            edge = float(HC.sigmoid64(t) + sign * HC.value_bound(t, A))
            inside = np.float32(edge)
            if (float(inside) - edge) * sign > 0:                           # rounded outwards: step back in
                inside = np.nextafter(inside, np.float32(0.5 * (1 - sign)))
            outside = np.nextafter(inside, np.float32(0.5 * (1 + sign)))
            for step, ok in ((inside, True), (outside, False)):
                v2 = val.clone()
                v2[m, e] = float(step)
                got = HC.check(c, ref, HC.make_keys(v2, idx, c))
                assert got.ok == ok and (got.ratio <= 1.0) == ok, (d, m, e, float(step), got)
