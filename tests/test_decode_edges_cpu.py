"""The decode edge cases of tests/decode_cases.py are what they claim (CPU only, oracle.decode_ref alone): tied scores are
bit-equal, the IoU pairs sit exactly on / one float below the threshold, the candidate counts and the hop coverage are
as listed, every image decodes to people, and the `ties` cases can tell the documented tie rule from its reverse --
otherwise tests/test_decode_edges_gpu.py would pass vacuously."""
import numpy as np
import pytest

import decode_cases as DC
from oracle import decode_ref as D

GEOMS = list(DC.GEOMS)


@pytest.mark.parametrize("name", GEOMS)
def test_ties_are_bit_equal_and_decide_the_survivors(name):
    g = DC.geom(name)
    heads = DC.build(name, "ties")
    for i, head in enumerate(heads):
        bbox, score, cells = DC.root_boxes(name, head)
        vals, mult = np.unique(score.view(np.uint32), return_counts=True)
        assert len(vals) <= 3 and mult.min() > 1, (i, vals, mult)            # a handful of values, each of them tied
        assert set(vals.view(np.float32).tolist()) <= {1.0, 0.75, 0.5}
        kept = D.nms_ref(bbox, 0.3, score)
        assert 0 < len(kept) < len(cells)                                    # some suppress each other, some do not
        rev = DC.nms_ref_reversed_ties(bbox, 0.3, score)
        assert set(kept.tolist()) != set(rev.tolist()), (i, "the reversed tie rule keeps the same boxes")
    _, score, cells = DC.root_boxes(name, heads[1])
    assert len(cells) == g.ncell and np.all(score.view(np.uint32) == np.float32(1.0).view(np.uint32))


@pytest.mark.parametrize("thr", DC.IOU_THRS)
@pytest.mark.parametrize("name", GEOMS)
def test_iou_edge_pairs_sit_on_the_threshold(name, thr):
    head = DC.build(name, "iou_edge", thr)[0]
    bbox, score, cells = DC.root_boxes(name, head)
    pairs = DC.iou_edge_pairs(name, thr)
    assert sorted(cells.tolist()) == sorted(c for _, _, a, b in pairs for c in (a, b))
    pos = {int(c): k for k, c in enumerate(cells)}
    t32 = np.float32(thr)
    assert float(t32) == thr
    below = float(t32) - float(np.nextafter(t32, np.float32(0)))
    full = set(cells[D.nms_ref(bbox, thr, score)].tolist())
    for kind, suppress, a, b in pairs:
        two = np.stack([bbox[pos[a]], bbox[pos[b]]])
        m = {}
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sel = D.nms_ref(two, thr, np.asarray([1.0, 0.5], np.float32), margins=m)
        assert len(sel) == (1 if suppress else 2), kind
        if kind.startswith("equal"):
            assert m["iou"] == 0.0, (kind, m)                                 # iou == thr exactly
        elif kind.startswith("below"):
            assert m["iou"] == below, (kind, m, below)                        # iou == nextafter(thr, 0)
        elif kind in ("touch", "zero_inside"):
            assert m["iou"] == thr, (kind, m)                                 # iou == 0
        else:
            assert "iou" not in m, (kind, m)                                  # 0/0: NaN, never a finite margin
            area = (two[:, 2] - two[:, 0]) * (two[:, 3] - two[:, 1])
            assert np.all(area == 0)
        # ... and the pairs do not disturb each other inside the image
        assert a in full and ((b in full) != suppress), kind


@pytest.mark.parametrize("name", GEOMS)
def test_candidate_counts(name):
    exp = DC.expected(name, "counts")
    want = DC.ladder(name)
    assert [len(r["cand"]) for r in exp] == want
    g = DC.geom(name)
    assert {0, 1, 127, 128, 129, g.ncell - 1, g.ncell} <= set(want)          # both sides of the spread threshold


@pytest.mark.parametrize("name", GEOMS)
def test_hops_cover_what_they_promise(name):
    g = DC.geom(name)
    images = DC.hops_images(name)
    heads = DC.build(name, "hops")
    exp = DC.expected(name, "hops")
    s_all = np.stack([DC.hop_s(g, i) for i in images])                       # [images, cell]
    for k, i in enumerate(images):
        dense = D.limb_argmax_dense(heads[k], g.local_grid)
        for e in (0, 5, E_LAST):
            assert np.array_equal(dense[e].reshape(-1), DC.hop_s(g, i, e)), (i, e)
    if name in DC.FULL_HOPS:
        assert len(images) == g.S
        assert np.array_equal(np.sort(s_all, axis=0), np.tile(np.arange(g.S)[:, None], (1, g.ncell)))
    else:
        assert set(s_all.reshape(-1).tolist()) == set(range(g.S))            # every window row and column
    # every cell is a root and nothing is suppressed; edge 0 is evaluated for every human; hops land on and off the grid,
    # on targets exactly at the threshold (accepted), one float below (rejected) and well above
    kind = DC.hop_kind(g)
    seen = set()
    for k, r in enumerate(exp):
        assert len(r["selected"]) == g.ncell and r["n"] >= 1
        roots = r["kp_cell"][:, 0]
        assert np.array_equal(r["limb_arg"][:, 0], s_all[k][roots])
        u = r["limb_arg"][:, 0]
        jh, jw = roots // g.W + u // g.sW - g.sH // 2, roots % g.W + u % g.sW - g.sW // 2
        on = (jh >= 0) & (jw >= 0) & (jh < g.H) & (jw < g.W)
        tgt = np.where(on, jh * g.W + jw, 0)
        got = r["kp_cell"][:, DC.HOP_DST]
        assert np.all(got[~on] == -1)
        assert np.array_equal(got[on] >= 0, kind[tgt[on]] != 1)
        assert np.array_equal(got[on][got[on] >= 0], tgt[on][got[on] >= 0])
        seen |= {("off",)} if (~on).any() else set()
        seen |= {("on", int(v)) for v in np.unique(kind[tgt[on]])}
    assert seen == {("off",), ("on", 0), ("on", 1), ("on", 2)}


E_LAST = D.E - 1


@pytest.mark.parametrize("variant", DC.VARIANTS)
@pytest.mark.parametrize("name", GEOMS)
def test_every_nonempty_image_decodes_to_people(name, variant):
    for thr in (DC.IOU_THRS if variant == "iou_edge" else (0.5,)):
        for i, r in enumerate(DC.expected(name, variant, thr)):
            assert (r["n"] >= 1) == (len(r["cand"]) >= 1), (thr, i)


def test_nms_line_boxes_reach_the_limit_trimming():
    """The stand-alone NMS sets: the first 64-chunk keeps fewer than 64, so a limit of 70 is crossed in the middle of the
    second chunk, some of whose boxes are suppressed by boxes the first chunk kept."""
    bb = DC.nms_line_boxes(200)
    full = D.nms_ref(bb, 0.3)
    first = int((full < 64).sum())
    assert first < 64 < 70 < int((full < 128).sum())
    second_dropped = sorted(set(range(64, 128)) - set(full.tolist()))
    own = {i for i in second_dropped if i % 4 == 1}
    assert own and set(second_dropped) - own                                 # by its own chunk, and by an earlier one
    for i in set(second_dropped) - own:
        two = np.stack([bb[i - 64], bb[i]])
        assert len(D.nms_ref(two, 0.3)) == 1 and (i - 64) in full.tolist()
    assert np.array_equal(D.nms_ref(bb, 0.3, limit=70), full[:70])
    z = DC.nms_scores("zeros", 10)
    assert np.array_equal(np.signbit(z[:4]), [False, True, False, True]) and np.all(z[:4] == 0)


def _r16(x):
    return (x + 15) // 16 * 16


def _nms_lds_bytes(n):
    """csrc/decode.hip nms_lds_bytes, restated."""
    nwords = (n + 63) // 64
    return _r16(16 * n) + _r16(8 * n) + _r16(8 * n * nwords) + 3 * _r16(4 * n) + 16


def _parse_lds_bytes(ncell, K=D.K, E=D.E, max_edges=32):
    """csrc/decode.hip parse_lds_bytes, restated."""
    nwords = (ncell + 63) // 64
    first = max(_r16(16 * ncell) + _r16(8 * ncell) + _r16(8 * ncell * nwords), _r16(4 * K * ncell))
    return first + 3 * _r16(4 * ncell) + _r16(2 * ncell * K) + 2 * _r16(2 * ncell * E) + _r16(4 * (36 + max_edges))


def test_size_limits_follow_from_the_lds_formulas_and_match_the_header():
    """ppn_nms and the decode refuse what needs more than 160 KB of LDS: n <= 998 and H*W <= 704 (22 x 32 is a largest
    grid).  include/ppn.h states both."""
    import os
    lds = 160 * 1024
    assert max(n for n in range(1, 1025) if _nms_lds_bytes(n) <= lds) == 998
    assert _nms_lds_bytes(998) == 163712 and _nms_lds_bytes(999) == 163872
    assert max(n for n in range(1, 1025) if _parse_lds_bytes(n) <= lds) == 704 == DC.geom("g22x32").ncell
    assert _parse_lds_bytes(704) == 160784 and _parse_lds_bytes(705) == 166736
    assert all(_nms_lds_bytes(n) < _nms_lds_bytes(n + 1) and _parse_lds_bytes(n) < _parse_lds_bytes(n + 1) for n in range(1, 1024))
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ppn.h")).read()
    assert "n <= 998" in hdr and "n <= 1024" not in hdr
    assert "H*W <= 704" in hdr
