"""GPU: the decode family (csrc/decode.hip) on the edge cases of tests/decode_cases.py -- tied scores, IoU knife edges,
every (cell, window index) hop, candidate counts on both sides of every threshold, max_humans / min_kp / limit clamps and
the size limits -- at grids other than the workload's 24x24.  Every comparison is exact (np.array_equal) against
oracle.decode_ref; the three homes of the root NMS must also agree with each other bit for bit.

Which dispatch each geometry reaches, derived by hand from launch_limb_argmax (V = 4 iff ncell % 4 == 0 and the head is
16-byte aligned; CS = largest of 3, 2, 1 with ncell % (CS * V) == 0 and ncell / CS >= 64; Q = ncell / CS / V;
NS = min(576 / Q, 32, S); threads = NS * Q rounded up to 64; early NMS iff threads >= ncell and its LDS <= 96 KB) and
from ppn_decode / decode_fused_impl (parse threads = ncell rounded up to 64, nwords = threads / 64; the spread root NMS
of ppn_decode_fused_ws takes images with >= 128 candidates, 8 workgroups each):

    geometry  ncell  S    V  CS  Q    NS  threads  early NMS  parse threads  nwords  spread from
    g11x13    143    77   1  1   143  4   576      on         192            3       128
    g16x16    256    81   4  2   32   18  576      on         256            4       128
    g10x20    200    441  4  2   25   23  576      on         256            4       128
    g26x26    676    25   4  1   169  3   512      off        704            11      128
    g22x32    704    35   4  2   88   6   576      off        704            11      128
    g24x24    576    441  4  3   48   12  576      on         576            9       128

With early NMS off, ppn_decode's root NMS runs in the parse kernel.  ppn_decode_fused (no workspace) always uses the parse
kernel's own NMS; ppn_decode_fused_ws uses root_mask_kernel + the parse kernel's greedy resolve from 128 candidates up.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_cases as DC
from oracle import decode_ref as D
from pytorch_pose_proposal_network_amd import synth

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3                                      # PPN_E_UNSUPPORTED (include/ppn.h)
SENT_I, SENT_F = -77, -123.0
FIELDS = ("kp_cell", "limb_arg", "bbox", "score")

# Largest n ppn_nms accepts, from nms_lds_bytes(n) <= 160 KB = 163840 with nwords = ceil(n / 64) = 16 for n in 961..1024
# and r16 = round up to 16:  r16(16 n) + r16(8 n) + r16(8 n * 16) + 3 r16(4 n) + 16
#   n = 998: 15968 + 7984 + 127744 + 3 * 4000 + 16 = 163712  (accepted)
#   n = 999: 15984 + 8000 + 127872 + 3 * 4000 + 16 = 163872  (refused)
NMS_MAX_N = 998
# Largest decodable grid, from parse_lds_bytes(ncell, K = 18, E = 17) <= 163840 with nwords = ceil(ncell / 64):
#   first = max(r16(16 n) + r16(8 n) + r16(8 n nwords), r16(72 n));  total = first + 3 r16(4 n) + r16(36 n) + 2 r16(34 n) + 272
#   n = 704 (nwords 11): 11264 + 5632 + 61952 = 78848;  + 8448 + 25344 + 47872 + 272 = 160784  (accepted)
#   n = 705 (nwords 12): 11280 + 5648 + 67680 = 84608;  + 8496 + 25392 + 47968 + 272 = 166736  (refused)
# 22 x 32 = 704 cells is a largest grid; every grid of more than 704 cells is refused.
MAX_CELLS = 704


def _dec():
    from pytorch_pose_proposal_network_amd import decode
    return decode


def _decoder(name, batch, nms_thr=0.3, det_thr=0.15, min_kp=1, max_humans=None):
    g = DC.geom(name)
    return _dec().Decoder(batch, (g.H, g.W), g.insize_hw, g.local_grid, det_thr, nms_thr, min_kp, max_humans)


def _fill(o):
    """Sentinels in the output buffers: an entry point that writes nothing cannot pass on its predecessor's results."""
    o.count.fill_(SENT_I); o.kp_cell.fill_(SENT_I); o.limb_arg.fill_(SENT_I)
    o.bbox.fill_(SENT_F); o.score.fill_(SENT_F)


def _args(d):
    o = d.out
    return (o.count.data_ptr(), o.kp_cell.data_ptr(), o.limb_arg.data_ptr(), o.bbox.data_ptr(), o.score.data_ptr())


def _rc_decode(d, head):
    from pytorch_pose_proposal_network_amd import lib as L
    return d.lib.ppn_decode(C.byref(d.cfg), head.data_ptr(), d.batch, d.workspace.data_ptr(), *_args(d), L.current_stream_ptr())


def _rc_fused(d, unary, keys):
    from pytorch_pose_proposal_network_amd import lib as L
    return d.lib.ppn_decode_fused(C.byref(d.cfg), unary.data_ptr(), keys.data_ptr(), d.batch, *_args(d), L.current_stream_ptr())


def _rc_fused_ws(d, unary, keys):
    from pytorch_pose_proposal_network_amd import lib as L
    return d.lib.ppn_decode_fused_ws(C.byref(d.cfg), unary.data_ptr(), keys.data_ptr(), d.batch, d._fused_ws.data_ptr(),
                                     *_args(d), L.current_stream_ptr())


def _run_all(d, heads_t):
    """{entry point: (count i32 [B], per-image dicts)} of the three homes of the root NMS on the same heads."""
    from pytorch_pose_proposal_network_amd import lib as L
    unary, keys = DC.unary_and_keys(heads_t)
    out = {}
    for name, call in (("ppn_decode", lambda: _rc_decode(d, heads_t)), ("ppn_decode_fused", lambda: _rc_fused(d, unary, keys)),
                       ("ppn_decode_fused_ws", lambda: _rc_fused_ws(d, unary, keys))):
        _fill(d.out)
        L.check(call(), name)
        out[name] = (d.out.count.cpu().numpy().copy(), d.out.to_host())
    return out


def _assert_same(res, exp, tag):
    assert res["n"] == int(exp["n"]), (tag, res["n"], int(exp["n"]))
    for k in ("root_cell",) + FIELDS:
        assert np.array_equal(res[k], exp[k]), (tag, k)


def _check_all(got, exp, tag):
    for ep, (cnt, res) in got.items():
        assert cnt.tolist() == [r["n"] for r in exp], (tag, ep)
        for i, r in enumerate(exp):
            _assert_same(res[i], r, (tag, ep, i))
    first = got["ppn_decode"]
    for ep in ("ppn_decode_fused", "ppn_decode_fused_ws"):
        assert np.array_equal(first[0], got[ep][0])
        for a, b in zip(first[1], got[ep][1]):
            for k in FIELDS:
                assert a[k].tobytes() == b[k].tobytes(), (tag, ep, k)


CASES = [(n, v, t) for n in DC.GEOMS for v in DC.VARIANTS for t in (DC.IOU_THRS if v == "iou_edge" else (0.5,))]


@pytest.mark.parametrize("name,variant,thr", CASES, ids=[f"{n}-{v}" + (f"-{t}" if v == "iou_edge" else "") for n, v, t in CASES])
def test_case_through_all_three_root_nms_homes(name, variant, thr):
    """Every (geometry, variant) batch through ppn_decode, ppn_decode_fused and ppn_decode_fused_ws: each equals the
    oracle, the three equal each other, and the arg-max launch equals the dense NumPy arg-max.  The iou_edge image
    built for one threshold is decoded at both."""
    g = DC.geom(name)
    heads = DC.build(name, variant, thr)
    heads_t = torch.from_numpy(heads).cuda()
    nms_thrs = DC.IOU_THRS if variant == "iou_edge" else (0.3,)
    for nms_thr in nms_thrs:
        d = _decoder(name, len(heads), nms_thr=nms_thr)
        if variant == "iou_edge":
            exp = [D.decode_ref(h, nms_thr=nms_thr, insize=g.insize, local_grid=g.local_grid) for h in heads]
            if nms_thr == thr:
                sel = set(exp[0]["cand"][exp[0]["selected"]].tolist())
                for kind, suppress, a, b in DC.iou_edge_pairs(name, thr):
                    assert a in sel and ((b in sel) != suppress), kind
        else:
            exp = DC.expected(name, variant)
        _check_all(_run_all(d, heads_t), exp, (name, variant, nms_thr))
    am = d.limb_argmax(heads_t).cpu().numpy()
    for i in range(len(heads)):
        assert np.array_equal(am[i], D.limb_argmax_dense(heads[i], g.local_grid)), i


@pytest.mark.parametrize("variant", ["ties", "hops", "counts"])
def test_unaligned_head_takes_the_scalar_argmax(variant):
    """11 x 13 once more with the head 4 bytes into a larger allocation: V = 1 through the alignment test as well as
    through ncell % 4 (ppn_decode and ppn_limb_argmax read the head; the fused entry points never see it)."""
    from pytorch_pose_proposal_network_amd import lib as L
    name = "g11x13"
    g = DC.geom(name)
    heads = DC.build(name, variant)
    big = torch.empty(heads.size + 8, dtype=torch.float32, device="cuda")
    skip = (16 - big.data_ptr() % 16) // 4 % 4 + 1                # first element 4 bytes past a 16-byte boundary
    view = big[skip:skip + heads.size].view(heads.shape)
    view.copy_(torch.from_numpy(heads))
    assert view.data_ptr() % 16 == 4
    d = _decoder(name, len(heads))
    _fill(d.out)
    L.check(_rc_decode(d, view), "ppn_decode")
    res = d.out.to_host()
    for i, r in enumerate(DC.expected(name, variant)):
        _assert_same(res[i], r, (variant, i))
    am = d.limb_argmax(view).cpu().numpy()
    for i in range(len(heads)):
        assert np.array_equal(am[i], D.limb_argmax_dense(heads[i], g.local_grid)), i


def _max_humans_sources():
    crowd = np.stack([synth.planted_crowd_head(7 + i) for i in range(3)])
    yield "crowd24", dict(out_hw=(24, 24), insize_hw=(384, 384), local_grid=(21, 21)), crowd, [D.decode_ref(h) for h in crowd]
    g = DC.geom("g11x13")
    yield ("ties11x13", dict(out_hw=(g.H, g.W), insize_hw=g.insize_hw, local_grid=g.local_grid), DC.build("g11x13", "ties"),
           DC.expected("g11x13", "ties"))


@pytest.mark.parametrize("source", ["crowd24", "ties11x13"])
def test_max_humans_clamp_leaves_later_rows_alone(source):
    """max_humans below, at and above the number of people kept, batch 3: count is the unclamped oracle count, the first
    min(count, max_humans) rows are the oracle's first rows, and EVERY later row of every image still holds its
    sentinel (a row written past the clamp would land in the next image's rows).  All three entry points; to_host() and
    HostStage.unpack() return the clamped lists."""
    from pytorch_pose_proposal_network_amd import lib as L
    dec = _dec()
    tag, kw, heads, exp = next(s for s in _max_humans_sources() if s[0] == source)
    heads_t = torch.from_numpy(np.ascontiguousarray(heads)).cuda()
    unary, keys = DC.unary_and_keys(heads_t)
    kept = exp[0]["n"]
    assert kept >= 3 and len({r["n"] for r in exp}) > 1              # the images differ: both sides of the clamp at once
    for mh in (1, 2, kept - 1, kept, kept + 1):
        d = dec.Decoder(3, max_humans=mh, **kw)
        for ep, call in (("ppn_decode", lambda: _rc_decode(d, heads_t)), ("ppn_decode_fused", lambda: _rc_fused(d, unary, keys)),
                         ("ppn_decode_fused_ws", lambda: _rc_fused_ws(d, unary, keys))):
            _fill(d.out)
            L.check(call(), ep)
            o = d.out
            raw = {k: getattr(o, k).cpu().numpy() for k in FIELDS}
            assert o.count.cpu().numpy().tolist() == [r["n"] for r in exp], (mh, ep)
            for b, r in enumerate(exp):
                nout = min(r["n"], mh)
                for k in FIELDS:
                    assert np.array_equal(raw[k][b, :nout], r[k][:nout]), (mh, ep, b, k)
                    sent = SENT_I if raw[k].dtype == np.int32 else np.float32(SENT_F)
                    assert np.all(raw[k][b, nout:] == sent), (mh, ep, b, k, "row past the clamp written")
            host = o.to_host()
            stage = dec.HostStage(3, cap=min(mh, 64))
            o.to_host_async(stage)
            torch.cuda.synchronize()
            for lists in (host, stage.unpack()):
                for b, r in enumerate(exp):
                    nout = min(r["n"], mh)
                    assert lists[b]["n"] == nout, (mh, ep, b)
                    for k in FIELDS:
                        assert np.array_equal(lists[b][k], r[k][:nout]), (mh, ep, b, k)


@pytest.mark.parametrize("det_thr", [0.15, 0.5])
@pytest.mark.parametrize("min_kp", [1, 2, 5, 17, 18])
def test_min_kp_and_det_thr(min_kp, det_thr):
    """min_kp and det_thr other than the defaults, on planted crowds (24 x 24) and on the first hops images of 11 x 13."""
    dec = _dec()
    crowd = np.stack([synth.planted_crowd_head(21 + i) for i in range(2)])
    got = dec.decode_heads(torch.from_numpy(crowd).cuda(), detection_thresh=det_thr, min_num_keypoints=min_kp).to_host()
    total = 0
    for i in range(2):
        exp = D.decode_ref(crowd[i], det_thr=det_thr, min_kp=min_kp)
        _assert_same(got[i], exp, ("crowd", i))
        total += exp["n"]
    assert total > 0 if min_kp <= 2 else total == 0 if min_kp == 18 else True    # 17 limbs: 18 more keypoints never
    name = "g11x13"
    g = DC.geom(name)
    heads = DC.build(name, "hops")[:8]
    exp = [D.decode_ref(h, det_thr=det_thr, min_kp=min_kp, insize=g.insize, local_grid=g.local_grid) for h in heads]
    d = _decoder(name, len(heads), det_thr=det_thr, min_kp=min_kp)
    _check_all(_run_all(d, torch.from_numpy(np.ascontiguousarray(heads)).cuda()), exp, ("hops", min_kp, det_thr))


# ----------------------------------------------------------------------------------------------
# ppn_nms
# ----------------------------------------------------------------------------------------------
def _limits(n):
    return (1, 2, 63, 64, 65, 70, 127, 128, 129, n, n + 5, 0, -1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 500, NMS_MAX_N])
def test_nms_limits_and_ties(n):
    """ppn_nms on the line boxes (the first chunk keeps fewer than 64, later chunks lose boxes to their own and to
    earlier chunks: tests/test_decode_edges_cpu.py) with every score set -- none, distinct, all equal, two values,
    signed zeros mixed with both signs -- and every limit, the ones that are crossed in the middle of a later chunk
    included.  limit <= 0 means none."""
    dec = _dec()
    bb = DC.nms_line_boxes(n)
    for kind in DC.NMS_SCORE_SETS:
        sc = DC.nms_scores(kind, n)
        full = D.nms_ref(bb, 0.3, sc)
        for limit in _limits(n):
            got = dec.non_maximum_suppression(bb, 0.3, sc, limit=limit)
            exp = D.nms_ref(bb, 0.3, sc, limit=limit if limit > 0 else None)
            assert got.dtype == np.int32 and np.array_equal(got, exp), (kind, limit, got[:8], exp[:8])
            assert np.array_equal(exp, full[:limit] if limit > 0 else full)


@pytest.mark.parametrize("name", list(DC.GEOMS))
def test_nms_on_the_tied_and_knife_edge_box_sets(name):
    """The root boxes of the ties images (tied scores: nms_kernel's own sort key against the documented rule) and of the
    iou_edge images (at both thresholds, with and without scores) through the stand-alone ppn_nms."""
    dec = _dec()
    for head in DC.build(name, "ties"):
        bb, sc, _ = DC.root_boxes(name, head)
        assert len(bb) <= NMS_MAX_N
        assert np.array_equal(dec.non_maximum_suppression(bb, 0.3, sc), D.nms_ref(bb, 0.3, sc))
        assert np.array_equal(dec.non_maximum_suppression(bb, 0.3, sc, limit=70), D.nms_ref(bb, 0.3, sc, limit=70))
    for built_for in DC.IOU_THRS:
        bb, sc, _ = DC.root_boxes(name, DC.build(name, "iou_edge", built_for)[0])
        for thr in DC.IOU_THRS:
            with np.errstate(all="ignore"):
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")                   # 0/0 in the oracle: the NaN pairs are the point
                    e1, e2 = D.nms_ref(bb, thr, sc), D.nms_ref(bb, thr)
            assert np.array_equal(dec.non_maximum_suppression(bb, thr, sc), e1), (built_for, thr)
            assert np.array_equal(dec.non_maximum_suppression(bb, thr), e2), (built_for, thr)


# ----------------------------------------------------------------------------------------------
# size limits: host-side refusals (these calls return before any launch)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [NMS_MAX_N + 1, 1024])
def test_nms_refuses_past_its_limit(n):
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    bb = torch.from_numpy(DC.nms_line_boxes(n)).cuda()
    sel = torch.full((n,), SENT_I, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), SENT_I, dtype=torch.int32, device="cuda")
    rc = lib.ppn_nms(bb.data_ptr(), None, n, 0.3, 0, sel.data_ptr(), cnt.data_ptr(), L.current_stream_ptr())
    assert rc == UNSUPPORTED
    assert str(n).encode() in lib.ppn_last_error()
    torch.cuda.synchronize()
    assert int(cnt.item()) == SENT_I and bool((sel == SENT_I).all())


@pytest.mark.parametrize("hw", [(15, 47), (32, 32)])
def test_decode_refuses_grids_past_the_lds_limit(hw):
    """705 cells (one past MAX_CELLS) and 32 x 32: ppn_decode, ppn_decode_fused and ppn_decode_fused_ws refuse with
    PPN_E_UNSUPPORTED and a message before launching anything, and leave the result buffers alone.  ppn_limb_argmax has
    no such limit (its LDS is NS * ncl * 8 bytes): it works on both grids and equals the dense NumPy arg-max."""
    dec = _dec()
    H, W = hw
    assert H * W > MAX_CELLS
    d = dec.Decoder(1, hw, (H * 16, W * 16), (3, 3))
    from pytorch_pose_proposal_network_amd import prng
    head = prng.uniform01(prng.stream_seed(61, H), d.channels * H * W).reshape(1, d.channels, H, W)
    head[:, 108:] = np.floor(head[:, 108:] * 8) / 8                  # ties inside the windows
    head_t = torch.from_numpy(head).cuda()
    unary, keys = DC.unary_and_keys(head_t)
    for ep, call in (("ppn_decode", lambda: _rc_decode(d, head_t)), ("ppn_decode_fused", lambda: _rc_fused(d, unary, keys)),
                     ("ppn_decode_fused_ws", lambda: _rc_fused_ws(d, unary, keys))):
        _fill(d.out)
        assert call() == UNSUPPORTED, ep
        assert str(H * W).encode() in d.lib.ppn_last_error(), ep
        torch.cuda.synchronize()
        o = d.out
        assert bool((o.count == SENT_I).all()) and bool((o.kp_cell == SENT_I).all()) and bool((o.limb_arg == SENT_I).all())
        assert bool((o.bbox == SENT_F).all()) and bool((o.score == SENT_F).all())
    am = d.limb_argmax(head_t).cpu().numpy()
    assert np.array_equal(am[0], D.limb_argmax_dense(head[0], (3, 3)))
