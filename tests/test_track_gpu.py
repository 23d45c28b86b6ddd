"""GPU: ppn_track_update held byte for byte to tests/track_ref.py on the cases of tests/track_cases.py -- outputs, flags and
the whole state after every call -- plus the buffers it must leave alone, resets, graph capture and the rt entry points."""
import os

import numpy as np
import pytest
import torch

import track_cases as TC
import track_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = (7, 300)


def _tracker(case, **kw):
    from pytorch_pose_proposal_network_amd import track
    c = case["cfg"]
    return track.Tracker(case["streams"], case["frames"], case["M"], c["K"], c["iou_thr"], c["kp_gate"], c["min_close"],
                         c["max_age"], c["birth_thr"], c["alpha"], **kw)


def _result(call, M):
    from pytorch_pose_proposal_network_amd import decode
    t = {k: torch.from_numpy(call[k]).cuda() for k in ("count", "kp_cell", "bbox", "score")}
    return decode.DecodeResult(t["count"], t["kp_cell"], None, t["bbox"], t["score"], M)


def _same(got, exp, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    if exp.dtype == np.uint32:
        got = got.view(np.uint32)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    assert got.tobytes() == exp.tobytes(), (what, int((got.view(np.uint32) != exp.view(np.uint32)).sum()), "words differ")


def _people_rows(call, M):
    """Per image the rows p < P."""
    return np.arange(M)[None, :] < np.clip(call["count"], 0, M)[:, None]


def _run(case, tracker=None, want_xy=True):
    """Every call of the case through the kernel; returns what track_cases.run_ref returns."""
    tr = tracker or _tracker(case)
    steps = []
    for c in case["calls"]:
        out = tr.update(_result(c, case["M"]), c["n_frames"], want_xy)
        steps.append((dict(ids=out.ids.cpu().numpy(), hits=out.hits.cpu().numpy(),
                           xy=None if out.xy is None else out.xy.cpu().numpy(), live=out.live.cpu().numpy()),
                      tr.state_to_host()))
    return steps


def _check(name, case):
    """Kernel against restatement after every call.  Both keep one set of output buffers that starts zeroed, so the rows
    of out_xy that a call does not write compare equal too."""
    got, exp = _run(case), TC.run_ref(name, case)
    for i, ((g_out, g_st), (e_out, e_st)) in enumerate(zip(got, exp)):
        for k in ("ids", "hits", "xy", "live"):
            _same(g_out[k], e_out[k], (name, i, k))
        for k in e_st:
            _same(g_st[k], e_st[k], (name, i, "state", k))
    return got, exp


CASES = {
    "drift": TC.drift, "absence1": lambda M: TC.absence(M, 1), "absence2": lambda M: TC.absence(M, 2),
    "absence3": lambda M: TC.absence(M, 3), "close_beats_iou": TC.close_beats_iou, "equal_keys": TC.equal_keys,
    "iou_breaks_ties": TC.iou_breaks_ties, "two_want_one": TC.two_want_one, "freed_slot_reused": TC.freed_slot_reused,
    "smoothing1": lambda M: TC.smoothing(M, 1.0), "smoothing.5": lambda M: TC.smoothing(M, 0.5),
    "birth_threshold": TC.birth_threshold, "k3_age0": lambda M: TC.small_k(M, 0), "k3_age2": lambda M: TC.small_k(M, 2),
    "k32": TC.large_k, "edge_batch": TC.edge_batch,
}


@pytest.mark.parametrize("M", SIZES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_matches_the_restatement(name, M):
    _check(f"{name}/{M}", CASES[name](M))


@pytest.mark.parametrize("M", SIZES)
def test_chunking_invariance(M):
    def run(name, case):
        return _check(name, case)[0]
    TC.assert_chunking_invariant(TC.chunking_views(M, run))


def test_knife_edges():
    case, pts, r2 = TC.gate_sweep()
    got, exp = _check("gate_sweep", case)
    ids = got[0][0]["ids"][1::2, 0]
    assert set(ids.tolist()) == {1, 2}                                      # both sides of the gate occur
    case, boxes = TC.iou_sweep()
    got, exp = _check("iou_sweep", case)
    assert set(got[0][0]["ids"][1::2, 0].tolist()) == {1, 2}


@pytest.mark.parametrize("M", SIZES)
def test_untouched_bytes_and_want_xy(M):
    """Sentinels: every out_id / out_hits entry is overwritten, out_xy rows >= P and the state of idle streams keep their
    bytes; want_xy=False leaves out_xy alone altogether."""
    case = TC.edge_batch(M)
    call, K = case["calls"][0], case["cfg"]["K"]
    for want_xy in (True, False):
        tr = _tracker(case)
        for n, t in tr.state.items():
            t[2].fill_(-7 if t.dtype == torch.int32 else -7.5)              # stream 2 is idle
        before = tr.state_to_host()
        tr.ids.fill_(-99); tr.hits.fill_(-99); tr.live.fill_(-99); tr.xy.fill_(-99.5)
        st = R.copy_state(before)
        out = dict(ids=np.full((15, M), -99, np.int32), hits=np.full((15, M), -99, np.int32),
                   xy=np.full((15, M, K, 2), -99.5, np.float32) if want_xy else None, live=np.full(15, -99, np.int32))
        R.track_update(case["cfg"], st, call["count"], call["kp_cell"], call["bbox"], call["score"], 5, 3,
                       call["n_frames"], out=out)
        res = tr.update(_result(call, M), call["n_frames"], want_xy)
        assert (res.xy is None) == (not want_xy)
        _same(res.ids, out["ids"], "ids"); _same(res.hits, out["hits"], "hits"); _same(res.live, out["live"], "live")
        assert (out["ids"] != -99).all() and (out["hits"] != -99).all() and (out["live"] != -99).all()
        xy = tr.xy.cpu().numpy()
        if want_xy:
            _same(xy, out["xy"], "xy")
            written = _people_rows(call, M) & (np.repeat(call["n_frames"], 3) > np.tile(np.arange(3), 5))[:, None]
            assert (xy[~written] == -99.5).all() and (xy[written] != -99.5).all()
        else:
            assert (xy == -99.5).all()
        after = tr.state_to_host()
        for k in st:
            _same(after[k], st[k], ("state", k))
            assert after[k][2].tobytes() == before[k][2].tobytes(), k       # the idle stream, sentinel bytes and all


def test_reset_and_rerun():
    case = TC.chunking(7, "streams")[0]
    tr = _tracker(case)
    first = _run(case, tr)
    tr.reset()
    assert all(int(t.abs().sum()) == 0 for t in tr.state.values())
    tr.xy.zero_()                          # an output buffer, not state: rows beyond an image's people are never written
    again = _run(case, tr)
    for (o1, s1), (o2, s2) in zip(first, again):
        assert all(o1[k].tobytes() == o2[k].tobytes() for k in o1) and all(s1[k].tobytes() == s2[k].tobytes() for k in s1)
    # a per-stream reset leaves the other streams alone
    before = tr.state_to_host()
    tr.reset(streams=[1])
    after = tr.state_to_host()
    for k in before:
        assert not after[k][1].any(), k
        assert after[k][[0, 2]].tobytes() == before[k][[0, 2]].tobytes(), k
    assert before["id"][1].any() and before["last_id"][1] > 0
    with pytest.raises(ValueError):
        tr.reset(streams=[3])


def test_flags_accumulate_until_cleared():
    case = TC.edge_batch(300)
    tr = _tracker(case)
    _run(case, tr)
    assert tr.flags().tolist() == [2, 3, 0, 0, 0]
    tr.clear_flags()
    assert tr.flags().tolist() == [0] * 5


def test_to_host():
    case = TC.edge_batch(7)
    tr = _tracker(case)
    call = case["calls"][0]
    rows = tr.update(_result(call, 7), call["n_frames"]).to_host()
    (out, st), = TC.run_ref("edge_batch/7", case)
    assert len(rows) == 15
    for b, r in enumerate(rows):
        n = int(np.clip(call["count"][b], 0, 7)) if out["live"][b] >= 0 else 0
        assert r["live"] == out["live"][b] and r["ids"].shape == (n,)
        _same(r["ids"], out["ids"][b, :n], b); _same(r["hits"], out["hits"][b, :n], b); _same(r["xy"], out["xy"][b, :n], b)


def test_shape_dtype_and_device_checks():
    case = TC.drift(7)
    tr = _tracker(case)
    good = _result(case["calls"][0], 7)
    from pytorch_pose_proposal_network_amd import decode
    for field, bad in (("count", good.count.long()), ("kp_cell", good.kp_cell[:, :, :17]), ("bbox", good.bbox.cpu()),
                       ("score", good.score.transpose(1, 2))):
        kw = dict(count=good.count, kp_cell=good.kp_cell, limb_arg=None, bbox=good.bbox, score=good.score, max_humans=7)
        kw[field] = bad
        with pytest.raises(ValueError):
            tr.update(decode.DecodeResult(**kw))
    with pytest.raises(ValueError):
        tr.update(decode.DecodeResult(good.count, good.kp_cell, None, good.bbox, good.score, 8))
    with pytest.raises(ValueError):
        tr.update(good, n_frames=[1, 1])
    assert not any(int(t.abs().sum()) for t in tr.state.values())           # nothing ran


def test_graph_capture_replays_to_the_same_bytes():
    case = TC.chunking(7, "streams")[0]
    eager = _run(case)
    tr = _tracker(case)
    staged = _result(case["calls"][0], 7)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = _tracker(case)
        warm.update(staged)                                                 # the module is loaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        tr.update(staged)
    tr.reset()                                                              # whatever the capture did not run
    for i, c in enumerate(case["calls"]):
        for k in ("count", "kp_cell", "bbox", "score"):
            getattr(staged, k).copy_(torch.from_numpy(c[k]))
        g.replay()
        torch.cuda.synchronize()
        out, st = eager[i]
        _same(tr.ids, out["ids"], i); _same(tr.hits, out["hits"], i); _same(tr.xy, out["xy"], i); _same(tr.live, out["live"], i)
        now = tr.state_to_host()
        for k in st:
            _same(now[k], st[k], (i, k))


# ---- network level: D-22, float32, 96 x 96 ------------------------------------------------------------------------------
def test_rt_entry_points():
    from pytorch_pose_proposal_network_amd import drn, model, prng, rt, synth, track
    g = np.load(os.path.join(GOLDEN, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    m = model.PoseProposalNet(drn.drn_d_22(), insize=(96, 96), outsize=(6, 6), compute_dtype="float32").cuda()
    m.load_state_dict(synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats))
    m.eval()
    one = torch.from_numpy(prng.u8_frames(515, 1, (96, 96))).cuda()
    frames = one.expand(4, -1, -1, -1).contiguous()
    res = rt.inference_batch(frames, m)
    n = int(res.count[0])
    assert 0 < n <= 36 and res.count.tolist() == [n] * 4
    manual = track.Tracker(1, 4, 36)
    exp = manual.update(res)
    exp = [t.clone() for t in (exp.ids, exp.hits, exp.xy, exp.live)]
    tr = track.Tracker(1, 4, 36)
    res2, got = rt.inference_batch_tracked(frames, m, tr)
    assert torch.equal(res2.count, res.count) and torch.equal(res2.bbox[:, :n], res.bbox[:, :n])    # rows of people only
    for a, b in zip((got.ids, got.hits, got.xy, got.live), exp):
        assert torch.equal(a, b)
    roots = int((res.kp_cell[0, :n, 0] >= 0).sum())
    assert roots == n                                                       # the decode lists people by their root
    ids, hits = got.ids.cpu().numpy(), got.hits.cpu().numpy()
    for t in range(4):
        assert ids[t, :n].tolist() == list(range(1, n + 1)) and (ids[t, n:] == -1).all()
        assert hits[t, :n].tolist() == [t + 1] * n
    assert got.live.tolist() == [n] * 4 and tr.flags().tolist() == [0]

    single = track.Tracker(1, 1, 36)
    for t in range(2):
        humans, scores, pid = rt.inference_tracked(one[0], m, (6, 6), (21, 21), single)
        assert len(humans) == len(scores) == n and pid == list(range(1, n + 1))
    assert single.hits[0, :n].tolist() == [2] * n
