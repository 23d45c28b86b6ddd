"""GPU: ppn_zone_update held byte for byte to tests/zones_ref.py on the cases of tests/zones_cases.py -- every output and the
whole state after every call -- plus the bytes it must leave alone, resets, graph capture and the rt entry point."""
import os

import numpy as np
import pytest
import torch

import zones_cases as ZC
import zones_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = (7, 300)
ANCHOR = {R.ANCHOR_CENTER: "center", R.ANCHOR_BOTTOM: "bottom"}
OUTS = ("slot", "inside", "zone", "line")


def _upload_tables(z, geom):
    """The case's tables as they are (the clamping cases hold what set_zones would reject)."""
    for k, v in geom.items():
        z.geom[k].copy_(torch.from_numpy(v))


def _zones(case, raw=False, **kw):
    """A Zones with the case's geometry: through set_zones / set_lines, or the raw tables."""
    from pytorch_pose_proposal_network_amd import zones
    c, g = case["cfg"], case["geom"]
    z = zones.Zones(case["streams"], case["frames"], case["M"], c["K"], c["max_gap"], ANCHOR[c["anchor"]], c["loiter"], **kw)
    if raw:
        _upload_tables(z, g)
        return z
    for s in range(case["streams"]):
        z.set_zones(s, [g["zone_xy"][s, i, :g["zone_nv"][s, i]] for i in range(g["zone_n"][s])])
        z.set_lines(s, [g["line_xy"][s, l] for l in range(g["line_n"][s])])
    for k, v in g.items():                                          # what the setters uploaded is the restatement's table
        assert z.geom[k].cpu().numpy().tobytes() == v.tobytes(), k
    return z


def _inputs(call, M):
    """(DecodeResult, TrackResult) of a call, on the device."""
    from pytorch_pose_proposal_network_amd import decode, track
    t = {k: torch.from_numpy(call[k]).cuda() for k in ("count", "kp_cell", "bbox", "ids")}
    xy = None if call["xy"] is None else torch.from_numpy(call["xy"]).cuda()
    return (decode.DecodeResult(t["count"], t["kp_cell"], None, t["bbox"], None, M),
            track.TrackResult(t["ids"], None, xy, None, t["count"]))


def _same(got, exp, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    if exp.dtype == np.uint32:
        got = got.view(np.uint32)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    assert got.tobytes() == exp.tobytes(), (what, int((got.view(np.uint32) != exp.view(np.uint32)).sum()), "words differ")


def _outputs(res):
    return {k: getattr(res, k).cpu().numpy() for k in OUTS}


def _run(case, z=None, raw=False):
    """Every call of the case through the kernel; returns what zones_cases.run_ref returns."""
    z = z or _zones(case, raw)
    return ZC.run_case(case, lambda c: _outputs(z.update(*_inputs(c, case["M"]), c["n_frames"])), z.state_to_host)


def _compare(got, exp, name):
    for i, ((g_out, g_st), (e_out, e_st)) in enumerate(zip(got, exp)):
        for k in OUTS:
            _same(g_out[k], e_out[k], (name, i, k))
        for k in e_st:
            _same(g_st[k], e_st[k], (name, i, "state", k))


def _check(name, case, raw=False):
    got, exp = _run(case, raw=raw), ZC.run_ref(name, case)
    assert len(got) == len(exp) == len(case["calls"])
    _compare(got, exp, name)
    return got


@pytest.mark.parametrize("nl", (0, 1, 16))
@pytest.mark.parametrize("nz", (1, 16))
@pytest.mark.parametrize("K", (1, 18))
@pytest.mark.parametrize("M", SIZES)
def test_kernel_matches_the_restatement(M, K, nz, nl):
    """A random-walk crowd with a fixed seed, 8 calls of one frame on three streams, one of them busy, two idle: one zone
    (a triangle) and 16 (3 to 8 vertices), 0, 1 and 16 lines; the anchor and xy alternate with the shape."""
    anchor = R.ANCHOR_BOTTOM if (nz == 16) == (K == 18) else R.ANCHOR_CENTER
    case = ZC.geometry(M, K, nz, nl, anchor, with_xy=nl != 1)
    got = _check(f"geometry/{M}/{K}/{nz}/{nl}", case)
    st = got[-1][1]
    assert not st["id"][1:].any() and not st["zone_total"][1:].any() and st["flags"].tolist() == [0, 0, 0]     # idle streams
    assert st["zone_total"][0, :nz].any() and not st["zone_total"][0, nz:].any() and not st["line_total"][0, nl:].any()
    if nz == 16:
        assert st["zone_total"][0, :, 1].any() and any(o["zone"][0, :, 3].any() for o, _ in got)   # exits; loitering
    if nl == 16:
        assert st["line_total"][0, :, 0].any() and st["line_total"][0, :, 1].any()


@pytest.mark.parametrize("anchor", (R.ANCHOR_CENTER, R.ANCHOR_BOTTOM))
@pytest.mark.parametrize("with_xy", (True, False))
@pytest.mark.parametrize("M", SIZES)
def test_frames_in_one_call(M, with_xy, anchor):
    """Three frames per call, ragged n_frames, counts below 0 and above M (at M = 300 the latter overflows the 64 slots), xy
    given and NULL, both anchors; K = 3, four zones and four lines per stream."""
    case = ZC.frames3(M, anchor=anchor, with_xy=with_xy)
    got = _check(f"frames3/{M}/{with_xy}/{anchor}", case)
    assert got[-1][1]["flags"].tolist() == [0, 1 if M == 300 else 0, 0]
    slot, zone = got[0][0]["slot"], got[0][0]["zone"]
    assert (slot[3:] == -1).all() and (slot[1] == -1).all() and not zone[3:].any() and not zone[1, :, :2].any()   # idle; a count < 0
    if M == 300:
        assert (got[1][0]["slot"][3] >= 0).sum() == 64 and got[1][0]["zone"][3, :4, 0].sum() > 64


@pytest.mark.parametrize("name", sorted(ZC.scenarios()))
def test_hand_checked_scenarios(name):
    """The cases whose outcome tests/test_zones_cpu.py asserts by hand, through the kernel."""
    _check("scenario/" + name, ZC.scenarios()[name])


@pytest.mark.parametrize("with_xy", (True, False))
@pytest.mark.parametrize("anchor", (R.ANCHOR_CENTER, R.ANCHOR_BOTTOM))
def test_polygon_knife_edges(anchor, with_xy):
    (out, st), = _check(f"knife/{anchor}/{with_xy}", ZC.knife_edges(with_xy, anchor))
    for z, name in enumerate(("square", "square", "diamond", "u", "u", "collinear")):
        got = {pt for p, pt in enumerate(ZC.KNIFE_POINTS) if out["inside"][0, p] >> z & 1}
        assert got == ZC.KNIFE_INSIDE[name], (z, name)


@pytest.mark.parametrize("with_xy", (True, False))
def test_people_that_take_no_part(with_xy):
    got = _check(f"bystanders/{with_xy}", ZC.bystanders(with_xy))
    assert got[0][0]["slot"][0].tolist() == [-1] * 5 + [0, -1, -1] and got[2][1]["id"][0, :4].tolist() == [14, 15, 16, 0]


def test_tables_are_clamped_not_trusted():
    _check("clamped", ZC.clamped(), raw=True)


@pytest.mark.parametrize("M", SIZES)
def test_chunking_invariance(M):
    ZC.assert_chunking_invariant(ZC.chunking_views(M, _check))


@pytest.mark.parametrize("M", SIZES)
def test_untouched_bytes(M):
    """Canaries.  Every output lies inside a larger buffer of sentinel bytes: every byte of the output is overwritten (also
    for the images that are not processed), none next to it.  Every geometry table lies between NaN floats and huge counts: an
    entry read from beside a table would change the result.  An idle stream's state, sentinel bytes and all, is untouched."""
    case = ZC.frames3(M)
    z = _zones(case)
    pad = 64
    bufs = {}
    for k in OUTS:
        own = getattr(z, k)
        buf = torch.full((own.numel() + 2 * pad,), -99, dtype=torch.int32, device="cuda")
        bufs[k] = buf
        setattr(z, k, buf[pad:pad + own.numel()].view(own.shape))
    from pytorch_pose_proposal_network_amd import lib
    tables = {}
    for k, own in z.geom.items():
        fill = float("nan") if own.dtype == torch.float32 else 2 ** 30
        buf = torch.full((own.numel() + 2 * pad,), fill, dtype=own.dtype, device="cuda")
        buf[pad:pad + own.numel()] = own.reshape(-1)
        tables[k] = buf
        z.geom[k] = buf[pad:pad + own.numel()].view(own.shape)
    z._geom = lib.ZoneGeom(*(z.geom[n].data_ptr() for n, _ in lib.ZoneGeom._fields_))
    for t in z.state.values():
        t[1].fill_(-7 if t.dtype == torch.int32 else -7.5)          # stream 1 is idle in the first call
    before = z.state_to_host()
    st = R.copy_state(before)
    c = case["calls"][0]
    exp = R.zone_update(case["cfg"], case["geom"], st, c["count"], c["kp_cell"], c["bbox"], c["ids"], c["xy"], 3, 3, c["n_frames"],
                        out={k: np.full(v.shape, -99, np.int32).view(v.dtype) for k, v in R.fresh_outputs(9, M).items()})
    res = z.update(*_inputs(c, M), c["n_frames"])
    for k in OUTS:
        _same(getattr(res, k), exp[k], k)
        assert (exp[k].view(np.int32) != -99).all()                 # the restatement, too, wrote every entry
        assert (bufs[k][:pad] == -99).all() and (bufs[k][-pad:] == -99).all(), k
    after = z.state_to_host()
    for k in st:
        _same(after[k], st[k], ("state", k))
        assert after[k][1].tobytes() == before[k][1].tobytes(), k   # the idle stream, sentinel bytes and all


def test_reset_and_rerun():
    case = ZC.chunking(7, "mixed")[0]
    z = _zones(case)
    first = _run(case, z)
    z.reset()
    assert all(int(t.abs().sum()) == 0 for t in z.state.values()) and z.geom["zone_n"].tolist() == [5, 5, 5]
    _compare(_run(case, z), first, "rerun")
    zt, lt = z.totals()
    assert zt.tobytes() == first[-1][1]["zone_total"].tobytes() and lt.tobytes() == first[-1][1]["line_total"].tobytes()
    # a per-stream reset leaves the other streams alone
    before = z.state_to_host()
    z.reset(streams=[1])
    after = z.state_to_host()
    for k in before:
        assert not after[k][1].any(), k
        assert after[k][[0, 2]].tobytes() == before[k][[0, 2]].tobytes(), k
    assert before["id"][1].any() and before["zone_total"][1].any() and before["last"][1].any()
    with pytest.raises(ValueError):
        z.reset(streams=[3])


def test_flags_accumulate_until_cleared():
    case = ZC.frames3(300)
    z = _zones(case)
    calls = case["calls"]
    z.update(*_inputs(calls[0], 300), calls[0]["n_frames"])
    assert z.flags().tolist() == [0, 0, 0]
    z.update(*_inputs(calls[1], 300), calls[1]["n_frames"])
    assert z.flags().tolist() == [0, 1, 0]
    z.update(*_inputs(calls[2], 300), calls[2]["n_frames"])          # no overflow in this call: the flag stays
    assert z.flags().tolist() == [0, 1, 0]
    z.clear_flags()
    assert z.flags().tolist() == [0, 0, 0]


def test_shape_dtype_and_device_checks():
    from pytorch_pose_proposal_network_amd import decode, track
    case = ZC.geometry(7, 3, 1, 1)
    z = _zones(case)
    good, tracks = _inputs(case["calls"][0], 7)
    for field, bad in (("count", good.count.long()), ("kp_cell", good.kp_cell[:, :, :2]), ("bbox", good.bbox.cpu()),
                       ("bbox", good.bbox.transpose(1, 2))):
        kw = dict(count=good.count, kp_cell=good.kp_cell, limb_arg=None, bbox=good.bbox, score=None, max_humans=7)
        kw[field] = bad
        with pytest.raises(ValueError):
            z.update(decode.DecodeResult(**kw), tracks)
    with pytest.raises(ValueError):
        z.update(decode.DecodeResult(good.count, good.kp_cell, None, good.bbox, None, 8), tracks)
    for ids, xy in ((tracks.ids.long(), tracks.xy), (tracks.ids[:, :6], tracks.xy), (tracks.ids.cpu(), tracks.xy),
                    (tracks.ids, tracks.xy.double()), (tracks.ids, tracks.xy[..., :1]), (tracks.ids, tracks.xy.cpu())):
        with pytest.raises(ValueError):
            z.update(good, track.TrackResult(ids, None, xy, None, good.count))
    with pytest.raises(ValueError):
        z.update(good, tracks, n_frames=[1, 1])
    assert not any(int(t.abs().sum()) for t in z.state.values()) and (z.slot == -1).all()           # nothing ran
    z.update(good, track.TrackResult(tracks.ids, None, tracks.xy.cpu(), None, good.count), smoothed=False)   # xy is not looked at
    assert z.state["id"][0].any()


def test_graph_capture_replays_to_the_same_bytes():
    """One captured update, replayed on new inputs call after call: the state is carried over from replay to replay."""
    case = ZC.chunking(7, "mixed")[0]
    eager = _run(case)
    z = _zones(case)
    staged, tracks = _inputs(case["calls"][0], 7)
    nf = torch.zeros(3, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm = _zones(case)
        warm.update(staged, tracks, nf)                                     # the module is loaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        z.update(staged, tracks, nf)
    z.reset()                                                               # whatever the capture did not run
    for i, c in enumerate(case["calls"]):
        for k in ("count", "kp_cell", "bbox"):
            getattr(staged, k).copy_(torch.from_numpy(c[k]))
        tracks.ids.copy_(torch.from_numpy(c["ids"])); tracks.xy.copy_(torch.from_numpy(c["xy"]))
        nf.copy_(torch.from_numpy(c["n_frames"]))
        g.replay()
        torch.cuda.synchronize()
        out, st = eager[i]
        for k in OUTS:
            _same(getattr(z, k), out[k], (i, k))
        now = z.state_to_host()
        for k in st:
            _same(now[k], st[k], (i, k))
    assert eager[-1][1]["zone_total"].any() and eager[-1][1]["line_total"].any()


# ---- network level: D-22, float32, 96 x 96 ------------------------------------------------------------------------------
def test_rt_entry_point():
    from pytorch_pose_proposal_network_amd import drn, model, prng, rt, synth, track, zones
    g = np.load(os.path.join(GOLDEN, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    m = model.PoseProposalNet(drn.drn_d_22(), insize=(96, 96), outsize=(6, 6), compute_dtype="float32").cuda()
    m.load_state_dict(synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats))
    m.eval()
    one = torch.from_numpy(prng.u8_frames(515, 1, (96, 96))).cuda()
    frames = one.expand(4, -1, -1, -1).contiguous()
    res, tracks = rt.inference_batch_tracked(frames, m, track.Tracker(1, 4, 36))
    n = int(res.count[0])
    assert 0 < n <= 36 and res.count.tolist() == [n] * 4

    def make():
        z = zones.Zones(1, 4, 36, loiter=3)
        z.set_zones(0, [[(0, 0), (96, 0), (96, 96), (0, 96)], [(0, 0), (48, 0), (48, 96), (0, 96)]])
        z.set_lines(0, [(48, 0, 48, 96)])
        return z

    manual = make()
    exp = manual.update(res, tracks)
    z = make()
    res2, tracks2, got = rt.inference_batch_zones(frames, m, track.Tracker(1, 4, 36), z)
    assert torch.equal(res2.count, res.count) and torch.equal(tracks2.ids, tracks.ids)
    for k in OUTS:
        assert torch.equal(getattr(got, k), getattr(exp, k)), k
    for k in z.state:
        assert torch.equal(z.state[k], manual.state[k]), k
    # the same frame four times: everybody is born in frame 0 and stays; the whole-image zone holds every valid person
    inside = got.inside[:, :n]
    assert got.slot[:, :n].tolist() == [list(range(n))] * 4 and (got.slot[:, n:] == -1).all() and not got.inside[:, n:].any()
    n0, n1 = int((inside[0] & 1).sum()), int((inside[0] >> 1 & 1).sum())
    assert n0 > 0 and got.zone[:, 0].tolist() == [[n0, n0, 0, 0], [n0, 0, 0, 0], [n0, 0, 0, n0], [n0, 0, 0, n0]]
    assert got.zone[:, 1].tolist() == [[n1, n1, 0, 0], [n1, 0, 0, 0], [n1, 0, 0, n1], [n1, 0, 0, n1]]
    assert not got.line.any() and not got.zone[:, 2:].any() and z.flags().tolist() == [0]
    zt, lt = z.totals()
    assert zt[0, :2].tolist() == [[n0, 0], [n1, 0]] and not lt.any()
