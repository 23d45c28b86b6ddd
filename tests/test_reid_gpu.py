"""GPU: the re-identification's kernels against tests/reid_ref.py, every byte.  ppn_people_descr on the four formats (tight and
padded pitches, a frame stride above the planes, planes at odd addresses, rectangles below, at and above the sample grid, at
the picture's last row and column, and every kind of slot that must not be read); ppn_reid_update on the shared cases of
tests/reid_cases.py laid out as 2 streams x 3 frames, a crowd that overflows the gallery, cut invariance and repeatability;
the rects -> describe -> update triple under graph capture; the tracker, the clips and the network in front of and behind it.
Every case stays inside its buffers by construction; the outputs are followed by sentinel bytes that are checked."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import crops_ref as CR
import reid_cases as RC
import reid_ref as R
import track_cases as TC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL, TAIL = 0xC3, 64
FORMATS = ("nv12", "i420", "yuyv", "bgr")
PIX = {"nv12": 0, "i420": 1, "yuyv": 2, "bgr": 3}
SC = RC.scenarios()


def _guarded(host):
    """(the over-allocated byte buffer, the view that holds `host`): TAIL sentinel bytes follow the view."""
    host = np.ascontiguousarray(host)
    nb = host.nbytes
    big = torch.full((nb + TAIL,), SENTINEL, dtype=torch.uint8, device="cuda")
    big[:nb] = torch.from_numpy(host.reshape(-1).view(np.uint8))
    return big, nb


def _back(big, nb, like):
    raw = big.cpu().numpy()
    assert (raw[nb:] == SENTINEL).all(), "bytes behind an output were written"
    return raw[:nb].view(like.dtype).reshape(like.shape)


def _lib():
    from pytorch_pose_proposal_network_amd import lib
    return lib, lib.load()


# ---- the descriptor -------------------------------------------------------------------------------------------------------
BIG = 2 ** 31 - 2
# name -> (H, W, extra bytes per row, extra bytes per frame, the planes' address modulo 4, [frame][slot] = (rect, status))
TABLES = {
    "tiny_tight": (16, 16, 0, 0, 0, [[((0, 0, 16, 16), 0), ((4, 4, 8, 8), 0), ((8, 8, 8, 8), 0), ((0, 0, 0, 0), 1),
                                      ((2, 2, 8, 8), 2)]]),
    "padded_odd_planes": (48, 64, 10, 37, 1, [
        [((0, 0, 48, 64), 0), ((40, 56, 8, 8), 0), ((-2, 0, 8, 8), 0), ((44, 0, 8, 8), 0), ((0, 60, 8, 8), 0)],
        [((0, 1, 8, 8), 0), ((1, 0, 8, 8), 0), ((4, 6, 8, 8), 0), ((0, 0, 8, 7), 0), ((0, 0, 7, 8), 0)],
        [((10, 11, 1, 5), 0), ((46, 62, 2, 2), 0), ((0, 0, 0, 0), 1), ((2, 2, BIG, 4), 0), ((6, 2, 20, 30), 4)]]),
    # the sample grid itself: 96 x 32, and rectangles above it
    "grid_sized": (100, 36, 6, 0, 2, [[((2, 2, 96, 32), 0), ((0, 0, 100, 36), 0), ((0, -2, 96, 32), 0)],
                                      [((4, 4, 96, 32), 0), ((0, 0, 98, 34), 0), ((6, 2, 96, 32), 3)]]),
}


def _surface_case(fmt, name, seed):
    H, W, pad, gap, mod, table = TABLES[name]
    row = {"nv12": W, "i420": W, "yuyv": 2 * W, "bgr": 3 * W}[fmt]
    pitch = row + pad + (pad & 1 if fmt == "i420" else 0)            # I420: the chroma pitch is half of an even pitch
    nbytes, pitch, pc, uo, vo = R.layout(fmt, H, W, pitch)
    Fr, stride = len(table), nbytes + gap
    host = np.random.default_rng(seed).integers(0, 256, (Fr, stride), dtype=np.uint8)
    for f in range(Fr):                                              # a flat patch, so that some histograms are single bins
        host[f, :8 * pitch] = 77
    roi = np.array([[r for r, _ in fr] for fr in table], np.int32)
    status = np.array([[s for _, s in fr] for fr in table], np.int32)
    return dict(H=H, W=W, pitch=pitch, pc=pc, uo=uo, vo=vo, stride=stride, host=host, roi=roi, status=status, mod=mod)


def _run_descr(fmt, c):
    lib, l = _lib()
    Fr, Rn = c["status"].shape
    store = torch.zeros(c["host"].size + 8, dtype=torch.uint8, device="cuda")
    off = (c["mod"] - store.data_ptr()) % 4
    dev = store[off:off + c["host"].size]
    dev.copy_(torch.from_numpy(c["host"].reshape(-1)))
    base = dev.data_ptr()
    assert base % 4 == c["mod"]
    surf = lib.YuvSurface(format=PIX[fmt], height=c["H"], width=c["W"], pitch=c["pitch"], pitch_c=c["pc"],
                          frame_stride=c["stride"], y=base, u=None if c["uo"] is None else base + c["uo"],
                          v=None if c["vo"] is None else base + c["vo"], matrix=0, full_range=0)
    roi, status = torch.from_numpy(c["roi"]).cuda(), torch.from_numpy(c["status"]).cuda()
    d0, v0 = np.full((Fr, Rn, R.LEN), 0xABCD, np.uint16), np.full((Fr, Rn), 0x55, np.int32)
    (dbig, dn), (vbig, vn) = _guarded(d0), _guarded(v0)
    lib.check(l.ppn_people_descr(C.byref(surf), Fr, roi.data_ptr(), status.data_ptr(), Rn, dbig.data_ptr(), vbig.data_ptr(),
                                 lib.current_stream_ptr()), "ppn_people_descr")
    torch.cuda.synchronize()
    assert torch.equal(roi.cpu(), torch.from_numpy(c["roi"])) and torch.equal(status.cpu(), torch.from_numpy(c["status"]))
    assert torch.equal(dev.cpu(), torch.from_numpy(c["host"].reshape(-1)))                   # the surface is only read
    return _back(dbig, dn, d0), _back(vbig, vn, v0)


_DESCR_REF = {}


def _descr_ref(fmt, name):
    if (fmt, name) not in _DESCR_REF:
        c = _surface_case(fmt, name, 40 + len(name))
        _DESCR_REF[fmt, name] = (c, R.people_descr(c["host"], fmt, c["H"], c["W"], c["roi"], c["status"], c["pitch"]))
    return _DESCR_REF[fmt, name]


@pytest.mark.parametrize("name", list(TABLES))
@pytest.mark.parametrize("fmt", FORMATS)
def test_descriptors_match_the_restatement(fmt, name):
    c, (descr, valid) = _descr_ref(fmt, name)
    got_d, got_v = _run_descr(fmt, c)
    assert np.array_equal(got_v, valid), (got_v.tolist(), valid.tolist())
    assert np.array_equal(got_d, descr), np.argwhere(got_d != descr)[:5].tolist()
    assert not got_d[valid == 0].any()                                                       # zeros, as specified
    assert (got_d[valid == 1].reshape(-1, 9, 8).sum(axis=2) == 1024).all()
    if name == "tiny_tight":
        assert valid.tolist() == [[1, 1, 1, 0, 0]]
    if name == "padded_odd_planes":                                  # odd x0 / y0 / w / h: bad exactly where chroma is shared
        odd = {"nv12": [0, 0, 1, 0, 0], "i420": [0, 0, 1, 0, 0], "yuyv": [0, 1, 1, 0, 1], "bgr": [1, 1, 1, 1, 1]}[fmt]
        assert valid[0].tolist() == [1, 1, 0, 0, 0] and valid[1].tolist() == odd
        assert valid[2].tolist() == [1 if fmt == "bgr" else 0, 1, 0, 0, 0]                   # h = 1 in BGR
    if name == "grid_sized":
        assert valid.tolist() == [[1, 1, 0], [1, 1, 0]]
    again_d, again_v = _run_descr(fmt, c)
    assert again_d.tobytes() == got_d.tobytes() and again_v.tobytes() == got_v.tobytes()      # two runs, identical bytes


# ---- the gallery ----------------------------------------------------------------------------------------------------------
def _run_gallery(case, state=None):
    """The case's calls through ppn_reid_update with guarded outputs: per call (outputs, state after it)."""
    lib, l = _lib()
    S, Fr, M = case["streams"], case["frames"], case["M"]
    cfg = lib.ReIdCfg(**case["cfg"])
    st0 = R.fresh_state(S) if state is None else state
    names = [n for n, _ in lib.ReIdState._fields_]
    held = {n: _guarded(st0[n]) for n in names}
    st = lib.ReIdState(*(held[n][0].data_ptr() for n in names))
    steps = []
    for call in case["calls"]:
        dev = {k: torch.from_numpy(np.ascontiguousarray(call[k])).cuda() for k in ("count", "ids", "descr", "valid")}
        nf = None if call["n_frames"] is None else torch.from_numpy(call["n_frames"]).cuda()
        o0 = dict(pid=np.full((S * Fr, M), 0x66, np.int32), sim=np.full((S * Fr, M), 0x66, np.int32),
                  live=np.full(S * Fr, 0x66, np.int32))
        outs = {k: _guarded(v) for k, v in o0.items()}
        lib.check(l.ppn_reid_update(C.byref(cfg), C.byref(st), dev["count"].data_ptr(), dev["ids"].data_ptr(),
                                    dev["descr"].data_ptr(), dev["valid"].data_ptr(), S, Fr, M,
                                    None if nf is None else nf.data_ptr(), outs["pid"][0].data_ptr(),
                                    outs["sim"][0].data_ptr(), outs["live"][0].data_ptr(), lib.current_stream_ptr()),
                  "ppn_reid_update")
        torch.cuda.synchronize()
        for k in dev:
            assert torch.equal(dev[k].cpu(), torch.from_numpy(np.ascontiguousarray(call[k]))), k      # inputs are only read
        steps.append(({k: _back(*outs[k], o0[k]) for k in o0}, {n: _back(*held[n], st0[n]).copy() for n in names}))
    return steps


def _assert_steps(got, exp, what):
    assert len(got) == len(exp)
    for i, ((go, gs), (eo, es)) in enumerate(zip(got, exp)):
        for k in eo:
            assert np.array_equal(go[k], eo[k]), (what, "call", i, k, go[k].tolist(), eo[k].tolist())
        for k in es:
            assert gs[k].tobytes() == es[k].tobytes(), (what, "call", i, "state", k, np.argwhere(gs[k] != es[k])[:4].tolist())
        R.assert_invariant(gs)
        for b in range(go["pid"].shape[0]):                          # the positive pids of an image are distinct
            pos = go["pid"][b][go["pid"][b] > 0]
            assert len(set(pos.tolist())) == len(pos)


@pytest.mark.parametrize("name", list(SC))
def test_gallery_cases_as_two_streams_of_three_frames(name):
    scn = SC[name]
    case = RC.as_case([scn["seq"], RC.video(len(name), 5)], scn["cfg"], 3, 7)
    _assert_steps(_run_gallery(case), RC.run_ref(case), name)


def test_gallery_videos_with_a_small_memory_and_few_rois():
    cfg = R.make_cfg(thr=5000, memory=2, max_rois=4, min_lost=2)
    case = RC.as_case([RC.video(5, 9, p_rename=0.3), RC.video(6, 7, n_people=7, p_here=0.9)], cfg, 3, 7)
    exp = RC.run_ref(case)
    _assert_steps(_run_gallery(case), exp, "videos")
    assert max(int(o["sim"].max()) for o, _ in exp) >= 5000          # somebody was relinked


def test_a_crowd_overflows_the_gallery():
    case = RC.crowd()
    exp = RC.run_ref(case)
    got = _run_gallery(case)
    _assert_steps(got, exp, "crowd")
    assert got[0][1]["flags"][0] == R.SLOT_OVERFLOW and got[0][0]["live"][0] == 128
    assert (got[0][0]["pid"][0, 128:130] == -1).all() and (got[3][0]["pid"][0, :130] == -1).sum() == 2
    again = _run_gallery(case)                                       # two runs give identical bytes
    for (go, gs), (ao, as_) in zip(got, again):
        assert all(go[k].tobytes() == ao[k].tobytes() for k in go) and all(gs[k].tobytes() == as_[k].tobytes() for k in gs)


def test_cut_invariance_on_the_device():
    seqs = [RC.video(1, 6), RC.video(11, 6, p_rename=0.4)]
    cfg = R.make_cfg(thr=5000, memory=2, max_rois=4)
    cases = (RC.as_case(seqs, cfg, 6, 7), RC.as_case(seqs, cfg, 1, 7), RC.as_case(seqs, cfg, 4, 7, cuts=[(2, 2), (4, 4)]))
    whole, ones, split = (_run_gallery(c) for c in cases)
    for c, got in zip(cases, (whole, ones, split)):
        _assert_steps(got, RC.run_ref(c), "cuts")
    for k, v in whole[-1][1].items():
        assert v.tobytes() == ones[-1][1][k].tobytes() == split[-1][1][k].tobytes(), k
    for s in range(2):
        for t in range(6):
            c, tt = (0, t) if t < 2 else (1, t - 2)
            for k in ("pid", "sim"):
                w = whole[0][0][k][s * 6 + t].tolist()
                assert w == ones[t][0][k][s].tolist() == split[c][0][k][s * 4 + tt].tolist(), (k, s, t)


def test_an_unprocessed_stream_keeps_every_byte():
    case = RC.as_case([SC["three_return"]["seq"], RC.video(3, 5)], R.make_cfg(thr=RC.THR), 3, 7)
    first = _run_gallery(dict(case, calls=case["calls"][:1]))[0][1]
    call = dict(case["calls"][1], n_frames=np.array([0, -3], np.int32))
    (out, st), = _run_gallery(dict(case, calls=[call]), state=first)
    for k in st:
        assert st[k].tobytes() == first[k].tobytes(), k
    assert (out["pid"] == -1).all() and (out["sim"] == -1).all() and (out["live"] == -1).all()


# ---- the Python layer: rects -> describe -> update ------------------------------------------------------------------------
def _result(call, M):
    from pytorch_pose_proposal_network_amd import decode
    t = {k: torch.from_numpy(np.ascontiguousarray(call[k])).cuda() for k in ("count", "kp_cell", "bbox", "score")}
    return decode.DecodeResult(t["count"], t["kp_cell"], None, t["bbox"], t["score"], M)


def _walk_reid(**kw):
    from pytorch_pose_proposal_network_amd import reid
    args = dict(max_rois=RC.WALK_R, K=RC.WALK_K, sim_thr=0.7)
    args.update(kw)
    return reid.ReId(1, 1, RC.WALK_M, RC.WALK_HW, "nv12", **args)


def _assert_walk_step(r, out, step, t):
    host = out.to_host()
    for k in ("roi", "status", "descr", "valid"):
        assert np.array_equal(host[k], step[k]), (t, k)
    for k in ("pid", "sim", "live"):
        assert np.array_equal(host[k], step["out"][k]), (t, k, host[k].tolist(), step["out"][k].tolist())
    st = r.state_to_host()
    for k, v in step["state"].items():
        assert st[k].tobytes() == v.tobytes(), (t, "state", k)


def test_the_triple_replays_from_a_captured_graph():
    from pytorch_pose_proposal_network_amd import track
    ref = RC.walk_ref()
    w, steps = ref["walk"], ref["steps"]
    staged = _result(w["calls"][0], RC.WALK_M)
    ids = torch.from_numpy(steps[0]["ids"]).cuda()
    tracks = track.TrackResult(ids, None, None, None, staged.count)
    raw = torch.from_numpy(w["raw"][0:1]).cuda()
    r = _walk_reid()
    assert r.thr == RC.THR
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _walk_reid().reid(raw, staged, tracks)                       # the module is loaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                        # three launches in a row: a linear graph
        r.reid(raw, staged, tracks)
    r.reset()                                                        # the capture launched nothing; be sure of the state anyway
    direct = _walk_reid()
    for t, step in enumerate(steps):
        for k in ("count", "kp_cell", "bbox", "score"):              # the people, their ids and the frame change in place
            getattr(staged, k).copy_(torch.from_numpy(np.ascontiguousarray(w["calls"][t][k])))
        ids.copy_(torch.from_numpy(step["ids"]))
        raw.copy_(torch.from_numpy(w["raw"][t:t + 1]))
        for x in (r.pid, r.sim, r.live, r.descr, r.valid, r.roi, r.status):
            x.view(torch.uint8).fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        _assert_walk_step(r, r.out, step, t)                         # the gallery is carried from replay to replay
        out = direct.reid(raw, staged, tracks)
        _assert_walk_step(direct, out, step, t)


def test_the_walk_with_the_tracker_and_the_clips_on_the_device():
    """The returning person gets a new track id and its old pid; fed with as_tracks() the clips keep ONE slot for it, with
    the tracker's own ids two."""
    from pytorch_pose_proposal_network_amd import clips, track
    ref = RC.walk_ref()
    w, steps = ref["walk"], ref["steps"]
    tracker = track.Tracker(1, 1, RC.WALK_M, K=RC.WALK_K, max_age=RC.WALK_MAX_AGE)
    r = _walk_reid()
    mk = lambda: clips.PoseClips(1, 1, RC.WALK_M, K=RC.WALK_K, length=16, max_gap=w["T"])
    by_pid, by_tid = mk(), mk()
    rows = []
    for t, step in enumerate(steps):
        res = _result(w["calls"][t], RC.WALK_M)
        tracks = tracker.update(res)
        assert np.array_equal(tracks.ids.cpu().numpy(), step["ids"]), t
        out = r.reid(torch.from_numpy(w["raw"][t:t + 1]).cuda(), res, tracks)
        _assert_walk_step(r, out, step, t)
        as_tracks = out.as_tracks(tracks)
        assert as_tracks.ids is out.pid and as_tracks.xy is tracks.xy and as_tracks.hits is tracks.hits
        rows.append(by_pid.push(res, as_tracks).row.cpu().numpy()[0].copy())
        by_tid.push(res, tracks)
    first, last = w["away"]
    assert rows[last + 1][2] == rows[first - 1][2] >= 0              # the same clip slot before and after the absence
    st_pid, st_tid = by_pid.state_to_host(), by_tid.state_to_host()
    assert (st_pid["id"][0] != 0).sum() == 3 and (st_tid["id"][0] != 0).sum() == 4
    slot = int(rows[-1][2])
    T = w["T"]                                                       # the clip goes on where the tracker's ids start one anew
    assert st_pid["len"][0, slot] == T and sorted(st_tid["len"][0][st_tid["id"][0] != 0].tolist()) == [T - last - 1, T, T, T]
    assert r.flags().tolist() == [0]


@pytest.mark.parametrize("fmt", ("bgr", "yuyv"))
def test_more_people_than_rois_and_a_count_above_max_humans(fmt):
    """count 9 with max_humans 7 and max_rois 4: people 4..6 get ids but no descriptor, rows >= 7 do not exist."""
    from pytorch_pose_proposal_network_amd import reid, track
    H, W, M, K, Rn = 40, 64, 7, 3, 4
    people = [TC.person(10 + 3 * i, 8 + 8 * i, K, h=16, w=10, score=0.9 - 0.05 * i) for i in range(7)]
    call = TC.pack([people, people[:5]], M, K, counts=[9, None])
    nbytes, pitch = R.layout(fmt, H, W)[:2]
    host = np.random.default_rng(9).integers(0, 256, (2, nbytes), dtype=np.uint8)
    ids = np.array([[11, 12, 13, 14, 15, 16, 17], [21, 22, 13, 24, 15, -1, -1]], np.int32)
    r = reid.ReId(2, 1, M, (H, W), fmt, max_rois=Rn, K=K, min_size=2, sim_thr=0.3)
    raw = torch.from_numpy(host).cuda()
    raw = raw.view(2, H, W, 3) if fmt == "bgr" else raw
    res = _result(call, M)
    rcfg = R.make_cfg(thr=r.thr, max_rois=Rn)
    st = R.fresh_state(2)
    for _ in range(2):                                               # the second call binds everybody
        out = r.reid(raw, res, track.TrackResult(torch.from_numpy(ids).cuda(), None, None, None, res.count)).to_host()
        roi, status = CR.people_rois(call["count"], call["kp_cell"], call["bbox"], (H, W), 1.0, 1.0, Rn, CR.MODE_PEOPLE, 0.0,
                                     0.0, CR.ALIGN[fmt], 2)
        descr, valid = R.people_descr(host, fmt, H, W, roi, status)
        exp = R.reid_update(rcfg, st, call["count"], ids, descr, valid, 2, 1)
        assert np.array_equal(out["roi"], roi) and np.array_equal(out["status"], status) and valid.sum() >= 6
        assert np.array_equal(out["descr"], descr) and np.array_equal(out["valid"], valid)
        for k in ("pid", "sim", "live"):
            assert np.array_equal(out[k], exp[k]), k
        got = r.state_to_host()
        for k, v in st.items():
            assert got[k].tobytes() == v.tobytes(), k
    assert (exp["pid"][0] > 0).all() and st["n"][0, 4:7].tolist() == [0, 0, 0] and st["n"][0, :4].tolist() == [2] * 4


# ---- network level: D-22, float32, 96 x 96 ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    from pytorch_pose_proposal_network_amd import drn, model, synth
    g = np.load(os.path.join(GOLDEN, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    m = model.PoseProposalNet(drn.drn_d_22(), insize=(96, 96), outsize=(6, 6), compute_dtype="float32").cuda()
    m.load_state_dict(synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats))
    m.eval()
    return m


def test_inference_reid_on_the_network(net):
    from pytorch_pose_proposal_network_amd import crops, reid, rt, track
    h, w, F_, M = 64, 96, 2, 36
    host = np.random.default_rng(700).integers(0, 256, (F_, R.layout("nv12", h, w)[0]), dtype=np.uint8)
    raw = torch.from_numpy(host).cuda()
    r = reid.ReId(1, F_, M, (h, w), "nv12", coords_hw=(96, 96), max_rois=8, min_size=4)
    res, tracks, out = rt.inference_reid(raw, "nv12", (h, w), net, track.Tracker(1, F_, M), r, size=96)
    kept = {k: getattr(res, k).clone() for k in ("count", "kp_cell", "limb_arg", "bbox", "score")}
    got = out.to_host()
    ids = tracks.ids.cpu().numpy()
    cr = crops.PersonCropper(F_, M, (h, w), "nv12", (32, 24), max_crops=8, min_size=4, coords_hw=(96, 96))
    res2, _, tracks2 = rt.inference_crops(raw, "nv12", (h, w), net, cr, tracker=track.Tracker(1, F_, M), size=96)
    same = lambda x, y: torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
    assert same(kept["count"], res2.count)                           # the same DecodeResult bytes
    for f, n in enumerate(res2.count.cpu().tolist()):                # the rows of people: a decode writes no others
        for k in ("kp_cell", "limb_arg", "bbox", "score"):
            assert same(kept[k][f, :min(n, M)], getattr(res2, k)[f, :min(n, M)]), (k, f)
    assert np.array_equal(ids, tracks2.ids.cpu().numpy())
    # the restatement on the people that came out
    count = kept["count"].cpu().numpy()
    sy, sx = CR.scales((h, w), (96, 96))
    roi, status = CR.people_rois(count, kept["kp_cell"].cpu().numpy(), kept["bbox"].cpu().numpy(), (h, w), sy, sx, 8,
                                 CR.MODE_PEOPLE, 0.0, 0.0, (2, 2), 4)
    descr, valid = R.people_descr(host, "nv12", h, w, roi, status)
    st = R.fresh_state(1)
    exp = R.reid_update(R.make_cfg(thr=r.thr, max_rois=8), st, count, ids, descr, valid, 1, F_)
    assert np.array_equal(got["roi"], roi) and np.array_equal(got["status"], status)
    assert np.array_equal(got["descr"], descr) and np.array_equal(got["valid"], valid)
    for k in ("pid", "sim", "live"):
        assert np.array_equal(got[k], exp[k]), k
    state = r.state_to_host()
    R.assert_invariant(state)
    for b in range(F_):
        pos = got["pid"][b][got["pid"][b] > 0]
        assert len(set(pos.tolist())) == len(pos) and ((got["pid"][b] > 0) == (ids[b] > 0)).all()
    assert (got["pid"] > 0).sum() > 0 and valid.sum() > 0
    with pytest.raises(ValueError):
        rt.inference_reid(raw, "nv12", (h, w), net, track.Tracker(1, F_, M), r, size=96, flip=True)
    with pytest.raises(ValueError):                                  # a ReId that stands in another space is refused
        rt.inference_reid(raw, "nv12", (h, w), net, track.Tracker(1, F_, M),
                          reid.ReId(1, F_, M, (h, w), "nv12", coords_hw=(50, 50)), size=96)
