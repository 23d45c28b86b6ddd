"""GPU: csrc/stgcn.hip.  The two MFMA stages against the derived per-element bounds of tests/stgcn_cases.py (f64 reference from
the unfolded state dict, tests/stgcn_ref.py); the selection byte for byte; the whole network against the restatement within
4 E, E = max |restatement in f32 - restatement in f64| on the same inputs; invariance under the population, graph replay,
the rt entry point and the refusals.

Measured on an MI355X (profiles/actions_errors.txt, rewritten by test_whole_network): see that file for E and the kernels'
error per network."""
import os

import numpy as np
import pytest
import torch

import stgcn_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ERRORS = os.path.join(ROOT, "profiles", "actions_errors.txt")
PAD = 64                     # canary elements on either side of an output (256 bytes: the alignment of the view is kept)
SENT = 12345.0


def _guarded(n, dtype=torch.float32, fill=SENT):
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n]


def _intact(buf, fill=SENT):
    return bool((buf[:PAD] == fill).all()) and bool((buf[-PAD:] == fill).all())


def _AC():
    from pytorch_pose_proposal_network_amd import actions
    return actions


def _weights(c):
    AC = _AC()
    return AC.BlockWeights(AC.fold(c["spec"], c["sd"])["blocks"][0], "cuda")


def _n(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


# ---- the stages ---------------------------------------------------------------------------------------------------------------
def _run_gcn(c):
    AC, k = _AC(), c["case"]
    size = k.n * k.T * k.K * k.cout
    buf, out = _guarded(size + k.T * k.K * k.cout)                     # room for one clip past the active ones
    AC.launch_gcn(AC.desc(k.K, 3, k.T, k.cin, k.cout, 1, "none"), _weights(c), SC.to_ntvc(c["x"]).cuda(), _n(k.n), 64, out)
    torch.cuda.synchronize()
    assert _intact(buf) and bool((out[size:] == SENT).all()), "written outside the active clips"
    return SC.to_nctv(out[:size].view(k.n, k.T, k.K, k.cout)).cpu()


def _run_tcn(c):
    AC, k = _AC(), c["case"]
    To = (k.T - 1) // k.stride + 1
    size = k.n * To * k.K * k.cout
    buf, out = _guarded(size + To * k.K * k.cout)
    AC.launch_tcn(AC.desc(k.K, 3, k.T, k.cin, k.cout, k.stride, k.residual), _weights(c), SC.to_ntvc(c["u"]).cuda(),
                  SC.to_ntvc(c["x"]).cuda(), _n(k.n), 64, out)
    torch.cuda.synchronize()
    assert _intact(buf) and bool((out[size:] == SENT).all()), "written outside the active clips"
    return SC.to_nctv(out[:size].view(k.n, To, k.K, k.cout)).cpu()


@pytest.mark.parametrize("name", sorted(SC.GCN_CASES))
def test_gcn_stage_within_its_bound(name):
    c = SC.gcn_case(name)
    r = SC.ratio(_run_gcn(c), c["ref"], c["bound"])
    print(f"gcn {name}: err / bound = {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("name", sorted(SC.TCN_CASES))
def test_tcn_stage_within_its_bound(name):
    c = SC.tcn_case(name)
    r = SC.ratio(_run_tcn(c), c["ref"], c["bound"])
    print(f"tcn {name}: err / bound = {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("name", sorted(SC.WALL_CASES))
def test_tcn_reads_nothing_across_a_clip_boundary(name):
    c = SC.tcn_case(name)
    got = _run_tcn(c)
    assert bool(torch.isfinite(got).all())
    r = SC.ratio(got[1:2], c["ref"][1:2], c["bound"][1:2])              # the clip between two walls of 1e30
    print(f"tcn {name}: err / bound = {r:.4f}")
    assert r <= 1.0


def test_fewer_active_clips_than_given_leave_the_rest_alone():
    c = SC.gcn_case("16_16_n5")
    AC, k = _AC(), c["case"]
    per = k.T * k.K * k.cout
    buf, out = _guarded(5 * per)
    AC.launch_gcn(AC.desc(k.K, 3, k.T, k.cin, k.cout, 1, "none"), _weights(c), SC.to_ntvc(c["x"]).cuda(), _n(2), 64, out)
    torch.cuda.synchronize()
    assert _intact(buf) and bool((out[2 * per:] == SENT).all())
    got = SC.to_nctv(out[:2 * per].view(2, k.T, k.K, k.cout)).cpu()
    assert SC.ratio(got, c["ref"][:2], c["bound"][:2]) <= 1.0


# ---- selection ------------------------------------------------------------------------------------------------------------------
T_SEL = 4


def _population(kind, S, T, seed):
    rng = np.random.default_rng(seed)
    if kind == "none":
        ids, length = np.zeros((S, 64), np.int32), rng.integers(0, T + 1, (S, 64)).astype(np.int32)
    elif kind == "all":
        ids, length = np.arange(1, S * 64 + 1, dtype=np.int32).reshape(S, 64), np.full((S, 64), T, np.int32)
    else:                                                               # free slots, short clips, negative ids
        ids = rng.integers(-2, 5, (S, 64)).astype(np.int32) * (rng.random((S, 64)) < 0.7)
        length = rng.integers(0, T + 1, (S, 64)).astype(np.int32)
    x = rng.uniform(-0.6, 0.6, (S, 64, 3, T, 18)).astype(np.float32)
    return x, ids.astype(np.int32), length


def _batch(x, ids, length):
    from pytorch_pose_proposal_network_amd import clips
    return clips.ClipBatch(torch.from_numpy(x).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(length).cuda())


@pytest.fixture(scope="module")
def tiny():
    AC = _AC()
    spec = AC.stgcn_spec("tiny", 10)
    return spec, AC.random_state_dict(spec, 21)


@pytest.mark.parametrize("S", (1, 2))
@pytest.mark.parametrize("min_len", (1, T_SEL))
@pytest.mark.parametrize("kind", ("mixed", "none", "all"))
def test_selection_byte_for_byte(tiny, kind, min_len, S):
    AC = _AC()
    spec, sd = tiny
    m = AC.ActionModel(spec, sd, S, T_SEL, min_len)
    cap, nc = S * 64, spec.num_class
    guards = {}
    for name, n, dt, fill in (("logits", cap * nc, torch.float32, SENT), ("label", cap, torch.int32, 77), ("active", cap, torch.int32, 77),
                              ("rank", cap, torch.int32, 77), ("n_active", 1, torch.int32, 77), ("x0", m.x0.numel(), torch.float32, SENT)):
        buf, view = _guarded(n, dt, fill)
        guards[name] = (buf, fill)
        setattr(m, name, view.view(getattr(m, name).shape))
    x, ids, length = _population(kind, S, T_SEL, 5 + S)
    res = m(_batch(x, ids, length))
    torch.cuda.synchronize()
    on = ((ids != 0) & (length >= min_len)).reshape(-1)
    want = np.flatnonzero(on).astype(np.int32)
    n = len(want)
    assert {"mixed": 0 < n < cap, "none": n == 0, "all": n == cap}[kind]
    rank = np.full(cap, -1, np.int32)
    rank[want] = np.arange(n, dtype=np.int32)
    assert res.n_active.cpu().numpy().tobytes() == np.array([n], np.int32).tobytes()
    assert res.active.cpu().numpy().tobytes() == np.concatenate([want, np.full(cap - n, -1, np.int32)]).tobytes()
    assert m.rank.cpu().numpy().tobytes() == rank.tobytes()
    for name, (buf, fill) in guards.items():
        assert _intact(buf, fill), name
    label, logits = res.label.cpu().numpy().reshape(-1), res.logits.cpu().numpy().reshape(cap, nc)
    assert (label[~on] == -1).all() and logits[~on].tobytes() == bytes(4 * nc * int((~on).sum()))
    assert np.isfinite(logits).all() and (label[on] == logits[on].argmax(1)).all()
    # data_bn: three roundings (scale, shift, the fused multiply-add) on |x scale| + |shift|
    sc, sh = (v.reshape(18, 3) for v in AC.fold(spec, sd)["in"])
    x0 = m.x0.cpu().numpy().reshape(cap, T_SEL, 18, 3)
    xa = x.reshape(cap, 3, T_SEL, 18)[want].transpose(0, 2, 3, 1).astype(np.float64)
    ref = xa * sc + sh
    assert (np.abs(x0[:n] - ref) <= 3 * SC.U * (np.abs(xa * sc) + np.abs(sh)) + SC.TINY).all()
    assert (x0[n:] == np.float32(SENT)).all()                          # nothing is written past the active clips
    by_id = res.to_host()
    assert [len(d) for d in by_id] == [len(set(ids[s][on.reshape(S, 64)[s]].tolist())) for s in range(S)]


# ---- the whole network ----------------------------------------------------------------------------------------------------------
SLOTS_USED = (3, 17, 40)
_lines = {}


def _record(name, line):
    _lines[name] = line
    old = {}
    if os.path.exists(ERRORS):
        for ln in open(ERRORS).read().splitlines():
            if ":" in ln:
                old[ln.split(":", 1)[0]] = ln
    old.update({k: f"{k}: {v}" for k, v in _lines.items()})
    with open(ERRORS, "w") as f:
        f.write("\n".join(old[k] for k in sorted(old)) + "\n")


def _network_batch(net, S, slots):
    """A ClipBatch with net's clips in `slots` (flat indices) of S streams, everything else free."""
    T, K = net["T"], net["spec"].K
    x, ids, length = np.zeros((S * 64, 3, T, K), np.float32), np.zeros(S * 64, np.int32), np.zeros(S * 64, np.int32)
    for i, s in enumerate(slots):
        x[s], ids[s], length[s] = net["clips"][i].numpy(), 100 + i, T
    return _batch(x.reshape(S, 64, 3, T, K), ids.reshape(S, 64), length.reshape(S, 64))


@pytest.mark.parametrize("name", ("tiny", "paper"))
def test_whole_network(name):
    net = SC.network(name)
    E, ref = net["E"], net["ref64"]
    m = _AC().ActionModel(net["spec"], net["sd"], 1, net["T"])
    res = m(_network_batch(net, 1, SLOTS_USED))
    torch.cuda.synchronize()
    assert res.active[:4].tolist() == list(SLOTS_USED) + [-1] and int(res.n_active) == 3
    logits = res.logits[0, list(SLOTS_USED)].cpu().double()
    err = float((logits - ref).abs().max())
    _record(name, f"T = {net['T']}, 3 clips, max |logit| = {float(ref.abs().max()):.4f}; E = max |restatement f32 - f64| = {E:.3e}; "
                  f"kernels' max |logit - restatement f64| = {err:.3e} = {err / E:.2f} E (allowed: 4 E)")
    print(_lines[name])
    assert err <= 4 * E
    label = res.label[0, list(SLOTS_USED)].cpu().long()
    assert torch.equal(label, res.logits[0, list(SLOTS_USED)].cpu().argmax(1))
    decided = SC.margins(ref) > 8 * E
    assert int((~decided).sum()) <= 0.05 * len(SLOTS_USED)
    assert torch.equal(label[decided], ref.argmax(1)[decided])
    others = [i for i in range(64) if i not in SLOTS_USED]
    assert (res.label[0, others] == -1).all() and not res.logits[0, others].any()
    assert {k: v[0] for k, v in res.to_host()[0].items()} == {100 + i: int(label[i]) for i in range(3)}


def test_logits_do_not_depend_on_the_population_or_the_place():
    net = SC.network("tiny")
    m = _AC().ActionModel(net["spec"], net["sd"], 2, net["T"])
    alone = m(_network_batch(net, 2, (5,))).logits[0, 5].clone()
    T, K = net["T"], net["spec"].K
    rng = np.random.default_rng(9)
    x = np.zeros((2, 64, 3, T, K), np.float32)
    x[1] = rng.uniform(-0.6, 0.6, (64, 3, T, K)).astype(np.float32)
    x[1, 9] = net["clips"][0].numpy()
    ids, length = np.zeros((2, 64), np.int32), np.zeros((2, 64), np.int32)
    ids[1], length[1] = np.arange(1, 65), T
    res = m(_batch(x, ids, length))
    assert int(res.n_active) == 64 and res.active[9].item() == 64 + 9
    assert torch.equal(res.logits[1, 9].view(torch.int32), alone.view(torch.int32))
    assert bool(res.logits[1].any(dim=1).all()) and len(set(res.logits[1, :, 0].tolist())) > 32


# ---- graph ----------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replays_on_any_population():
    net = SC.network("tiny")
    AC = _AC()
    T, K = net["T"], net["spec"].K
    m, direct = AC.ActionModel(net["spec"], net["sd"], 1, T), AC.ActionModel(net["spec"], net["sd"], 1, T)
    pops = []
    for seed, live in ((1, (0, 2, 63)), (2, tuple(range(5, 47))), (3, ())):
        rng = np.random.default_rng(seed)
        x = rng.uniform(-0.6, 0.6, (1, 64, 3, T, K)).astype(np.float32)
        ids, length = np.zeros((1, 64), np.int32), np.zeros((1, 64), np.int32)
        for s in live:
            ids[0, s], length[0, s] = s + 1, T
        pops.append((x, ids, length))
    staged = _batch(*pops[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(staged)                                                       # the module is loaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m(staged)
    got = []
    for x, ids, length in pops:                                         # no synchronisation between the replays
        staged.x.copy_(torch.from_numpy(x), non_blocking=True)
        staged.ids.copy_(torch.from_numpy(ids), non_blocking=True)
        staged.length.copy_(torch.from_numpy(length), non_blocking=True)
        g.replay()
        got.append([t.clone() for t in (m.logits, m.label, m.active, m.n_active)])
    torch.cuda.synchronize()
    for (x, ids, length), mine in zip(pops, got):
        res = direct(_batch(x, ids, length))
        for a, b in zip(mine, (res.logits, res.label, res.active, res.n_active)):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    logits, label, active, n_active = got[2]
    assert not logits.any() and (label == -1).all() and (active == -1).all() and int(n_active) == 0
    assert int(got[0][3]) == 3 and int(got[1][3]) == 42


# ---- network level: D-22, float32, 96 x 96 ----------------------------------------------------------------------------------------
def test_rt_entry_point(tiny):
    from pytorch_pose_proposal_network_amd import clips, drn, model, prng, rt, synth, track
    AC = _AC()
    spec, sd = tiny
    g = np.load(os.path.join(GOLDEN, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    net = model.PoseProposalNet(drn.drn_d_22(), insize=(96, 96), outsize=(6, 6), compute_dtype="float32").cuda()
    net.load_state_dict(synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats))
    net.eval()
    one = torch.from_numpy(prng.u8_frames(515, 1, (96, 96))).cuda()
    frames = one.expand(4, -1, -1, -1).contiguous()
    manual_clips = clips.PoseClips(1, 4, 36, length=6)
    res, tracks, rows, batch = rt.inference_batch_clips(frames, net, track.Tracker(1, 4, 36), manual_clips)
    n = int(res.count[0])
    assert 0 < n <= 36
    exp = AC.ActionModel(spec, sd, 1, 6, min_len=4)(batch)
    exp = [t.clone() for t in (exp.logits, exp.label, exp.active, exp.n_active)]

    pc, am = clips.PoseClips(1, 4, 36, length=6), AC.ActionModel(spec, sd, 1, 6, min_len=4)
    res2, tracks2, rows2, batch2, act = rt.inference_batch_actions(frames, net, track.Tracker(1, 4, 36), pc, am)
    assert torch.equal(res2.count, res.count) and torch.equal(tracks2.ids, tracks.ids) and torch.equal(rows2.row, rows.row)
    assert torch.equal(batch2.x, batch.x) and torch.equal(batch2.ids, batch.ids)
    for a, b in zip(exp, (act.logits, act.label, act.active, act.n_active)):
        assert torch.equal(a, b)
    assert int(act.n_active) == n and act.active[:n].tolist() == list(range(n)) and (act.label[0, :n] >= 0).all()
    assert (act.label[0, n:] == -1).all() and sorted(act.to_host()[0]) == list(range(1, n + 1))
    # a model that wants full clips finds none after four frames of six
    full = AC.ActionModel(spec, sd, 1, 6)
    assert int(full(batch2).n_active) == 0 and (full.label == -1).all()
    with pytest.raises(ValueError):
        rt.inference_batch_actions(frames, net, track.Tracker(1, 4, 36), pc, AC.ActionModel(spec, sd, 1, 8))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_return_the_documented_codes(tiny):
    from pytorch_pose_proposal_network_amd import lib
    for what, rc, want in SC.refusals(lib):
        assert rc == want, what
    AC = _AC()
    spec, sd = tiny
    with pytest.raises(ValueError):
        AC.ActionModel(spec, sd, 0, 8)
    with pytest.raises(ValueError):
        AC.ActionModel(spec, sd, 1, 257)
    with pytest.raises(ValueError):
        AC.ActionModel(AC.STGCNSpec(((16, 16, 1, "identity"),), 4), AC.random_state_dict(AC.STGCNSpec(((16, 16, 1, "identity"),), 4), 1), 1, 8)
    m = AC.ActionModel(spec, sd, 1, 8)
    x, ids, length = _population("all", 1, 8, 1)
    with pytest.raises(ValueError):
        m(_batch(x[:, :, :, :7], ids, length))                          # clips of another length
