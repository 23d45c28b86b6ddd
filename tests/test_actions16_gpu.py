"""GPU: csrc/stgcn16.hip, the action model's float16 mode.  The two MFMA stages against the derived per-element bounds of
tests/stgcn16_cases.py (f64 reference on operands rounded to half, tests/stgcn16_ref.py) and, on small-integer operands, on
every byte; the selection byte for byte; the whole network against the emulation in f64 within 4 E16, E16 = max |emulation in
f32 arithmetic - emulation in f64| on the same inputs (from the emulation, never from the kernels); invariance under the
population, graph replay, the rt entry point and half_range_report.

Measured on an MI355X (profiles/actions_errors.txt, keys "tiny float16" and "paper float16", rewritten by
test_whole_network): see that file for E16 and the kernels' error per network."""
import os

import numpy as np
import pytest
import torch

import stgcn16_cases as SC16
import stgcn_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ERRORS = os.path.join(ROOT, "profiles", "actions_errors.txt")
PAD = 64                     # canary elements on either side of an output (the alignment of the view is kept)
SENT = 12352.0               # exactly representable in half (a multiple of 8 below 16384)
F16 = torch.float16


def _guarded(n, dtype=F16, fill=SENT):
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n]


def _intact(buf, fill=SENT):
    return bool((buf[:PAD] == fill).all()) and bool((buf[-PAD:] == fill).all())


def _AC():
    from pytorch_pose_proposal_network_amd import actions
    return actions


def _L():
    from pytorch_pose_proposal_network_amd import lib
    return lib


def _weights(c):
    """Of a random case: actions.py's own fold; of a hand-made case: its block."""
    AC = _AC()
    b = AC.fold(c["spec"], c["sd"])["blocks"][0] if "sd" in c else c["b"]
    return AC.BlockWeights(b, "cuda", "float16")


def _n(n):
    return torch.tensor([n], dtype=torch.int32, device="cuda")


def _half_ntvc(t, pad4=False):
    """[n, c, t, v] f64 holding half values -> half [n, t, v, c] on the device; cin = 3 with the zero pad channel."""
    h = SC.to_ntvc(t).to(F16)
    assert torch.equal(h.double(), SC.to_ntvc(t))
    if pad4 and h.shape[-1] == 3:
        h = torch.cat([h, torch.zeros_like(h[..., :1])], dim=-1).contiguous()
    return h.cuda()


# ---- the stages ---------------------------------------------------------------------------------------------------------------
def _run_gcn(c, n_active=None):
    AC, k = _AC(), c["case"]
    n = k.n if n_active is None else n_active
    per = k.T * k.K * k.cout
    buf, out = _guarded((k.n + 1) * per)                                # room for one clip past the given ones
    AC.launch_gcn(AC.desc(k.K, 3, k.T, k.cin, k.cout, 1, "none", _L().PPN_F16), _weights(c), _half_ntvc(c["x"], True), _n(n), 64, out)
    torch.cuda.synchronize()
    assert _intact(buf) and bool((out[n * per:] == SENT).all()), "written outside the active clips"
    return SC.to_nctv(out[:n * per].view(n, k.T, k.K, k.cout)).cpu()


def _run_tcn(c, n_active=None):
    AC, k = _AC(), c["case"]
    n = k.n if n_active is None else n_active
    To = (k.T - 1) // k.stride + 1
    per = To * k.K * k.cout
    buf, out = _guarded((k.n + 1) * per)
    AC.launch_tcn(AC.desc(k.K, 3, k.T, k.cin, k.cout, k.stride, k.residual, _L().PPN_F16), _weights(c), _half_ntvc(c["u"]),
                  _half_ntvc(c["x"], True), _n(n), 64, out)
    torch.cuda.synchronize()
    assert _intact(buf) and bool((out[n * per:] == SENT).all()), "written outside the active clips"
    return SC.to_nctv(out[:n * per].view(n, To, k.K, k.cout)).cpu()


@pytest.mark.parametrize("name", sorted(SC.GCN_CASES))
def test_gcn_stage_within_its_bound(name):
    c = SC16.gcn_case(name)
    r = SC.ratio(_run_gcn(c), c["ref"], c["bound"])
    print(f"gcn16 {name}: err / bound = {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("name", sorted(SC.TCN_CASES))
def test_tcn_stage_within_its_bound(name):
    c = SC16.tcn_case(name)
    r = SC.ratio(_run_tcn(c), c["ref"], c["bound"])
    print(f"tcn16 {name}: err / bound = {r:.4f}")
    assert r <= 1.0


@pytest.mark.parametrize("name", sorted(SC.WALL_CASES))
def test_tcn_reads_nothing_across_a_clip_boundary(name):
    c = SC16.tcn_case(name)
    got = _run_tcn(c)[1:2]                                              # the clip between two walls of 6.0e4
    assert bool(torch.isfinite(got).all())
    r = SC.ratio(got, c["ref"][1:2], c["bound"][1:2])
    print(f"tcn16 {name}: err / bound = {r:.4f}")
    assert r <= 1.0


def test_fewer_active_clips_than_given_leave_the_rest_alone():
    c = SC16.gcn_case("16_16_n5")
    assert SC.ratio(_run_gcn(c, 2), c["ref"][:2], c["bound"][:2]) <= 1.0
    c = SC16.tcn_case("16_16_k5_identity_t9")
    assert SC.ratio(_run_tcn(c, 1), c["ref"][:1], c["bound"][:1]) <= 1.0
    assert _run_gcn(SC16.gcn_case("16_16_n2"), 0).numel() == 0


def _same_bytes(got, ref):
    want = ref.to(F16)
    assert torch.equal(want.double(), ref)                              # the reference is exactly representable
    return got.contiguous().view(torch.int16).numpy().tobytes() == want.contiguous().view(torch.int16).numpy().tobytes()


def test_gcn_stage_on_small_integers_matches_on_every_byte():
    c = SC16.exact_gcn()
    assert SC16.small_integers(c["x"], c["y"], c["ref"]) and float(c["ref"].max()) > 8
    assert _same_bytes(_run_gcn(c), c["ref"])


def test_tcn_stage_on_small_integers_matches_on_every_byte():
    c = SC16.exact_tcn()
    assert SC16.small_integers(c["u"], c["x"], c["ref"]) and float(c["ref"].max()) > 8
    assert _same_bytes(_run_tcn(c), c["ref"])


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
    m = AC.ActionModel(spec, sd, S, T_SEL, min_len, compute_dtype="float16")
    cap, nc = S * 64, spec.num_class
    guards = {}
    for name, n, dt, fill in (("logits", cap * nc, torch.float32, SENT), ("label", cap, torch.int32, 77), ("active", cap, torch.int32, 77),
                              ("rank", cap, torch.int32, 77), ("n_active", 1, torch.int32, 77), ("x0", m.x0.numel(), F16, SENT)):
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
    f32 = AC.ActionModel(spec, sd, S, T_SEL, min_len)                   # the f32 entry point writes the same bytes
    r32 = f32(_batch(x, ids, length))
    for a, b in ((res.active, r32.active), (m.rank, f32.rank), (res.n_active, r32.n_active)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for name, (buf, fill) in guards.items():
        assert _intact(buf, fill), name
    label, logits = res.label.cpu().numpy().reshape(-1), res.logits.cpu().numpy().reshape(cap, nc)
    assert (label[~on] == -1).all() and logits[~on].tobytes() == bytes(4 * nc * int((~on).sum()))
    assert np.isfinite(logits).all() and (label[on] == logits[on].argmax(1)).all()
    # data_bn in f32 (three roundings: scale, shift, the fused multiply-add) and one rounding to half with its subnormal floor
    sc, sh = (v.reshape(18, 3) for v in AC.fold(spec, sd)["in"])
    x0 = m.x0.cpu().numpy().reshape(cap, T_SEL, 18, 4)
    xa = x.reshape(cap, 3, T_SEL, 18)[want].transpose(0, 2, 3, 1).astype(np.float64)
    ref = xa * sc + sh
    got = x0[:n, ..., :3].astype(np.float64)
    assert (np.abs(got - ref) <= SC16.H * np.abs(ref) + SC16.FLOOR + 3 * SC16.U * (np.abs(xa * sc) + np.abs(sh))).all()
    assert x0[:n, ..., 3].tobytes() == bytes(2 * n * T_SEL * 18)        # the pad channel is zero
    assert (x0[n:] == np.float16(SENT)).all()                           # nothing is written past the active clips


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
    net = SC16.network(name)
    E16, emu = net["E16"], net["emu64"]
    m = _AC().ActionModel(net["spec"], net["sd"], 1, net["T"], compute_dtype="float16")
    res = m(_network_batch(net, 1, SLOTS_USED))
    torch.cuda.synchronize()
    assert res.active[:4].tolist() == list(SLOTS_USED) + [-1] and int(res.n_active) == 3
    logits = res.logits[0, list(SLOTS_USED)].cpu().double()
    err, far = float((logits - emu).abs().max()), float((logits - net["ref64"]).abs().max())
    _record(f"{name} float16",
            f"T = {net['T']}, 3 clips, max |logit| = {float(emu.abs().max()):.4f}; E16 = max |emulation f32 - f64| = {E16:.3e}; "
            f"kernels' max |logit - emulation f64| = {err:.3e} = {err / E16:.2f} E16 (allowed: 4 E16); "
            f"max |logit - restatement f64 of the f32 model| = {far:.3e}")
    print(_lines[f"{name} float16"])
    assert err <= 4 * E16
    label = res.label[0, list(SLOTS_USED)].cpu().long()
    assert torch.equal(label, res.logits[0, list(SLOTS_USED)].cpu().argmax(1))
    decided = SC.margins(emu) > 8 * E16
    assert int((~decided).sum()) <= 0.05 * len(SLOTS_USED)
    assert torch.equal(label[decided], emu.argmax(1)[decided])
    others = [i for i in range(64) if i not in SLOTS_USED]
    assert (res.label[0, others] == -1).all() and not res.logits[0, others].any()
    assert {k: v[0] for k, v in res.to_host()[0].items()} == {100 + i: int(label[i]) for i in range(3)}


def test_logits_do_not_depend_on_the_population_or_the_place():
    net = SC16.network("tiny")
    m = _AC().ActionModel(net["spec"], net["sd"], 2, net["T"], compute_dtype="float16")
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
    assert alone.any() and torch.equal(res.logits[1, 9].view(torch.int32), alone.view(torch.int32))
    assert bool(res.logits[1].any(dim=1).all()) and len(set(res.logits[1, :, 0].tolist())) > 32


# ---- graph ----------------------------------------------------------------------------------------------------------------------
def test_a_captured_call_replays_on_any_population():
    net = SC16.network("tiny")
    AC = _AC()
    T, K = net["T"], net["spec"].K
    m, direct = (AC.ActionModel(net["spec"], net["sd"], 1, T, compute_dtype="float16") for _ in range(2))
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
    assert int(got[0][3]) == 3 and int(got[1][3]) == 42 and got[0][0].any()


# ---- network level: D-22, float32 detector, 96 x 96 --------------------------------------------------------------------------------
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
    out = {}
    for dt in ("float32", "float16"):
        pc, am = clips.PoseClips(1, 4, 36, length=6), AC.ActionModel(spec, sd, 1, 6, min_len=4, compute_dtype=dt)
        res, tracks, rows, batch, act = rt.inference_batch_actions(frames, net, track.Tracker(1, 4, 36), pc, am)
        own = AC.ActionModel(spec, sd, 1, 6, min_len=4, compute_dtype=dt)(batch)
        assert torch.equal(own.label, act.label) and torch.equal(own.logits, act.logits)
        out[dt] = (int(res.count[0]), act.active.clone(), act.n_active.clone(), act.label.clone())
    n = out["float32"][0]
    assert 0 < n <= 36 and int(out["float16"][2]) == n
    assert torch.equal(out["float16"][1], out["float32"][1]) and torch.equal(out["float16"][2], out["float32"][2])
    assert (out["float16"][3][0, :n] >= 0).all() and (out["float16"][3][0, n:] == -1).all()


# ---- the range report -------------------------------------------------------------------------------------------------------------
def test_half_range_report():
    net = SC16.network("tiny")
    m = _AC().ActionModel(net["spec"], net["sd"], 1, net["T"], compute_dtype="float16")
    batch = _network_batch(net, 1, SLOTS_USED)
    rep = m.half_range_report(batch)
    want = ["x0"] + [f"block{i}.{k}" for i in range(len(net["spec"].blocks)) for k in ("u", "out")]
    assert list(rep["tensors"]) == want and rep["finite"] is True and rep["limit"] == 65504.0
    assert all(0 < v < 65504 for v in rep["tensors"].values())
    assert torch.equal(m.logits.clone(), m(batch).logits)               # the call's result is left in place
    empty = m.half_range_report(_network_batch(net, 1, ()))
    assert empty["finite"] and not any(empty["tensors"].values())
    x = np.full((1, 64, 3, net["T"], 18), 3.0e38, np.float32)           # data_bn's output is beyond half
    ids, length = np.zeros((1, 64), np.int32), np.full((1, 64), net["T"], np.int32)
    ids[0, 7] = 1
    assert m.half_range_report(_batch(x, ids, length))["finite"] is False
