"""GPU: ppn_tta_merge / ppn_tta_stage held bit for bit to tests/tta_ref.py (which tests/test_tta_cpu.py pins to the target
encoder), the merged pair through the fused decode, and the flip_tta option of the rt entry points and the Validator.
Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

import tta_ref as R
from pytorch_pose_proposal_network_amd import prng, synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# PPN_TTA_SPLIT: None = the host's own choice; 1 = one workgroup per window (plain key stores); 2, 3 = slices that do not
# divide the small windows evenly; 99 = more slices than some windows have rows (clamped to one row per slice)
SPLITS = (None, 1, 2, 3, 99)
SMALL = {"odd": R.ODD, "even": R.EVEN, "vector": R.VECTOR, "groups": R.GROUPS, "wide": R.WIDE}
DECODABLE = {k: v for k, v in SMALL.items() if k != "wide"}


def _merger(shape):
    from pytorch_pose_proposal_network_amd import tta
    B, H, W, sH, sW = shape
    return tta.FlipMerger(B, (H, W), (sW, sH))


def _decoder(shape):
    from pytorch_pose_proposal_network_amd import decode
    B, H, W, sH, sW = shape
    return decode.Decoder(B, (H, W), (16 * H, 16 * W), (sW, sH))


def _pair(a, b):
    return torch.from_numpy(np.concatenate([a, b], 0)).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _same_bytes(got, exp, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    assert got.tobytes() == exp.tobytes(), (what, int((got.view(np.uint32) != exp.view(np.uint32)).sum()), "words differ")


def _split_env(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("PPN_TTA_SPLIT", raising=False)
    else:
        monkeypatch.setenv("PPN_TTA_SPLIT", str(split))


def _check_merge(monkeypatch, shape, pair, splits):
    B, H, W, sH, sW = shape
    a, b = pair
    unary, keys, head = R.merge_ref(a, b, sH, sW)
    dev = _pair(a, b)
    mg = _merger(shape)
    for split in splits:
        _split_env(monkeypatch, split)
        for want_head in (False, True):
            mg.unary.fill_(-3.0); mg.keys.fill_(-1)                 # stale contents must not survive
            if mg.head is not None:
                mg.head.fill_(-3.0)
            out = mg.merge(dev, want_head=want_head)
            assert len(out) == (3 if want_head else 2)
            _same_bytes(out[0], unary, ("unary", split, want_head))
            assert np.array_equal(_u64(out[1]), keys), ("keys", split, want_head, int((_u64(out[1]) != keys).sum()))
            if want_head:
                _same_bytes(out[2], head, ("head", split))
                first = [t.clone() for t in out]
                again = mg.merge(dev, want_head=True)               # a second run: identical bytes
                assert all(torch.equal(x, y) for x, y in zip(first, again))
    assert torch.equal(dev, _pair(a, b))                            # the inputs are read only


@pytest.mark.parametrize("gen", ["dyadic", "uniform"])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_merge_matches_the_oracle(monkeypatch, name, gen):
    shape = SMALL[name]
    pair = R.dyadic_pair(3, shape) if gen == "dyadic" else R.uniform_pair(4, shape)
    _check_merge(monkeypatch, shape, pair, SPLITS)


def test_merge_at_the_real_geometry(monkeypatch):
    """24 x 24 cells, 21 x 21 windows, batch 2: the host's own split (15 slices) and the unsplit launch."""
    _check_merge(monkeypatch, R.REAL, R.uniform_pair(6, R.REAL), (None, 1))


@pytest.mark.parametrize("name", ["odd", "even", "vector"])
def test_ties_take_the_first_index_in_merged_order(monkeypatch, name):
    shape = SMALL[name]
    B, H, W, sH, sW = shape
    a, b = R.dyadic_pair(7, shape)
    _, keys, head = R.merge_ref(a, b, sH, sW)
    win = head[:, 6 * R.K:].reshape(B, R.E, sH * sW, H, W)
    assert ((win == win.max(2, keepdims=True)).sum(2) > 1).sum() > 50              # maxima attained at several s
    s_first = (~keys).astype(np.uint32).astype(np.int64)
    wrong = R.backwards_argmax(a, b, sH, sW)
    assert (wrong != s_first).sum() > 10                            # arg-max in Bm's own order gives other indices
    mg = _merger(shape)
    for split in SPLITS:
        _split_env(monkeypatch, split)
        got = _u64(mg.merge(_pair(a, b))[1])
        assert np.array_equal((~got).astype(np.uint32).astype(np.int64), s_first), split


def _assert_results_equal(got, exp, tag):
    assert len(got) == len(exp)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert int(g["n"]) == int(e["n"]), (tag, i, g["n"], e["n"])
        for k in ("root_cell", "kp_cell", "limb_arg", "bbox", "score"):
            ga, ea = np.asarray(g[k]), np.asarray(e[k])
            assert ga.shape == ea.shape and ga.tobytes() == ea.tobytes(), (tag, i, k)


@pytest.mark.parametrize("gen", ["dyadic", "uniform"])
@pytest.mark.parametrize("name", sorted(DECODABLE))
def test_decode_of_the_merged_pair(name, gen):
    from oracle import decode_ref as D
    shape = DECODABLE[name]
    B, H, W, sH, sW = shape
    a, b = R.dyadic_pair(8, shape) if gen == "dyadic" else R.uniform_pair(9, shape)
    head = R.merge_ref(a, b, sH, sW)[2]
    mg, dec = _merger(shape), _decoder(shape)
    unary, keys, merged = mg.merge(_pair(a, b), want_head=True)
    fused = dec.decode_fused(unary, keys).to_host()
    plain = dec(merged).to_host()
    ref = [D.decode_ref(head[i], insize=(16 * W, 16 * H), local_grid=(sW, sH)) for i in range(B)]
    _assert_results_equal(fused, plain, "fused vs materialised")
    _assert_results_equal(fused, ref, "fused vs decode_ref")


def test_stage_doubles_the_batch():
    mg = _merger(R.ODD)
    rng = np.random.default_rng(12)
    u8 = torch.from_numpy(rng.integers(0, 256, size=(2, 5, 7, 3), dtype=np.uint8)).cuda()
    f32 = torch.from_numpy(rng.standard_normal((2, 3, 5, 7)).astype(np.float32)).cuda()
    for x, axis in ((u8, 2), (f32, 3)):
        keep = x.clone()
        exp = torch.cat([x, x.flip(axis)])
        assert torch.equal(mg.stage(x), exp)
        out = torch.full_like(exp, 7)
        assert mg.stage(x, out=out) is out and torch.equal(out, exp)
        assert torch.equal(out[:2], keep) and torch.equal(x, keep)
    with pytest.raises(ValueError):
        mg.stage(u8, out=torch.empty(2, 5, 7, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        mg.stage(f32.double())


def test_planted_people_survive_the_merge():
    """A = planted(P), Bm = planted(mirror P): the merged pair decodes to what A alone decodes to."""
    from oracle import decode_ref as D
    people = R.people_in_distinct_cells()
    a = R.planted(people)[None]
    bm = R.planted([R.mirror_person(p) for p in people])[None]
    shape = (1, 24, 24, 21, 21)
    mg, dec = _merger(shape), _decoder(shape)
    fused = dec.decode_fused(*mg.merge(_pair(a, bm))).to_host()
    alone = dec(torch.from_numpy(a).cuda()).to_host()
    assert fused[0]["n"] == 3
    _assert_results_equal(fused, alone, "merged vs A alone")
    _assert_results_equal(fused, [D.decode_ref(a[0])], "merged vs decode_ref(A)")


# ---- network level: D-22, float32, 96 x 96, batch 2 ------------------------------------------------------------------------
def _state_dict():
    g = np.load(os.path.join(GOLDEN, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    return synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats)


def test_flip_tta_through_the_network():
    from pytorch_pose_proposal_network_amd import decode, drn, model, rt, tta
    m = model.PoseProposalNet(drn.drn_d_22(), insize=(96, 96), outsize=(6, 6), compute_dtype="float32").cuda()
    m.load_state_dict(_state_dict())
    m.eval()
    frames = torch.from_numpy(prng.u8_frames(515, 2, (96, 96))).cuda()
    mg = tta.FlipMerger(2, (6, 6), (21, 21))
    dec = decode.Decoder(2, (6, 6), (96, 96), (21, 21))

    before = [{k: np.copy(v) for k, v in r.items()} for r in rt.inference_batch(frames, m).to_host()]
    buf = m.input_buffer(4, 96, 96)
    pair = mg.stage(frames, out=buf)
    assert pair.data_ptr() == buf.data_ptr()
    head_pair = m.forward_u8(pair).clone()
    _same_bytes(head_pair[:2], m.forward_u8(frames).cpu().numpy(), "first half vs the frames alone")
    _same_bytes(head_pair[2:], m.forward_u8(frames.flip(2).contiguous()).cpu().numpy(), "second half vs the mirrored frames")
    manual = [{k: np.copy(v) for k, v in r.items()} for r in dec.decode_fused(*mg.merge(head_pair)).to_host()]

    got = rt.inference_batch(frames, m, flip_tta=True).to_host()
    _assert_results_equal(got, manual, "inference_batch(flip_tta=True) vs the manual composition")
    got = rt.inference_batch(frames, m, decoder=dec, flip_tta=True, merger=mg).to_host()
    _assert_results_equal(got, manual, "... with a caller's Decoder and FlipMerger")
    res, drawn = rt.inference_batch_drawn(frames, m, flip_tta=True)
    _assert_results_equal(res.to_host(), manual, "inference_batch_drawn(flip_tta=True)")
    assert tuple(drawn.shape) == tuple(frames.shape)
    # one frame through the reference-shaped entry point: the people of image 0
    humans, scores = rt.inference(frames[0].cpu().numpy(), m, (6, 6), (21, 21), flip_tta=True)
    assert len(humans) == manual[0]["n"]
    for i, (hm, sc) in enumerate(zip(humans, scores)):
        present = [k for k in range(18) if manual[0]["kp_cell"][i, k] >= 0]
        assert sorted(hm) == present
        for k in present:
            assert hm[k].tobytes() == manual[0]["bbox"][i, k].tobytes() and sc[k] == manual[0]["score"][i, k]
    # without the flag: today's call
    _assert_results_equal(rt.inference_batch(frames, m).to_host(), before, "flip_tta off")
    _assert_results_equal(rt.inference_batch(frames, m, flip_tta=False).to_host(),
                          dec.decode_fused(*m.forward_u8(frames, fused_decode=True)).to_host(), "flip_tta=False")


def _gt_from(results):
    """Ground truth planted on the decoded people: the box centres as joints, the root box as the head box."""
    kps, boxes = [], []
    for r in results:
        n = int(r["n"])
        bb = r["bbox"][:n]
        xy = np.stack([(bb[:, 1:, 1] + bb[:, 1:, 3]) / 2, (bb[:, 1:, 0] + bb[:, 1:, 2]) / 2], -1).astype(np.float32)
        kps.append(xy.reshape(n, 17, 2))
        boxes.append([((b[0, 1] + b[0, 3]) / 2, (b[0, 0] + b[0, 2]) / 2, b[0, 3] - b[0, 1], b[0, 2] - b[0, 0]) for b in bb])
    return kps, boxes


def test_validator_with_flip_tta():
    from pytorch_pose_proposal_network_amd import lib as L, tta, validate
    from pytorch_pose_proposal_network_amd.trainer import PPNTrainer
    from oracle import forward_ref as Fr, targets_ref as Tg
    tr = PPNTrainer("drn_d_22", _state_dict(), compute_dtype=L.PPN_F32, insize=(96, 96))
    net = tr._eval_net()
    x = torch.as_tensor(Fr.normalize_u8(prng.u8_frames(40, 2, (96, 96)))).cuda()
    tg = {k: torch.from_numpy(v).cuda() for k, v in Tg.synthetic_batch(60, 2, insize=(96, 96), outsize=(6, 6)).items()}
    M = 36

    # the manual composition: doubled batch, forward, merge, fused decode, match
    mg = tta.FlipMerger(2, (6, 6), (21, 21))
    dec = validate.D.Decoder(2, (6, 6), (96, 96), (21, 21), max_humans=M)
    head_pair = net(mg.stage(x)).clone()
    result = dec.decode_fused(*mg.merge(head_pair))
    people = result.to_host()
    assert sum(int(r["n"]) for r in people) > 0
    gt = validate.GroundTruth(*_gt_from(people))
    index = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    exp = validate.match_people(result, gt, index, validate.Records(2, M)).to_host()
    assert exp[3] == 0 and exp[1].any()                                     # some joints matched

    v = validate.Validator(net, gt, 2, tr.criterion, tr.task.w, max_humans=M, flip_tta=True)
    v.reset()
    v.step(x, [0, 1], tg)
    got = v.records.to_host()
    for g, e, what in zip(got[:3], exp[:3], ("score", "label", "count")):
        assert g.tobytes() == e.tobytes(), what
    assert got[3] == 0
    loss_tta, _ = v.finish()

    v0 = validate.Validator(net, gt, 2, tr.criterion, tr.task.w, max_humans=M)
    v0.reset()
    v0.step(x, [0, 1], tg)
    loss_plain, _ = v0.finish()
    assert loss_tta == loss_plain                                           # the loss stays on the plain head
    plain = v0.decoder(net(x)).to_host()
    assert any(int(p["n"]) != int(q["n"]) or not np.array_equal(p["bbox"], q["bbox"]) for p, q in zip(plain, people))
    # the trainer's wrapper passes the flag on
    loss_tr, _ = tr.validate([(x, [0, 1], tg)], gt, max_humans=M, flip_tta=True)
    assert loss_tr == loss_tta
