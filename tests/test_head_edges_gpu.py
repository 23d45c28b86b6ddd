"""GPU: the two arg-max code paths of the head conv on the cases of tests/head_cases.py, judged by its f64 checker (index range,
near-maximal logit, exact index on decided windows, value bound; bit for bit on the exact cases) -- not by each other.

* the edge-aligned limb kernel (csrc/conv_head.hip, ppn_conv_desc.limb_edge_pad): every listed window in both paddings, the XCD-slot
  splits, a walk of several tiles per workgroup across edge changes, pixel ranges, GEMM depths, small images, a NULL bias, ties.
  The rule for a window: a launch the route accepts gives correct keys; one it refuses returns an error and leaves the
  garbage-filled key buffer alone.  Windows 433 .. 448 must be accepted.
* the atomic-key epilogue of csrc/conv_big.hip: the same references, windows 20 .. 529, three unary counts, forced tiles, keys-only
  and materialising launches (the materialised head is checked element by element as well).
Every launch runs twice; the two runs must be bitwise equal.  Where both paths accept a case their keys are equal.
One line per case and type begins HEAD_EDGE: the worst value ratio, the undecided share, the tiles per workgroup reached."""
import numpy as np
import pytest
import torch

import head_cases as HC
from test_conv_gpu import run_conv, run_edge_argmax
from test_conv_tiles_gpu import _check_keys, force_tile  # noqa: F401  (force_tile: the fixture)

pytestmark = pytest.mark.gpu

DT = HC.DTYPE_NAMES
EDGE = [n for n, c in HC.CASES.items() if "edge" in c.paths and c.ranges is None]
RANGES = [n for n, c in HC.CASES.items() if c.ranges is not None]
ATOMIC = [(n, t) for n, c in HC.CASES.items() if "atomic" in c.paths
          for t in (HC.ATOMIC_TILES if n.startswith("atomic/") else (None,))]
MUST_ACCEPT = range(433, 449)


def _code(d):
    from pytorch_pose_proposal_network_amd import lib as L
    return {"f32": L.PPN_F32, "bf16": L.PPN_BF16, "f16": L.PPN_F16}[d]


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _edge_launch(name, d, ranges=None, operands=None):
    """(keys or None, error text or None, the key buffer as the launch left it): the edge-aligned tile on a case's operands."""
    c = HC.CASES[name]
    x, w, b = operands if operands is not None else HC.operands(name, d)
    info = {}
    try:
        keys, kn = run_edge_argmax(x, w.view(w.shape[0], -1, 1, 1), b, _code(d), c.uch, c.win,
                                   pad_bias=1000.0 if c.pad == "hostile" else 0.0, ranges=ranges, info=info)
    except RuntimeError as e:
        torch.cuda.synchronize()
        return None, str(e), info["keys"].cpu()
    assert "head_limb_argmax_kernel" in kn and info["guard_ok"], (name, d, kn)
    return keys, None, keys


def _judge(name, d, keys, what, sched=None):
    c = HC.CASES[name]
    ref = HC.reference(name, d)
    v = HC.check(c, ref, keys)
    print("HEAD_EDGE %s %s %s: value ratio %.3f, undecided %.4f%s" % (
        what, name, d, v.ratio, v.undecided,
        "" if sched is None else ", %d x %d tiles, %d workgroups, <= %d tiles per workgroup, %d empty" % (
            sched["n_ptiles"], c.E, sched["grid"], sched["max_tiles"], sched["empty"])))
    assert v.ok, (name, d, v)
    assert v.ratio <= 1.0, (name, d, v.ratio)
    if c.kind in ("random", "negative"):
        assert v.undecided <= HC.UNDECIDED_CAP, (name, d, v.undecided)
    else:
        assert HC.check_exact(c, ref, keys) is None, (name, d, HC.check_exact(c, ref, keys))


@pytest.mark.parametrize("d", DT)
@pytest.mark.parametrize("name", EDGE)
def test_edge_kernel(name, d):
    c = HC.CASES[name]
    keys, err, left = _edge_launch(name, d)
    if err is not None:
        # refused: an error, and the garbage in the key buffer untouched
        print("HEAD_EDGE edge %s %s: refused (%s)" % (name, d, err))
        assert c.win not in MUST_ACCEPT, (name, d, err)
        assert bool((left == HC.GARBAGE).all())
        return
    again, _, _ = _edge_launch(name, d)
    assert torch.equal(keys, again)
    sched = HC.schedule(HC.pixels(c), c.E, _n_cu())
    _judge(name, d, keys, "edge", sched)
    if name == "walk17":
        assert sched["max_tiles"] >= 3 and sched["edge_changes"] >= 2, sched     # fails, not skips, on a device where it does not hold
    if name in ("slots/9_exact", "slots/9_tail", "slots/7"):
        assert sched["empty"] > 0, sched


@pytest.mark.parametrize("d", DT)
@pytest.mark.parametrize("name", RANGES)
def test_edge_kernel_pixel_ranges(name, d):
    """Each launch leaves the pixels outside its range alone; the union equals the single launch bit for bit."""
    c = HC.CASES[name]
    M = HC.pixels(c)
    whole, err, _ = _edge_launch(name, d)
    assert err is None
    _judge(name, d, whole, "edge-ranges")
    flat = lambda k: k.permute(0, 2, 3, 1).reshape(M, c.E)                                             # noqa: E731
    for lo, n in c.ranges:
        part, err, _ = _edge_launch(name, d, ranges=[(lo, n)])
        assert err is None
        inside = torch.zeros(M, dtype=torch.bool)
        inside[lo: lo + n] = True
        assert torch.equal(flat(part)[inside], flat(whole)[inside])
        assert bool((flat(part)[~inside] == HC.GARBAGE).all())
    union, err, _ = _edge_launch(name, d, ranges=list(c.ranges))
    assert err is None and torch.equal(union, whole)
    again, _, _ = _edge_launch(name, d, ranges=list(c.ranges))
    assert torch.equal(union, again)
    # out of bounds: refused, nothing written
    for bad in ((M - 10, 20), (-4, 8)):
        keys, err, left = _edge_launch(name, d, ranges=[bad])
        assert keys is None and "pixel range" in err and bool((left == HC.GARBAGE).all())
    if (c.H * c.W) % 4 == 0:                                     # an NCHW launch: cuts on multiples of 4 only
        keys, err, left = _edge_launch(name, d, ranges=[(0, 387)])
        assert keys is None and "multiple of 4" in err and bool((left == HC.GARBAGE).all())


@pytest.mark.parametrize("d", DT)
def test_edge_kernel_refuses_an_odd_number_of_k_steps(d):
    c = HC.CASES["depth/2steps"]
    K = HC.ODD_DEPTH_STEPS * HC.k_step(d)
    x, w, b = HC._random_operands(c, d, K, torch.Generator().manual_seed(5))
    keys, err, left = _edge_launch("depth/2steps", d, operands=(x, w, b))
    assert keys is None and "even number of K steps" in err and bool((left == HC.GARBAGE).all())


@pytest.mark.parametrize("d", DT)
@pytest.mark.parametrize("name,tile", ATOMIC, ids=["%s-%s" % (n, "auto" if t is None else "%dx%d" % t) for n, t in ATOMIC])
def test_atomic_key_epilogue(force_tile, name, tile, d):  # noqa: F811
    c = HC.CASES[name]
    x, w, b = HC.operands(name, d)
    w4 = w.view(w.shape[0], -1, 1, 1)
    if tile is not None:
        force_tile(*tile)

    def launch(want_raw):
        info = {}
        raw, _ = run_conv(x, w4, _code(d), b1=b, act1=3, nchw=True, argmax=(c.uch, c.win), want_raw=want_raw, info=info)
        return raw, info

    try:
        raw, info = launch(True)
    except RuntimeError as e:
        # only a head too narrow for the large-tile kernel is refused (window 1: three channels)
        print("HEAD_EDGE atomic %s %s: refused (%s)" % (name, d, e))
        assert w.shape[0] < 64 and "large-tile kernel only" in str(e)
        return
    assert info["kernel"].startswith("conv_igemm_big_kernel"), info["kernel"]
    if tile is not None and w.shape[0] >= 256:
        assert "%d, %d, 8" % tile in info["kernel"], info["kernel"]
    ref = HC.reference(name, d)
    r = HC.head_ratio(c, ref, raw)
    print("HEAD_EDGE atomic-head %s %s %s: value ratio %.3f" % (name, d, info["kernel"], r))
    assert r <= 1.0
    _check_keys(info, raw, c.uch, c.win)                     # self-consistency: keys = first maximum of that head
    _judge(name, d, info["keys"], "atomic")
    raw2, info2 = launch(True)
    assert torch.equal(raw, raw2) and torch.equal(info["keys"], info2["keys"]) and torch.equal(info["unary"], info2["unary"])
    for _ in range(2):                                       # keys only, as the plans launch it
        _, only = launch(False)
        assert torch.equal(only["keys"], info["keys"]) and torch.equal(only["unary"], info["unary"])
    if "edge" in c.paths:
        keys_e, err, _ = _edge_launch(name, d)
        if err is None:
            assert torch.equal(keys_e, info["keys"])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_model_with_a_420_value_window_and_limb_scores_below_half(golden_dir, dtype):
    """PoseProposalNet with local_grid_size (21, 20) -- a 420-value limb window, 28 pad rows per edge in a 448-row tile, packed
    with zero weights and zero bias (model.py) -- and the head conv's limb biases lowered until every limb score is below 0.5: a
    pad row that competed would win every window with the value 0.5 at an index past the window."""
    import os
    from pytorch_pose_proposal_network_amd import decode, drn, model, prng, synth
    grid = (21, 20)
    win = grid[0] * grid[1]
    g = np.load(os.path.join(golden_dir, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    sd = synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats, head_channels=108 + 17 * win)
    bias = sd["conv3.bias"].copy()
    bias[108:] -= 20.0
    sd["conv3.bias"] = bias
    m = model.PoseProposalNet(drn.drn_d_22(), insize=(96, 96), outsize=(6, 6), local_grid_size=grid, compute_dtype=dtype).cuda()
    m.load_state_dict(sd)
    m.eval()
    frames = torch.from_numpy(prng.u8_frames(911, 3, (96, 96))).cuda()
    head = m.forward_u8(frames).clone()
    assert float(head[:, 108:].max()) < 0.5
    unary, keys = m.forward_u8(frames, fused_decode=True)
    assert torch.equal(unary, head[:, :108])
    e = head[:, 108:].reshape(3, 17, win, 6, 6)
    val = e.max(dim=2).values
    first = (e == val.unsqueeze(2)).to(torch.uint8).argmax(dim=2)                      # lowest index among ties
    assert torch.equal((0xFFFFFFFF - (keys & 0xFFFFFFFF)).to(torch.int64), first)
    assert torch.equal(((keys >> 32) & 0xFFFFFFFF).to(torch.int32).view(torch.float32), val)
    dec = decode.Decoder(3, (6, 6), (96, 96), grid)
    a = [{k: (v.copy() if hasattr(v, "copy") else v) for k, v in r.items()} for r in dec(head).to_host()]
    b = dec.decode_fused(unary, keys).to_host()
    for ra, rb in zip(a, b):
        assert ra["n"] == rb["n"]
        for k in ("kp_cell", "limb_arg", "bbox", "score"):
            assert np.array_equal(ra[k], rb[k]), k
