"""GPU: low-latency plans (PoseProposalNet(latency=True)): the launches too small to fill the GPU run as split-K pairs
(csrc/conv_splitk.hip) from one plan-owned workspace.  Same accuracy gates as the ordinary plans, bit-exact graph replay,
workspace reuse and batch independence; latency=False is today's plan."""
import os

import numpy as np
import pytest
import torch

from pytorch_pose_proposal_network_amd import prng, synth
from test_16bit_floors_gpu import CONFIGS, HEAD_FLOORS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32_TOL = 1e-4                                                   # tests/test_forward_gpu.py


def _golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def _sd(g):
    return synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats={k[3:]: g[k] for k in g.files if k.startswith("bn/")})


def _net(sd, size, **kw):
    from pytorch_pose_proposal_network_amd import model
    net = model.PoseProposalNet("drn_d_22", insize=(size, size), outsize=(size // 16, size // 16), **kw).cuda()
    net.load_state_dict(sd)
    return net.eval()


def _frames(g):
    size, batch = int(g["size"]), int(g["batch"])
    return torch.from_numpy(prng.u8_frames(int(g["seed_in"]), batch, (size, size))).cuda()


def _split_launches(net, u8):
    return [(n, k) for n, k, _, _ in net.profile_layers(u8, src_is_u8=True) if "conv_splitk" in k]


@pytest.fixture(scope="module")
def d22_384():
    g = _golden("forward_d22_384")
    return g, _sd(g), _frames(g)


def test_f32_latency_plan_96():
    g = _golden("forward_d22_96")
    net = _net(_sd(g), 96, compute_dtype="float32", latency=True)
    u8 = _frames(g)[:1]
    head = net.forward_u8(u8).cpu().numpy()
    noise = float(g["ref_f32_noise"])
    err, err64 = np.abs(head - g["head"][:1]).max(), np.abs(head - g["head_f64"][:1]).max()
    print(f"96: |hip-ref| {err:.3e} |hip-f64| {err64:.3e} |ref-f64| {noise:.3e}")
    assert err <= F32_TOL or err64 <= 1.5 * noise, (err, err64, noise)
    assert _split_launches(net, u8)


def test_f32_latency_plan_384(d22_384):
    g, sd, u8 = d22_384
    net = _net(sd, 384, compute_dtype="float32", latency=True)
    head = net.forward_u8(u8[:1]).cpu().numpy()
    assert head.shape == (1, 7605, 24, 24)
    idx = g["head_idx"]
    first = idx < head.size                                      # the fixture's samples that fall into image 0
    assert first.sum() > 1000
    err = np.abs(head.reshape(-1)[idx[first]] - g["head_val"][first]).max()
    print(f"384: |hip-ref| {err:.3e} over {int(first.sum())} samples")
    assert err <= F32_TOL, err
    names = _split_launches(net, u8[:1])
    print(names)
    assert len(names) >= 1


@pytest.mark.parametrize("cfg_name", ["bf16_default", "float16"])
def test_16bit_latency_plans_meet_the_head_floors(d22_384, cfg_name):
    g, sd, u8 = d22_384
    net = _net(sd, 384, latency=True, **CONFIGS[cfg_name])
    head = np.concatenate([net.forward_u8(u8[i:i + 1]).cpu().numpy() for i in range(u8.shape[0])])
    d = np.abs(head.reshape(-1)[g["head_idx"]] - g["head_val"])
    mx, mean = HEAD_FLOORS[cfg_name]
    print(f"{cfg_name} latency: |HIP - reference head| max {d.max():.4f} (<= {mx}) mean {d.mean():.5f} (<= {mean})")
    assert d.max() <= mx and d.mean() <= mean
    assert _split_launches(net, u8[:1])


@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
def test_replay_reuse_and_batch_independence(d22_384, dtype):
    """Frames A, B, A through ONE latency plan: direct launches first, the captured graph from the third run on.  Every
    result equals a fresh plan's, so the shared workspace carries nothing from launch to launch or frame to frame; and
    a batch-2 plan gives each image the bits it gets alone."""
    _, sd, u8 = d22_384
    net = _net(sd, 384, compute_dtype=dtype, latency=True)
    a, b = u8[:1], u8[1:2]
    want = {}
    for name, f in (("a", a), ("b", b)):
        want[name] = _net(sd, 384, compute_dtype=dtype, latency=True).forward_u8(f).clone()
    st = torch.cuda.Stream()                                      # the legacy default stream cannot be captured
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        got = [net.forward_u8(f).clone() for f in (a, b, a, b, a)]    # runs 0, 1 direct; 2.. replay the graph
    torch.cuda.synchronize()
    assert net.graph_captures()[(1, 384, 384, True, False, 0)] == 1
    for i, (h, name) in enumerate(zip(got, "ababa")):
        assert torch.equal(h, want[name]), f"run {i} (frame {name}) differs from a fresh plan's"
    both = net.forward_u8(u8[:2])
    assert _split_launches(net, u8[:2])
    assert torch.equal(both[0], want["a"][0]) and torch.equal(both[1], want["b"][0])


def test_latency_false_is_todays_plan(d22_384):
    _, sd, u8 = d22_384
    off = _net(sd, 384, compute_dtype="bfloat16", latency=False)
    absent = _net(sd, 384, compute_dtype="bfloat16")
    assert absent.latency is False
    h0, h1 = off.forward_u8(u8[:1]).clone(), absent.forward_u8(u8[:1]).clone()
    assert torch.equal(h0, h1)
    assert not _split_launches(off, u8[:1]) and not _split_launches(absent, u8[:1])
    assert off._get_plan(1, 384, 384, True).workspace is None
    k0 = [k for _, k, _, _ in off.profile_layers(u8[:1], src_is_u8=True)]
    k1 = [k for _, k, _, _ in absent.profile_layers(u8[:1], src_is_u8=True)]
    assert k0 == k1
