"""GPU: raw video frames (NV12, I420, YUYV) through ppn_ingest_yuv == tests/yuv_ref.ingest, every byte: colour conversion
(OpenCV's fixed-point rule), the resize rule of oracle/ingest_ref.py and the flip, in one launch; and the Python layers on
top (rt.ingest_yuv into the plan's input buffer, MultiLaneInference.submit_raw)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import yuv_ref as R
from pytorch_pose_proposal_network_amd import synth

pytestmark = pytest.mark.gpu


def _raw(seed, batch, nbytes):
    return np.random.default_rng(seed).integers(0, 256, (batch, nbytes), dtype=np.uint8)


def _check(raw, fmt, h, w, size_hw, pitch=None, **kw):
    """rt.ingest_yuv on `raw` u8 [B, >= frame bytes] against the reference, frame by frame."""
    from pytorch_pose_proposal_network_amd import rt
    got = rt.ingest_yuv(torch.from_numpy(raw).cuda(), fmt, (h, w), size=size_hw, pitch=pitch, **kw).cpu().numpy()
    assert got.shape == (raw.shape[0],) + tuple(size_hw) + (3,)
    for b in range(raw.shape[0]):
        exp = R.ingest(raw[b], fmt, h, w, size_hw, pitch, kw.get("matrix", "bt601"), kw.get("full_range", False),
                       kw.get("flip", False))
        assert np.array_equal(got[b], exp), (fmt, b, int((got[b] != exp).sum()))
    return got


# (src w, h), (dst w, h), batch, luma pitch in PIXELS (None: tight), bytes between the frames beyond a frame
GEOMETRY = [
    ((8, 6), (4, 3), 1, None, 0),          # exact halving
    ((10, 6), (7, 5), 1, None, 0),         # general downsize, dst_w % 4 != 0: byte-store tail
    ((6, 4), (16, 12), 1, None, 0),        # upsize; the edge clamps touch the last chroma column and row
    ((16, 16), (16, 16), 1, None, 0),      # identity: the output is the converted picture
    ((48, 32), (20, 12), 3, 64, 37),       # batch 3, pitched rows, frame stride larger than the frame (and odd)
    ((2, 2), (4, 4), 1, None, 0),          # smallest legal frame
]


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("fmt", R.FORMATS)
@pytest.mark.parametrize("src,dst,batch,pitch_px,gap", GEOMETRY, ids=[f"{s[0]}x{s[1]}to{d[0]}x{d[1]}" for s, d, *_ in GEOMETRY])
def test_geometry(src, dst, batch, pitch_px, gap, fmt, flip):
    (w, h), (dw, dh) = src, dst
    # pitch = 64 bytes per luma row; a packed YUYV row of 48 pixels has 96 bytes, so there the same 64 PIXELS = 128 bytes
    pitch = None if pitch_px is None else pitch_px * (2 if fmt == "yuyv" else 1)
    raw = _raw(w * 1000 + h + len(fmt), batch, R.frame_bytes(fmt, h, w, pitch) + gap)
    got = _check(raw, fmt, h, w, (dh, dw), pitch, flip=flip)
    if src == dst and not flip:
        assert np.array_equal(got[0], R.to_rgb(raw[0], fmt, h, w, pitch))


Y_EDGES = (0, 1, 15, 16, 17, 234, 235, 236, 254, 255)


@pytest.fixture(scope="module")
def colour_frames():
    """NV12 512x512, batch 16: each frame's 256x256 chroma samples are the 65536 (U, V) pairs, and the 4 luma bytes of a
    sample over the 16 frames cycle through 64 values that contain Y_EDGES -- every pair meets every one of them."""
    ys = np.array(list(Y_EDGES) + [v for v in range(3, 256, 4) if v not in Y_EDGES][:54], dtype=np.uint8)
    assert set(Y_EDGES) <= set(ys.tolist()) and len(ys) == 64
    U, V = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    frames = []
    for b in range(16):
        Y = np.empty((512, 512), np.uint8)
        for j, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            # rotate with the pair so that neighbouring samples do not share their luma
            Y[dy::2, dx::2] = ys[(4 * b + j + U.astype(np.int64) + 3 * V.astype(np.int64)) % 64]
        frames.append(R.pack(Y, U, V, "nv12"))
    raw = np.stack(frames)
    raw.setflags(write=False)
    return raw


@pytest.mark.parametrize("matrix,full_range", [("bt601", False), ("bt709", False), ("bt601", True), ("bt709", True)])
def test_colour_every_chroma_pair_at_the_luma_edges(colour_frames, matrix, full_range):
    got = _check(colour_frames, "nv12", 512, 512, (512, 512), matrix=matrix, full_range=full_range)
    assert got.min() == 0 and got.max() == 255                         # saturation at both ends was reached
    assert np.array_equal(got[3], R.to_rgb(colour_frames[3], "nv12", 512, 512, None, matrix, full_range))


def test_misaligned_destination_takes_the_byte_stores():
    from pytorch_pose_proposal_network_amd import rt
    h, w, dh, dw, batch = 12, 20, 8, 16, 2                              # dst_w % 4 == 0: only the address decides
    raw = _raw(77, batch, R.frame_bytes("i420", h, w))
    big = torch.full((batch * dh * dw * 3 + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    base = 4 - big.data_ptr() % 4 + 1 if big.data_ptr() % 4 else 1      # data_ptr() + base is 1 mod 4
    out = big[base:base + batch * dh * dw * 3].view(batch, dh, dw, 3)
    assert out.data_ptr() % 4 == 1 and out.is_contiguous()
    res = rt.ingest_yuv(torch.from_numpy(raw).cuda(), "i420", (h, w), size=(dh, dw), out=out)
    assert res.data_ptr() == out.data_ptr()
    host = big.cpu().numpy()
    for b in range(batch):
        assert np.array_equal(out[b].cpu().numpy(), R.ingest(raw[b], "i420", h, w, (dh, dw)))
    assert (host[:base] == 0x5A).all() and (host[base + batch * dh * dw * 3:] == 0x5A).all()     # nothing beside it


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_dst_bgr_swaps_the_channels(fmt):
    from pytorch_pose_proposal_network_amd import lib as L, rt
    h, w, dh, dw = 10, 12, 7, 9
    raw = _raw(78, 1, R.frame_bytes(fmt, h, w))
    dev = torch.from_numpy(raw).cuda()
    out = torch.zeros(1, dh, dw, 3, dtype=torch.uint8, device="cuda")
    n, pitch, pitch_c, uo, vo = rt.yuv_frame_layout(fmt, (h, w))
    d = L.IngestDesc(format=R.FORMATS.index(fmt), batch=1, src_h=h, src_w=w, pitch=pitch, pitch_c=pitch_c, frame_stride=n,
                     y=dev.data_ptr(), u=None if uo is None else dev.data_ptr() + uo,
                     v=None if vo is None else dev.data_ptr() + vo, matrix=0, full_range=0, dst=out.data_ptr(), dst_h=dh,
                     dst_w=dw, flip=1, dst_bgr=1)
    L.check(L.load().ppn_ingest_yuv(C.byref(d), L.current_stream_ptr()), "ppn_ingest_yuv")
    exp = R.ingest(raw[0], fmt, h, w, (dh, dw), flip=True)
    assert np.array_equal(out[0].cpu().numpy(), exp[:, :, ::-1])


def test_decoder_surface_1080p_pitched_to_network_size():
    h, w, pitch = 1080, 1920, 2048
    _check(_raw(79, 2, R.frame_bytes("nv12", h, w, pitch)), "nv12", h, w, (384, 384), pitch)


@pytest.fixture(scope="module")
def net96(golden_dir):
    from pytorch_pose_proposal_network_amd import rt
    g = np.load(os.path.join(golden_dir, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    model, outsize, lgs = rt.network(image_size=96, state_dict=synth.make_state_dict("drn_d_22", 0, bn_stats=stats))
    return model


def test_ingest_into_the_plan_input_feeds_forward(net96):
    from pytorch_pose_proposal_network_amd import rt
    h, w = 120, 160
    raw = _raw(80, 2, R.frame_bytes("yuyv", h, w))
    exp = np.stack([R.ingest(raw[b], "yuyv", h, w, (96, 96), flip=True) for b in range(2)])
    want = net96.forward_u8(torch.from_numpy(exp).cuda()).clone()
    buf = net96.input_buffer(2, 96, 96)
    frames = rt.ingest_yuv(torch.from_numpy(raw).cuda(), "yuyv", (h, w), size=96, out=buf, flip=True)
    assert frames.data_ptr() == buf.data_ptr() and np.array_equal(frames.cpu().numpy(), exp)
    assert torch.equal(net96.forward_u8(frames), want)

    class Cap:                                      # cv2 with CAP_PROP_CONVERT_RGB = 0 hands YUYV out as [H, W, 2]
        def read(self):
            return True, raw[1].reshape(h, w, 2)

    ret, one = rt.grab_frame_raw(Cap(), "yuyv", (h, w), size=96)
    assert ret and np.array_equal(one.cpu().numpy()[0], exp[1])


def test_submit_raw_from_pinned_host_and_from_the_device_equals_submit(net96):
    from pytorch_pose_proposal_network_amd import rt
    h, w, pitch = 120, 160, 192
    raws = [_raw(90 + i, 2, R.frame_bytes("nv12", h, w, pitch)) for i in range(4)]
    refs = [np.stack([R.ingest(r[b], "nv12", h, w, (96, 96), pitch, "bt709") for b in range(2)]) for r in raws]
    pipe = rt.MultiLaneInference(net96, 2, (96, 96), lanes=2)

    def drain(submit, items, host):
        out, pending = [], []
        for it in items:
            pending.append(submit(it))
            if len(pending) == 2:                  # a lane's result is read before the lane is reused
                r = pending.pop(0)
                r.ready.synchronize()
                out.append(r.hosted.unpack() if host else r.to_host())
        for r in pending:
            r.ready.synchronize()
            out.append(r.hosted.unpack() if host else r.to_host())
        return out

    want = drain(lambda f: pipe.submit(torch.from_numpy(f).cuda()), refs, False)
    with pytest.raises(ValueError):
        pipe.submit_raw(torch.from_numpy(raws[0]), "nv12", (h, w), pitch=pitch)          # pageable host memory
    hosts = [torch.from_numpy(r).pin_memory() for r in raws]
    pinned = drain(lambda r: pipe.submit_raw(r, "nv12", (h, w), to_host=True, matrix="bt709", pitch=pitch), hosts, True)
    device = drain(lambda r: pipe.submit_raw(torch.from_numpy(r).cuda(), "nv12", (h, w), matrix="bt709", pitch=pitch),
                   raws, False)
    pipe.close()
    assert sum(x["n"] for res in want for x in res) > 0
    for got in (pinned, device):
        assert len(got) == len(want)
        for s_, p_ in zip(want, got):
            for a, b in zip(s_, p_):
                assert a["n"] == b["n"]
                for k in ("kp_cell", "limb_arg", "bbox", "score"):
                    assert np.array_equal(a[k], b[k]), k
