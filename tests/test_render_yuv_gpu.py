"""GPU: drawing onto raw video surfaces (csrc/render.hip: ppn_draw_humans_yuv; render.Renderer.draw_yuv,
rt.inference_windows_drawn) against the NumPy restatement tests/render_yuv_ref.py, EVERY BYTE: each comparison is
np.array_equal on the whole buffer a surface lives in -- pitch padding, the bytes behind a frame and the guard bytes around
the surfaces included."""
import os

import numpy as np
import pytest
import torch

import render_cases as RC
import render_yuv_cases as YC
import render_yuv_ref as R
import yuv_ref as Y

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K, E = RC.K, RC.E
GUARD, CANARY = 32, 0xC7
SHAPES = [(18, 34), (40, 260), (16, 128)]      # below one tile, W % 4 == 2; a ragged last tile column, five tile rows; two tiles


def _result(count, kp_cell, bbox):
    from pytorch_pose_proposal_network_amd.decode import DecodeResult
    kp = torch.from_numpy(np.ascontiguousarray(kp_cell, np.int32)).cuda()
    B, M, _ = kp.shape
    return DecodeResult(count=torch.from_numpy(np.asarray(count, np.int32)).cuda(), kp_cell=kp,
                        limb_arg=torch.zeros(B, M, E, dtype=torch.int32, device="cuda"),
                        bbox=torch.from_numpy(np.ascontiguousarray(bbox, np.float32)).cuda(),
                        score=torch.zeros(B, M, K, device="cuda"), max_humans=M)


def _surface(rows, misalign=0):
    """Host rows u8 [F, n] -> (the whole device buffer, its expected host image builder, the [F, n] view inside it): GUARD
    canary bytes on either side, the view's address `misalign` past a multiple of 4."""
    F, n = rows.shape
    big = torch.full((F * n + 2 * GUARD + 8,), CANARY, dtype=torch.uint8, device="cuda")
    base = GUARD + (misalign - (big.data_ptr() + GUARD)) % 4
    view = big[base:base + F * n].view(F, n)
    assert view.data_ptr() % 4 == misalign
    view.copy_(torch.from_numpy(rows))

    def whole(expected_rows):
        host = np.full(big.numel(), CANARY, np.uint8)
        host[base:base + F * n] = expected_rows.reshape(-1)
        return host
    return big, whole, view


def _check(fmt, H, W, people, visbbox=False, grid_step=0, extra=0, row_pad=5, misalign=(0, 0), matrix="bt601",
           full_range=False, palette=None, seed=0, renderer=None):
    """In place and out of place against the restatement; returns (expected in place, source rows)."""
    from pytorch_pose_proposal_network_amd import render
    count, kp_cell, bbox = people
    B = len(count)
    _, pal, order, edges, _ = RC.fixture()
    pitch = (2 * W if fmt == "yuyv" else W) + extra
    rng = np.random.default_rng(seed + 1000 * H + W)
    n = Y.frame_bytes(fmt, H, W, pitch)
    n += row_pad if row_pad % 4 else (-n) % 4 + row_pad      # row_pad % 4 == 0: rows (the frame stride) a multiple of 4
    src, other = rng.integers(0, 256, (2, B, n), dtype=np.uint8)
    hit, colour = R.painted(B, H, W, count, kp_cell, bbox, order, edges, pal if palette is None else palette, visbbox, grid_step)
    kw = dict(pitch=pitch, matrix=matrix, full_range=full_range)
    exp_in, exp_out = R.draw_rows(src, src, fmt, H, W, hit, colour, **kw), R.draw_rows(src, other, fmt, H, W, hit, colour, **kw)
    res = _result(count, kp_cell, bbox)
    rend = render.Renderer(B, kp_cell.shape[1]) if renderer is None else renderer
    call = dict(visbbox=visbbox, grid_step=grid_step, palette=palette, pitch=pitch, matrix=matrix, full_range=full_range)

    big, whole, raw = _surface(src, misalign[0])
    assert rend.draw_yuv(raw, fmt, (H, W), res, out=raw, **call) is raw
    assert np.array_equal(big.cpu().numpy(), whole(exp_in)), f"{fmt} {H}x{W} in place"

    big_s, whole_s, raw = _surface(src, misalign[0])
    big_d, whole_d, dst = _surface(other, misalign[1])
    assert rend.draw_yuv(raw, fmt, (H, W), res, out=dst, **call) is dst
    assert np.array_equal(big_d.cpu().numpy(), whole_d(exp_out)), f"{fmt} {H}x{W} out of place"
    assert np.array_equal(big_s.cpu().numpy(), whole_s(src)), "the source of an out-of-place call changed"
    return exp_in, src, hit


def _crowd(B, M, H, W, seed):
    """People over every border with missing and garbage keypoints; with B == 3 image 1 has nobody and image 2 a count above M."""
    count, kp_cell, bbox = RC.people(np.random.default_rng(seed), B, M, H, W, garbage=True)
    if B == 3:
        count[:] = [M, 0, M + 3]
    return count, kp_cell, bbox


@pytest.mark.parametrize("extra", [0, 6, 8], ids=["tight", "pitch+6", "pitch+8"])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_formats_shapes_and_pitches(fmt, hw, extra):
    """Rows of a multiple of 4 bytes on aligned buffers: tight and pitch + 8 take the word stores out of place where
    W % 4 == 0, pitch + 6 and 18 x 34 the byte stores.  No grid here: image 1 (count 0) keeps every byte."""
    H, W = hw
    i = SHAPES.index(hw)
    exp, src, hit = _check(fmt, H, W, _crowd(3, 4, H, W, 7 + i), visbbox=bool(i % 2), extra=extra, row_pad=4)
    assert np.array_equal(exp[1], src[1]) and (exp[0] != src[0]).any() and (exp[2] != src[2]).any()
    assert hit[0].any() and not hit[1].any()


@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_misaligned_planes_and_odd_strides(fmt, hw):
    """Every plane of the source 1 byte past a multiple of 4, the destination 3 bytes past one, rows of an odd length."""
    H, W = hw
    _check(fmt, H, W, _crowd(3, 4, H, W, 21), grid_step=5, extra=6, row_pad=5, misalign=(1, 3))
    _check(fmt, H, W, _crowd(3, 4, H, W, 22), visbbox=True, extra=0, row_pad=7, misalign=(1, 2))


CASES = YC.anchor_cases()


@pytest.mark.parametrize("fmt", Y.FORMATS)
@pytest.mark.parametrize("name,people,visbbox,grid_step,tells", CASES, ids=[c[0] for c in CASES])
def test_chroma_anchoring(name, people, visbbox, grid_step, tells, fmt):
    """The hand-placed cases that tests/test_render_yuv_cpu.py shows to tell the right chroma rule from top-left-only and
    last-painted anchoring."""
    exp, src, hit = _check(fmt, YC.H, YC.W, YC.pack_people(people), visbbox, grid_step)
    assert hit.any() and (exp != src).any()


@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_chunked_bin_list_chroma_follows_the_final_colours(fmt):
    """16 people x 35 slots around one tile: 560 primitives, more than the 256 entries of the bin list, so the list is
    resolved in chunks and a later chunk repaints pixels of an earlier one."""
    people = RC.people(np.random.default_rng(16), 1, 16, 24, 40, spread=(20.0, 4.0, 3.5), missing=0.0)
    assert int((people[1] >= 0).sum()) == 16 * K and 16 * (K + E) > 256
    _check(fmt, 24, 40, people)
    _check(fmt, 24, 40, people, visbbox=True)


@pytest.mark.parametrize("matrix,full", R.SETS, ids=lambda v: str(v))
@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_colour_sets_and_a_custom_palette(fmt, matrix, full):
    H, W = 24, 36
    people = _crowd(2, 3, H, W, 5)
    a, _, _ = _check(fmt, H, W, people, grid_step=8, matrix=matrix, full_range=full)
    palette = [((37 * k) % 256, (91 * k + 13) % 256, 255 - (53 * k) % 256) for k in range(K)]
    b, _, _ = _check(fmt, H, W, people, grid_step=8, matrix=matrix, full_range=full, palette=palette)
    assert (a != b).any()


@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_drawing_again_changes_nothing_and_both_modes_agree(fmt):
    from pytorch_pose_proposal_network_amd import render
    H, W = 40, 260
    count, kp_cell, bbox = _crowd(3, 4, H, W, 31)
    res = _result(count, kp_cell, bbox)
    src = YC.raw_frames(np.random.default_rng(2), fmt, 3, H, W, tail=4)
    raw = torch.from_numpy(src).cuda()
    rend = render.Renderer(3, 4)
    once = rend.draw_yuv(raw, fmt, (H, W), res, grid_step=16)                   # out=None: a new tensor
    assert once.data_ptr() != raw.data_ptr() and once.shape == raw.shape and np.array_equal(raw.cpu().numpy(), src)
    first = once.cpu().numpy()
    assert (first != src).any() and np.array_equal(first[:, -4:], src[:, -4:])
    assert rend.draw_yuv(once, fmt, (H, W), res, grid_step=16, out=once) is once
    assert np.array_equal(once.cpu().numpy(), first)                            # twice in place == once
    out = torch.full_like(raw, CANARY)
    rend.draw_yuv(raw, fmt, (H, W), res, grid_step=16, out=out)
    assert np.array_equal(out.cpu().numpy()[:, :-4], first[:, :-4]) and (out[:, -4:] == CANARY).all()
    rend.draw_yuv(out, fmt, (H, W), res, grid_step=16, out=out)                 # out of place, then in place
    assert np.array_equal(out.cpu().numpy()[:, :-4], first[:, :-4])
    one_off = render.draw_people_yuv(raw, fmt, (H, W), res, grid_step=16)
    assert np.array_equal(one_off.cpu().numpy(), first)


@pytest.mark.parametrize("fmt", Y.FORMATS)
def test_under_graph_capture(fmt):
    from pytorch_pose_proposal_network_amd import render
    H, W = 40, 260
    _, pal, order, edges, _ = RC.fixture()
    inputs = [(_crowd(3, 4, H, W, s), YC.raw_frames(np.random.default_rng(s), fmt, 3, H, W)) for s in (41, 42)]
    (count, kp_cell, bbox), src = inputs[0]
    staged, raw = _result(count, kp_cell, bbox), torch.from_numpy(src).cuda()
    out, inplace = torch.empty_like(raw), torch.empty_like(raw)
    rend = render.Renderer(3, 4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # the module is loaded outside the capture
        rend.draw_yuv(raw, fmt, (H, W), staged, out=out)
        rend.draw_yuv(out, fmt, (H, W), staged, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rend.draw_yuv(raw, fmt, (H, W), staged, visbbox=True, grid_step=16, out=out)
        inplace.copy_(raw)
        rend.draw_yuv(inplace, fmt, (H, W), staged, visbbox=True, grid_step=16, out=inplace)
    for (count, kp_cell, bbox), src in inputs:
        out.fill_(CANARY)
        raw.copy_(torch.from_numpy(src))
        for t, v in ((staged.count, count), (staged.kp_cell, kp_cell), (staged.bbox, bbox)):
            t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
        g.replay()
        torch.cuda.synchronize()
        hit, colour = R.painted(3, H, W, count, kp_cell, bbox, order, edges, pal, True, 16)
        exp = R.draw_rows(src, src, fmt, H, W, hit, colour)
        assert np.array_equal(out.cpu().numpy(), exp) and np.array_equal(inplace.cpu().numpy(), exp)
        assert (exp != src).any()


def test_bgr_goes_through_the_rgb_rasteriser_with_swapped_channels():
    from pytorch_pose_proposal_network_amd import render
    H, W = 18, 34
    count, kp_cell, bbox = _crowd(3, 4, H, W, 51)
    res = _result(count, kp_cell, bbox)
    rgb = RC.gradient(3, H, W)
    bgr = torch.from_numpy(np.ascontiguousarray(rgb[..., ::-1])).cuda()
    swapped = [tuple(c)[::-1] for c in render.default_palette()]
    for raw in (bgr.view(3, -1), bgr):
        got = render.draw_people_yuv(raw, "bgr", (H, W), res, grid_step=5)
        assert got.shape == raw.shape and got.data_ptr() != raw.data_ptr()
        exp = render.draw_people(bgr, res, gridOn=True, outsize=(W // 5, 1), palette=swapped)
        assert int(W / (W // 5)) == 5 and torch.equal(got.view(3, H, W, 3), exp)
        assert np.array_equal(got.view(3, H, W, 3).cpu().numpy()[..., ::-1], RC.ref_draw(rgb, count, kp_cell, bbox, False, True, 5))
    same = bgr.clone()
    assert render.draw_people_yuv(same, "bgr", (H, W), res, out=same) is same and (same != bgr).any()
    with pytest.raises(ValueError):
        render.draw_people_yuv(bgr.view(3, -1), "bgr", (H, W), res, pitch=3 * W + 4)
    with pytest.raises(ValueError):
        render.draw_people_yuv(torch.zeros(3, H, 3 * W + 4, dtype=torch.uint8, device="cuda")[:, :, :3 * W], "bgr", (H, W), res)


def test_wrapper_checks_its_input():
    from pytorch_pose_proposal_network_amd import render
    H, W = 16, 32
    res = _result(*_crowd(2, 3, H, W, 61))
    raw = torch.zeros(2, Y.frame_bytes("nv12", H, W), dtype=torch.uint8, device="cuda")
    rend = render.Renderer(2, 3)
    for bad in (dict(raw=raw[:, :-1]), dict(raw=raw[:1]), dict(raw=raw.cpu()), dict(raw=raw.float()), dict(fmt="p010"),
                dict(matrix="bt2020"), dict(src_hw=(15, 32)), dict(src_hw=(16, 31)), dict(grid_step=-1), dict(pitch=30),
                dict(out=torch.zeros(2, raw.shape[1] + 1, dtype=torch.uint8, device="cuda")), dict(out=raw[:, 1:]),
                dict(out=raw.view(-1)[8:8 + raw.numel() - 16].view(2, -1))):
        kw = dict(dict(raw=raw, fmt="nv12", src_hw=(H, W), result=res), **bad)
        with pytest.raises(ValueError):
            rend.draw_yuv(**kw)
    big = torch.zeros(2 * raw.shape[1] + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):                                             # overlaps raw without being raw
        rend.draw_yuv(big[:2 * raw.shape[1]].view(2, -1), "nv12", (H, W), res, out=big[8:].view(2, -1))


def test_rgb_rasteriser_still_equals_its_restatement():
    """Guard beside tests/test_render_gpu.py: the RGB kernel shares its binning and coverage code with the surface kernels."""
    from pytorch_pose_proposal_network_amd import render
    H, W = 40, 100
    count, kp_cell, bbox = _crowd(3, 4, H, W, 71)
    frames = RC.gradient(3, H, W)
    exp = RC.ref_draw(frames, count, kp_cell, bbox, True, True, 10)
    res = _result(count, kp_cell, bbox)
    src = torch.from_numpy(frames).cuda()
    out = render.draw_people(src, res, visbbox=True, gridOn=True, outsize=(10, 1))
    assert np.array_equal(out.cpu().numpy(), exp) and np.array_equal(src.cpu().numpy(), frames)
    assert render.draw_people(src, res, visbbox=True, gridOn=True, out=src, outsize=(10, 1)) is src
    assert np.array_equal(src.cpu().numpy(), exp) and (exp != frames).any()


# ---- network level: D-22, float32, 96 x 96 ---------------------------------------------------------------------------
def test_inference_windows_drawn_paints_what_it_found():
    from pytorch_pose_proposal_network_amd import drn, model, rt, synth, windows as Wn
    g = np.load(os.path.join(GOLDEN, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    m = model.PoseProposalNet(drn.drn_d_22(), insize=(96, 96), outsize=(6, 6), compute_dtype="float32").cuda()
    m.load_state_dict(synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats))
    m.eval()
    h, w, F_ = 144, 208, 2
    host = np.random.default_rng(700).integers(0, 256, (F_, Y.frame_bytes("nv12", h, w)), dtype=np.uint8)
    raw = torch.from_numpy(host).cuda()
    lay = Wn.WindowLayout.tiles((h, w), 2, 2)
    plain = rt.inference_windows(raw, "nv12", (h, w), m, lay, size=96)
    want = {k: getattr(plain, k).clone() for k in ("count", "kp_cell", "limb_arg", "bbox", "score")}
    res, drawn = rt.inference_windows_drawn(raw, "nv12", (h, w), m, lay, size=96)
    assert res.max_humans == plain.max_humans == 4 * 36
    for k, v in want.items():
        assert torch.equal(getattr(res, k).view(torch.uint8), v.view(torch.uint8)), k
    assert drawn.shape == raw.shape and drawn.data_ptr() != raw.data_ptr() and np.array_equal(raw.cpu().numpy(), host)
    _, pal, order, edges, _ = RC.fixture()
    count, kp_cell, bbox = (want[k].cpu().numpy() for k in ("count", "kp_cell", "bbox"))
    assert int(count.sum()) > 0
    hit, colour = R.painted(F_, h, w, count, kp_cell, bbox, order, edges, pal)
    exp = R.draw_rows(host, host, "nv12", h, w, hit, colour)
    assert hit.any() and (exp != host).any()
    assert np.array_equal(drawn.cpu().numpy(), exp)
    res, same = rt.inference_windows_drawn(raw, "nv12", (h, w), m, lay, size=96, out=raw, visbbox=True)
    hit, colour = R.painted(F_, h, w, count, kp_cell, bbox, order, edges, pal, visbbox=True)
    assert same is raw and np.array_equal(raw.cpu().numpy(), R.draw_rows(host, host, "nv12", h, w, hit, colour))
    with pytest.raises(ValueError):
        rt.inference_windows_drawn(raw, "nv12", (h, w), m, lay, size=96, flip=True)
