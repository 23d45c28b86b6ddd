"""GPU: the monitoring overlay (csrc/render.hip: ppn_draw_scene, ppn_draw_scene_yuv; render.Overlay, the overlay= arguments of
render.Renderer, rt.inference_batch_zones_drawn) against the NumPy restatement tests/overlay_ref.py, EVERY BYTE: each
comparison is np.array_equal on the whole buffer the frames live in -- pitch padding, the bytes behind a frame and guard
bytes around the buffer included."""
import functools
import os
import types

import numpy as np
import pytest
import torch

import overlay_cases as OC
import overlay_ref as O
import render_cases as RC
import render_yuv_ref as RY
import yuv_ref as Y

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K, E = RC.K, RC.E
GUARD, CANARY = 32, 0xC7
SHAPES = [(18, 34), (40, 260), (16, 128)]      # tests/test_render_yuv_gpu.py's: below one tile; ragged, five tile rows; two tiles
FORMATS = ("rgb",) + tuple(Y.FORMATS)


def _result(count, kp_cell, bbox):
    from pytorch_pose_proposal_network_amd.decode import DecodeResult
    kp = torch.from_numpy(np.ascontiguousarray(kp_cell, np.int32)).cuda()
    B, M, _ = kp.shape
    return DecodeResult(count=torch.from_numpy(np.asarray(count, np.int32)).cuda(), kp_cell=kp,
                        limb_arg=torch.zeros(B, M, E, dtype=torch.int32, device="cuda"),
                        bbox=torch.from_numpy(np.ascontiguousarray(bbox, np.float32)).cuda(),
                        score=torch.zeros(B, M, K, device="cuda"), max_humans=M)


def _tracks(ids):
    return None if ids is None else types.SimpleNamespace(ids=torch.from_numpy(np.ascontiguousarray(ids, np.int32)).cuda())


def _load(z, tables):
    """The case's tables, results and totals into a Zones' device buffers."""
    for n in ("zone_n", "zone_nv", "zone_xy", "line_n", "line_xy"):
        z.geom[n].copy_(torch.from_numpy(tables[n]))
    z.zone.copy_(torch.from_numpy(tables["out_zone"]))
    z.line.copy_(torch.from_numpy(tables["out_line"]))
    z.state["line_total"].copy_(torch.from_numpy(tables["line_total"]))


def _zones(case):
    from pytorch_pose_proposal_network_amd import zones
    if case["zones"] is None:
        return None
    B, M = case["people"][1].shape[:2]
    z = zones.Zones(B // case["frames"], case["frames"], M)
    _load(z, case["zones"])
    return z


def _overlay(case):
    from pytorch_pose_proposal_network_amd import render
    ov = case["overlay"]
    return render.Overlay(ov["frames"], ov["scale"], ov["tick"], ov["plates"], ov["colours"])


def _surface(rows, misalign=0):
    """Host rows u8 [F, n] -> (the whole device buffer, its expected host image builder, the [F, n] view inside it): GUARD
    canary bytes on either side."""
    F, n = rows.shape
    big = torch.full((F * n + 2 * GUARD + 8,), CANARY, dtype=torch.uint8, device="cuda")
    base = GUARD + (misalign - (big.data_ptr() + GUARD)) % 4
    view = big[base:base + F * n].view(F, n)
    view.copy_(torch.from_numpy(rows))

    def whole(expected_rows):
        host = np.full(big.numel(), CANARY, np.uint8)
        host[base:base + F * n] = expected_rows.reshape(-1)
        return host
    return big, whole, view


def _painted(case):
    """(hit, colour) of the case's scene by the restatement."""
    _, pal, order, edges, _ = RC.fixture()
    count, kp_cell, bbox = case["people"]
    g = case["grid_step"]
    return O.painted_scene(len(count), case["H"], case["W"], count, kp_cell, bbox, order, edges, pal, case["visbbox"], g > 0,
                           max(g, 1), overlay=case["overlay"], ids=case["ids"], zones=case["zones"], n_frames=case["n_frames"])


def _check(case, fmt, painted=None, extra=0, misalign=(0, 0), seed=0):
    """One case in one format, in place and out of place, against the restatement; returns (expected in place, source)."""
    from pytorch_pose_proposal_network_amd import render
    count, kp_cell, bbox = case["people"]
    B, H, W = len(count), case["H"], case["W"]
    hit, colour = _painted(case) if painted is None else painted
    res, rend = _result(count, kp_cell, bbox), render.Renderer(B, kp_cell.shape[1])
    kw = dict(overlay=_overlay(case), tracks=_tracks(case["ids"]), zones=_zones(case), n_frames=case["n_frames"])
    rng = np.random.default_rng(seed + 1000 * H + W)
    if fmt == "rgb":
        src = RC.gradient(B, H, W, seed).reshape(B, -1)
        other = rng.integers(0, 256, src.shape, dtype=np.uint8)
        exp_in = np.where(hit[..., None], colour, src.reshape(B, H, W, 3)).reshape(B, -1)
        exp_out = exp_in
        g = case["grid_step"]
        call = lambda raw, out: rend(raw.view(B, H, W, 3), res, visbbox=case["visbbox"], gridOn=g > 0, out=out.view(B, H, W, 3),
                                     outsize=(W // max(g, 1), 1), **kw)
        assert g == 0 or int(W / (W // g)) == g
    else:
        pitch = (2 * W if fmt == "yuyv" else W) + extra
        n = Y.frame_bytes(fmt, H, W, pitch)
        src, other = rng.integers(0, 256, (2, B, n + (-n) % 4 + 4), dtype=np.uint8)
        exp_in = O.scene_rows(src, src, fmt, H, W, hit, colour, pitch=pitch)
        exp_out = O.scene_rows(src, other, fmt, H, W, hit, colour, pitch=pitch)
        call = lambda raw, out: rend.draw_yuv(raw, fmt, (H, W), res, visbbox=case["visbbox"], grid_step=case["grid_step"], out=out,
                                              pitch=pitch, **kw)
    big, whole, raw = _surface(src, misalign[0])
    call(raw, raw)
    assert np.array_equal(big.cpu().numpy(), whole(exp_in)), f"{case['name']} {fmt} in place"
    call(raw, raw)
    assert np.array_equal(big.cpu().numpy(), whole(exp_in)), f"{case['name']} {fmt} drawn twice in place"
    big_s, whole_s, raw = _surface(src, misalign[0])
    big_d, whole_d, dst = _surface(other, misalign[1])
    call(raw, dst)
    assert np.array_equal(big_d.cpu().numpy(), whole_d(exp_out)), f"{case['name']} {fmt} out of place"
    assert np.array_equal(big_s.cpu().numpy(), whole_s(src)), "the source of an out-of-place call changed"
    return exp_in, src


# ---- 1. shapes and formats -------------------------------------------------------------------------------------------
GEOMETRIES = [(1, 0, 3, 1), (16, 16, 8, 4)]                     # zones, lines, vertices, scale


@functools.lru_cache(maxsize=None)
def _scene(hw, geometry):
    case = OC.scene(hw[0], hw[1], *geometry, seed=3 * SHAPES.index(hw) + GEOMETRIES.index(geometry))
    return case, _painted(case)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "%dz%dl-nv%d-s%d" % g)
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_formats_and_pitches(hw, geometry, fmt):
    """RGB takes the 12-byte stores where W % 4 == 0; a surface the word stores at the tight pitch and pitch + 8 where
    W % 4 == 0, the byte stores at pitch + 6 and from misaligned planes.  At scale 4 a glyph is 20 x 28 pixels: labels span
    tiles and are cut at the right and bottom edges."""
    case, painted = _scene(hw, geometry)
    hit = painted[0]
    assert hit[0].any() and hit[1].any()
    if fmt == "rgb":
        exp, src = _check(case, fmt, painted)
        assert (exp != src).any()
        return
    for extra, misalign in ((0, (0, 0)), (6, (0, 0)), (8, (1, 3))):
        exp, src = _check(case, fmt, painted, extra=extra, misalign=misalign, seed=extra)
        assert (exp != src).any()


def test_the_big_scenes_have_labels_over_several_tiles_and_cut_at_the_edges():
    case, _ = _scene((40, 260), GEOMETRIES[1])
    count, kp_cell, bbox = case["people"]
    texts = [m for b in range(2) for _, kind, m, _ in O.overlay_prims(b, 40, 260, 4, count, kp_cell, bbox, case["overlay"],
                                                                      case["ids"], case["zones"]) if kind.endswith("_text")]
    assert any(m[:, :128].any() and m[:, 128:].any() and m[:8].any() and m[8:].any() for m in texts)
    assert any(m[:, -1].any() for m in texts) and any(m[-1].any() for m in texts)


# ---- 2. knife edges, 3. reactive colours, running totals -------------------------------------------------------------
CASES = OC.all_cases()


@functools.lru_cache(maxsize=None)
def _painted_case(i):
    return _painted(CASES[i])


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cases(case, fmt):
    """The hand-placed cases that tests/test_overlay_cpu.py shows to paint what they claim and to tell the rules apart."""
    exp, src = _check(case, fmt, _painted_case([c["name"] for c in CASES].index(case["name"])))
    assert (exp != src).any()


def test_colours_follow_a_zone_update_on_the_device():
    """Zones.update on the device, then the drawing from its buffers, nothing read back in between: two streams x two frames;
    stream 0's person stands in zone 0 and crosses line 0 in frame 1, stream 1's second frame is not processed."""
    from pytorch_pose_proposal_network_amd import render, zones
    H, W, M = 40, 64, 2
    images = [[OC.person(10, 10, 20, 20)], [OC.person(40, 10, 50, 20)], [OC.person(10, 10, 20, 20)], [OC.person(40, 10, 50, 20)]]
    count, kp_cell, bbox = OC.pack(images, M)
    ids = np.array([[9, -1], [9, -1], [16, -1], [16, -1]], np.int32)
    res, tracks = _result(count, kp_cell, bbox), _tracks(ids)
    tracks.xy = None
    z = zones.Zones(2, 2, M, loiter=2)
    polys, segs = [[(5, 5), (30, 5), (30, 30), (5, 30)], [(35, 5), (60, 5), (60, 30), (35, 30)]], [(32, 2, 32, 38)]
    for s in range(2):
        z.set_zones(s, polys)
        z.set_lines(s, segs)
    n_frames = torch.tensor([2, 1], dtype=torch.int32, device="cuda")
    zr = z.update(res, tracks, n_frames=n_frames)
    rend, ov = render.Renderer(4, M), _overlay(dict(overlay=OC.overlay(2)))
    frames = RC.gradient(4, H, W)
    got = rend(torch.from_numpy(frames).cuda(), res, overlay=ov, tracks=tracks, zones=z, zone_result=zr, n_frames=n_frames)
    out_zone, out_line, total = zr.zone.cpu().numpy(), zr.line.cpu().numpy(), z.state["line_total"].cpu().numpy()
    assert out_zone[0, 0].tolist() == [1, 1, 0, 0] and out_zone[1, 1].tolist() == [1, 1, 0, 0] and out_zone[1, 0, 2] == 1
    assert out_line[1, 0].sum() == 1 and out_line[0, 0].sum() == 0 and not out_zone[3].any() and total[0, 0].sum() == 1
    tables = dict({n: z.geom[n].cpu().numpy() for n in z.geom}, out_zone=out_zone, out_line=out_line, line_total=total)
    _, pal, order, edges, _ = RC.fixture()
    exp = O.scene_ref(frames, count, kp_cell, bbox, order, edges, pal, overlay=OC.overlay(2), ids=ids, zones=tables,
                      n_frames=[2, 1])
    assert np.array_equal(got.cpu().numpy(), exp)
    col = lambda name: (exp == np.array(OC.COLOURS[name], np.uint8)).all(-1)
    assert col("active")[0].any() and col("active")[1].any() and not col("active")[3].any()
    assert np.array_equal(exp[3], RC.ref_draw(frames, count, kp_cell, bbox)[3])            # not processed: people only
    # the label of line 0 reads 0:0 on frame 0 and the crossing on frame 1
    f, bk = (int(v) for v in total[0, 0])
    text = (exp == np.array(OC.COLOURS["text"], np.uint8)).all(-1)
    assert (text[0] & O.text_mask(H, W, 35, 23, 1, O.codes_of("0:0"))).sum() == O.text_mask(H, W, 35, 23, 1, O.codes_of("0:0")).sum()
    assert (text[1] & O.text_mask(H, W, 35, 23, 1, O.codes_of(f"{f}:{bk}"))).sum() == \
        O.text_mask(H, W, 35, 23, 1, O.codes_of(f"{f}:{bk}")).sum()
    # the Zones' own buffers are the default zone_result
    again = rend(torch.from_numpy(frames).cuda(), res, overlay=ov, tracks=tracks, zones=z, n_frames=[2, 1])
    assert torch.equal(again, got)


# ---- 4. no-overlay equivalence ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_without_an_overlay_or_without_parts_the_bytes_are_the_people_only_ones(fmt):
    from pytorch_pose_proposal_network_amd import render
    H, W = 40, 260
    count, kp_cell, bbox = RC.people(np.random.default_rng(31), 3, 4, H, W, garbage=True)
    res, rend = _result(count, kp_cell, bbox), render.Renderer(3, 4)
    ov = render.Overlay(frames=3, scale=2, colours=OC.COLOURS)
    if fmt == "rgb":
        src = torch.from_numpy(RC.gradient(3, H, W)).cuda()
        plain = render.draw_people(src, res, visbbox=True, gridOn=True, outsize=(26, 1))
        exp = RC.ref_draw(RC.gradient(3, H, W), count, kp_cell, bbox, True, True, 10)
        draw = lambda **kw: rend(src, res, visbbox=True, gridOn=True, outsize=(26, 1), **kw)
    else:
        host = np.random.default_rng(2).integers(0, 256, (3, Y.frame_bytes(fmt, H, W) + 4), dtype=np.uint8)
        src = torch.from_numpy(host).cuda()
        plain = render.draw_people_yuv(src, fmt, (H, W), res, visbbox=True, grid_step=10)
        _, pal, order, edges, _ = RC.fixture()
        exp = RY.draw_rows(host, host, fmt, H, W, *RY.painted(3, H, W, count, kp_cell, bbox, order, edges, pal, True, 10))
        draw = lambda **kw: rend.draw_yuv(src, fmt, (H, W), res, visbbox=True, grid_step=10, **kw)
    assert np.array_equal(plain.cpu().numpy(), exp)
    assert torch.equal(draw(), plain) and torch.equal(draw(overlay=None), plain)
    assert torch.equal(draw(overlay=ov), plain) and torch.equal(draw(overlay=ov, n_frames=[3]), plain)
    for bad in (dict(tracks=_tracks(np.ones((3, 4), np.int32))), dict(n_frames=[3]),
                dict(overlay=render.Overlay(frames=2)), dict(overlay=ov, tracks=_tracks(np.ones((3, 5), np.int32))),
                dict(overlay=ov, n_frames=[3, 3]), dict(overlay=ov, zone_result=types.SimpleNamespace())):
        with pytest.raises(ValueError):
            draw(**bad)


# ---- 6. graph capture ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb", "nv12"])
def test_under_graph_capture(fmt):
    from pytorch_pose_proposal_network_amd import render
    H, W = 40, 260
    scenes = [OC.scene(H, W, 16, 16, 8, 2, seed=s) for s in (40, 44)]                       # same flags: no visbbox, no grid
    assert all(not c["visbbox"] and c["grid_step"] == 0 for c in scenes)
    first = scenes[0]
    staged, tracks, z = _result(*first["people"]), _tracks(first["ids"]), _zones(first)
    if fmt == "rgb":
        sources = [RC.gradient(2, H, W, s).reshape(2, -1) for s in (0, 1)]
        draw = lambda raw, out: rend(raw.view(2, H, W, 3), staged, out=out.view(2, H, W, 3), overlay=ov, tracks=tracks, zones=z)
    else:
        sources = [np.random.default_rng(s).integers(0, 256, (2, Y.frame_bytes(fmt, H, W)), dtype=np.uint8) for s in (0, 1)]
        draw = lambda raw, out: rend.draw_yuv(raw, fmt, (H, W), staged, out=out, overlay=ov, tracks=tracks, zones=z)
    raw = torch.from_numpy(sources[0]).cuda()
    out, inplace = torch.empty_like(raw), torch.empty_like(raw)
    rend, ov = render.Renderer(2, 4), _overlay(first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # the module is loaded outside the capture
        draw(raw, out)
        draw(out, out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        draw(raw, out)
        inplace.copy_(raw)
        draw(inplace, inplace)
    for case, src in zip(scenes, sources):
        out.fill_(CANARY)
        raw.copy_(torch.from_numpy(src))
        count, kp_cell, bbox = case["people"]
        for t, v in ((staged.count, count), (staged.kp_cell, kp_cell), (staged.bbox, bbox), (tracks.ids, case["ids"])):
            t.copy_(torch.from_numpy(np.ascontiguousarray(v)))
        _load(z, case["zones"])
        g.replay()
        torch.cuda.synchronize()
        hit, colour = _painted(case)
        if fmt == "rgb":
            exp = np.where(hit[..., None], colour, src.reshape(2, H, W, 3)).reshape(2, -1)
        else:
            exp = O.scene_rows(src, src, fmt, H, W, hit, colour)
        assert np.array_equal(out.cpu().numpy(), exp) and np.array_equal(inplace.cpu().numpy(), exp)
        assert (exp != src).any()


# ---- 7. network level: D-22, float32, 96 x 96 ------------------------------------------------------------------------
def test_inference_batch_zones_drawn_paints_what_it_found():
    from pytorch_pose_proposal_network_amd import drn, model, prng, render, rt, synth, track, zones
    g = np.load(os.path.join(GOLDEN, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    m = model.PoseProposalNet(drn.drn_d_22(), insize=(96, 96), outsize=(6, 6), compute_dtype="float32").cuda()
    m.load_state_dict(synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats))
    m.eval()
    host = np.repeat(prng.u8_frames(515, 1, (96, 96)), 4, 0)
    frames = torch.from_numpy(host).cuda()

    def make():
        z = zones.Zones(2, 2, 36, loiter=2)
        for s in range(2):
            z.set_zones(s, [[(0, 0), (95, 0), (95, 95), (0, 95)], [(4, 4), (48, 8), (44, 90), (8, 80), (20, 40)]])
            z.set_lines(s, [(48, 0, 48, 95), (0, 60, 95, 30)])
        return z

    plain = rt.inference_batch_zones(frames, m, track.Tracker(2, 2, 36), make())
    z = make()
    ov = _overlay(dict(overlay=OC.overlay(2)))
    res, tracks, zr, drawn = rt.inference_batch_zones_drawn(frames, m, track.Tracker(2, 2, 36), z, ov)
    assert torch.equal(res.count, plain[0].count) and torch.equal(tracks.ids, plain[1].ids) and torch.equal(zr.zone, plain[2].zone)
    assert drawn.shape == frames.shape and drawn.data_ptr() != frames.data_ptr() and np.array_equal(frames.cpu().numpy(), host)
    count, kp_cell, bbox, ids = (t.cpu().numpy() for t in (res.count, res.kp_cell, res.bbox, tracks.ids))
    assert int(count.sum()) > 0 and (ids > 0).any() and int(zr.zone[:, 0, 0].sum()) > 0
    tables = dict({n: z.geom[n].cpu().numpy() for n in z.geom}, out_zone=zr.zone.cpu().numpy(), out_line=zr.line.cpu().numpy(),
                  line_total=z.state["line_total"].cpu().numpy())
    _, pal, order, edges, _ = RC.fixture()
    exp = O.scene_ref(host, count, kp_cell, bbox, order, edges, pal, overlay=OC.overlay(2), ids=ids, zones=tables)
    assert np.array_equal(drawn.cpu().numpy(), exp)
    people_only = RC.ref_draw(host, count, kp_cell, bbox)
    assert (exp != people_only).any() and (exp == np.array(OC.COLOURS["alert"], np.uint8)).all(-1)[1].any()
    # in place, with the default overlay
    res, tracks, zr, same = rt.inference_batch_zones_drawn(frames, m, track.Tracker(2, 2, 36), make(), out=frames)
    assert same is frames and (frames.cpu().numpy() != host).any()


def test_inference_windows_drawn_with_an_overlay_in_frame_pixels():
    from pytorch_pose_proposal_network_amd import drn, model, rt, synth, track, windows as Wn, zones
    g = np.load(os.path.join(GOLDEN, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    m = model.PoseProposalNet(drn.drn_d_22(), insize=(96, 96), outsize=(6, 6), compute_dtype="float32").cuda()
    m.load_state_dict(synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats))
    m.eval()
    h, w, F_, M = 144, 208, 2, 4 * 36
    host = np.random.default_rng(700).integers(0, 256, (F_, Y.frame_bytes("nv12", h, w)), dtype=np.uint8)
    raw = torch.from_numpy(host).cuda()
    lay = Wn.WindowLayout.tiles((h, w), 2, 2)
    z = zones.Zones(F_, 1, M)
    for s in range(F_):
        z.set_zones(s, [[(10, 10), (200, 12), (190, 130), (20, 120)]])
        z.set_lines(s, [(104, 0, 104, 143)])
    ov = _overlay(dict(overlay=OC.overlay(1, 2)))
    plain, people_only = rt.inference_windows_drawn(raw, "nv12", (h, w), m, lay, size=96)
    res, drawn, tracks, zr = rt.inference_windows_drawn(raw, "nv12", (h, w), m, lay, size=96, overlay=ov,
                                                        tracker=track.Tracker(F_, 1, M), zones=z)
    assert torch.equal(res.count, plain.count) and np.array_equal(raw.cpu().numpy(), host)
    count, kp_cell, bbox, ids = (t.cpu().numpy() for t in (res.count, res.kp_cell, res.bbox, tracks.ids))
    assert int(count.sum()) > 0 and (ids > 0).any() and int(zr.zone[:, 0, 0].sum()) > 0
    tables = dict({n: z.geom[n].cpu().numpy() for n in z.geom}, out_zone=zr.zone.cpu().numpy(), out_line=zr.line.cpu().numpy(),
                  line_total=z.state["line_total"].cpu().numpy())
    _, pal, order, edges, _ = RC.fixture()
    hit, colour = O.painted_scene(F_, h, w, count, kp_cell, bbox, order, edges, pal, overlay=OC.overlay(1, 2), ids=ids, zones=tables)
    exp = O.scene_rows(host, host, "nv12", h, w, hit, colour)
    assert np.array_equal(drawn.cpu().numpy(), exp) and (exp != people_only.cpu().numpy()).any()
    for bad in (dict(tracker=track.Tracker(F_, 1, M)), dict(overlay=ov, zones=z)):
        with pytest.raises(ValueError):
            rt.inference_windows_drawn(raw, "nv12", (h, w), m, lay, size=96, **bad)


def test_bgr_frames_take_the_overlay_with_swapped_channels():
    from pytorch_pose_proposal_network_amd import render
    case = OC.reactive()[0]
    count, kp_cell, bbox = case["people"]
    B, H, W = len(count), case["H"], case["W"]
    rgb = RC.gradient(B, H, W)
    bgr = torch.from_numpy(np.ascontiguousarray(rgb[..., ::-1])).cuda()
    hit, colour = _painted(case)
    got = render.Renderer(B, kp_cell.shape[1]).draw_yuv(bgr.view(B, -1), "bgr", (H, W), _result(count, kp_cell, bbox),
                                                        overlay=_overlay(case), tracks=_tracks(case["ids"]), zones=_zones(case))
    assert np.array_equal(got.view(B, H, W, 3).cpu().numpy()[..., ::-1], np.where(hit[..., None], colour, rgb))
