"""Drawing the decoded people on the device (csrc/render.hip, pytorch_pose_proposal_network_amd/render.py) against the frames
the reference drew (tests/golden/draw_cases.npz) and the NumPy restatement tests/render_ref.py, BIT FOR BIT: every
comparison in this file is "zero differing pixels"."""
import os

import numpy as np
import pytest
import torch

import render_cases as RC

pytestmark = pytest.mark.gpu

K, E = RC.K, RC.E


def _result(count, kp_cell, bbox):
    from pytorch_pose_proposal_network_amd.decode import DecodeResult
    kp = torch.from_numpy(np.ascontiguousarray(kp_cell, np.int32)).cuda()
    B, M, _ = kp.shape
    return DecodeResult(count=torch.from_numpy(np.asarray(count, np.int32)).cuda(), kp_cell=kp,
                        limb_arg=torch.zeros(B, M, E, dtype=torch.int32, device="cuda"),
                        bbox=torch.from_numpy(np.ascontiguousarray(bbox, np.float32)).cuda(),
                        score=torch.zeros(B, M, K, device="cuda"), max_humans=M)


def _draw_both(frames, count, kp_cell, bbox, visbbox=False, grid=False, grid_step=16):
    """(out-of-place result, in-place result) as NumPy arrays; the source of the out-of-place call must stay untouched."""
    from pytorch_pose_proposal_network_amd import render
    res = _result(count, kp_cell, bbox)
    W = frames.shape[2]
    outsize = (W // grid_step, 1)                       # int(W / outW) == grid_step for the steps used here
    assert not grid or int(W / outsize[0]) == grid_step
    src = torch.from_numpy(frames).cuda()
    out = render.draw_people(src, res, visbbox=visbbox, gridOn=grid, outsize=outsize)
    assert out.data_ptr() != src.data_ptr() and np.array_equal(src.cpu().numpy(), frames)
    inplace = src.clone()
    same = render.draw_people(inplace, res, visbbox=visbbox, gridOn=grid, out=inplace, outsize=outsize)
    assert same.data_ptr() == inplace.data_ptr()
    return out.cpu().numpy(), inplace.cpu().numpy()


def _check(frames, count, kp_cell, bbox, visbbox=False, grid=False, grid_step=16, expected=None, what=""):
    if expected is None:
        expected = RC.ref_draw(frames, count, kp_cell, bbox, visbbox, grid, grid_step)
    for name, got in zip(("out of place", "in place"), _draw_both(frames, count, kp_cell, bbox, visbbox, grid, grid_step)):
        diff = int((got != expected).any(-1).sum())
        assert diff == 0, f"{what} {name}: {diff} pixels differ"
    return expected


def test_every_fixture_case_in_place_and_out_of_place():
    cases = RC.fixture()[0]
    for c in cases:
        exp = _check(c["base"][None], [c["count"]], c["kp_cell"][None], c["bbox"][None], c["visbbox"], c["grid"],
                     c["grid_step"], expected=c["expected"][None], what=c["name"])
        untouched = (exp == c["base"][None]).all(-1)
        assert untouched.any() and np.array_equal(exp[untouched], c["base"][None][untouched])


def test_counts_are_clamped_and_absent_slots_ignored():
    rng = np.random.default_rng(11)
    frames = RC.gradient(4, 48, 64)
    count, kp_cell, bbox = RC.people(rng, 4, 3, 48, 64, garbage=True)       # kp_cell < 0 slots hold NaN / inf / huge boxes
    count[:] = [0, 7, -2, 2]                                                # nobody; more than max_humans; negative; two
    exp = _check(frames, count, kp_cell, bbox, what="counts")
    assert np.array_equal(exp[0], frames[0]) and np.array_equal(exp[2], frames[2])
    assert np.array_equal(exp[1], RC.ref_draw(frames[1:2], [3], kp_cell[1:2], bbox[1:2])[0])
    assert (exp[3] != frames[3]).any()


@pytest.mark.parametrize("hw", [(70, 100), (33, 47), (9, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("visbbox", [False, True], ids=["discs", "boxes"])
def test_frames_off_the_tile_grid(hw, visbbox):
    """Neither size is a multiple of the 8-row tile; 100 takes the 12-byte store path out of place, 47 and 130 the byte
    path; people reach over every border and every tile seam."""
    H, W = hw
    rng = np.random.default_rng(H * 1000 + W)
    count, kp_cell, bbox = RC.people(rng, 2, 4, H, W, missing=0.1)
    _check(RC.gradient(2, H, W), count, kp_cell, bbox, visbbox, grid=True, grid_step=7 if W != 100 else 10, what=f"{hw}")


def test_ties_at_the_four_edges_of_the_frame():
    """Disc centres and line ends at quarter-pixel steps around each edge and corner (truncation toward zero and the
    symmetric rounding of the scan line change behaviour at 0), and limbs that run along and across the borders."""
    H, W = 40, 52
    offs = [-2.5, -2.0, -0.75, -0.25, 0.0, 0.25, 0.5, 1.75, 2.0]
    pts = [(x, y) for x in (0.0, W - 1.0, W / 2) for y in (0.0, H - 1.0, H / 2) if (x, y) != (W / 2, H / 2)]
    neck, thorax = 15, 13
    people = []
    for (px, py) in pts:
        for o in offs:
            hm = {0: RC.box(W / 2, H / 2, 6, 6), neck: RC.box(px + o, py + o / 2, 3, 3),
                  thorax: RC.box(W / 2 + o, H / 2 - o, 2, 2)}
            people.append(hm)
    M = len(people)
    kp_cell = np.full((1, M, K), -1, np.int32)
    bbox = np.zeros((1, M, K, 4), np.float32)
    for i, hm in enumerate(people):
        for k, b in hm.items():
            kp_cell[0, i, k], bbox[0, i, k] = 1, b
    _check(RC.gradient(1, H, W), [M], kp_cell, bbox, what="edges")


def test_bin_pressure_many_people_on_one_tile():
    """A 6 x 6 grid's max_humans = 36 people, every keypoint present, all within one tile's reach: 36 * 35 = 1260
    primitives against one 8-row tile, five times the LDS list.  A capped or reordered list shows up here."""
    rng = np.random.default_rng(36)
    count, kp_cell, bbox = RC.people(rng, 2, 36, 96, 96, spread=(50.0, 44.0, 9.0), missing=0.0)
    assert int((kp_cell >= 0).sum()) == 2 * 36 * K
    _check(RC.gradient(2, 96, 96), count, kp_cell, bbox, what="bin pressure")
    _check(RC.gradient(2, 96, 96), count, kp_cell, bbox, visbbox=True, what="bin pressure, boxes")


def test_non_finite_and_huge_coordinates_are_skipped():
    rng = np.random.default_rng(3)
    frames = RC.gradient(2, 64, 64)
    count, kp_cell, bbox = RC.people(rng, 2, 4, 64, 64, missing=0.0)
    clean = RC.ref_draw(frames, count, kp_cell, bbox)
    poison = np.array([np.nan, np.inf, -np.inf, 2.0 ** 20, -2.0 ** 20, 3e38, -1e30], np.float32)
    hit = rng.random(bbox.shape) < 0.08                                      # present keypoints with one bad coordinate
    bbox[hit] = rng.choice(poison, int(hit.sum()))
    bbox[0, 0, 0] = [1.0, 2.0, 2.0 ** 20 - 1, 2.0 ** 20 - 1]                 # just inside the limit: drawn (and clipped)
    exp = _check(frames, count, kp_cell, bbox, what="poison")
    assert (exp != frames).any() and (exp != clean).any()


def test_two_calls_give_identical_bytes():
    from pytorch_pose_proposal_network_amd import render
    rng = np.random.default_rng(8)
    count, kp_cell, bbox = RC.people(rng, 3, 6, 72, 88)
    res = _result(count, kp_cell, bbox)
    src = torch.from_numpy(RC.gradient(3, 72, 88)).cuda()
    rend = render.Renderer(3, 6)
    a = rend(src, res).cpu().numpy()
    out = torch.empty_like(src)
    assert rend(src, res, out=out) is out
    assert np.array_equal(a, out.cpu().numpy())
    assert np.array_equal(a, RC.ref_draw(RC.gradient(3, 72, 88), count, kp_cell, bbox))
    with pytest.raises(ValueError):
        rend(src[:2].contiguous(), res)                                      # not the renderer's batch
    with pytest.raises(ValueError):
        rend(src, res, out=torch.empty(3, 72, 88, 4, dtype=torch.uint8, device="cuda"))


def test_reference_shaped_draw_humans():
    from pytorch_pose_proposal_network_amd import config, render
    c = RC.fixture()[0][0]
    humans = [{k: c["bbox"][i, k] for k in config.kp_paint_order() if c["kp_cell"][i, k] >= 0} for i in range(c["count"])]
    got = render.draw_humans(config.KEYPOINT_NAMES, config.EDGES, c["base"].copy(), humans, visbbox=c["visbbox"])
    assert np.array_equal(np.asarray(got), c["expected"])
    try:
        from PIL import Image
    except ImportError:                      # the array form above is the whole test where Pillow is absent
        return
    pil = Image.fromarray(c["base"].copy())
    assert render.draw_humans(config.KEYPOINT_NAMES, config.EDGES, pil, humans, visbbox=c["visbbox"]) is pil
    assert np.array_equal(np.asarray(pil), c["expected"])


def test_pipeline_draws_what_it_decoded(golden_dir):
    from pytorch_pose_proposal_network_amd import prng, render, rt, synth
    g = np.load(os.path.join(golden_dir, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    model, outsize, _ = rt.network(image_size=96, state_dict=synth.make_state_dict("drn_d_22", 0, bn_stats=stats))
    u8 = prng.u8_frames(5, 3, (96, 96))
    frames = torch.from_numpy(u8).cuda()
    res, drawn = rt.inference_batch_drawn(frames, model, gridOn=True)
    assert drawn.shape == frames.shape and drawn.data_ptr() != frames.data_ptr()
    hosted = res.to_host()
    plain = rt.inference_batch(frames, model).to_host()
    for a, b in zip(hosted, plain):
        assert a["n"] == b["n"]
        for k in ("kp_cell", "limb_arg", "bbox", "score"):
            assert np.array_equal(a[k], b[k]), k
    got = drawn.cpu().numpy()
    for i, r in enumerate(hosted):
        n = r["n"]
        kp = r["kp_cell"][None] if n else np.full((1, 1, K), -1, np.int32)
        bb = r["bbox"][None] if n else np.zeros((1, 1, K, 4), np.float32)
        exp = RC.ref_draw(u8[i:i + 1], [n], kp, bb, grid=True, grid_step=int(96 / outsize[0]))[0]
        assert int((got[i] != exp).any(-1).sum()) == 0, f"image {i}: {n} people"
    assert (got != u8).any()
    # the one-frame entry point draws the people rt.inference returns for that frame
    one = rt.inference_drawn(u8[0], model, outsize, (21, 21), gridOn=True)
    humans, _ = rt.inference(u8[0], model, outsize, (21, 21))
    exp = RC.ref_draw(u8[:1], *render.pack_humans(humans), grid=True, grid_step=int(96 / outsize[0]))[0]
    assert np.array_equal(np.asarray(one), exp)
