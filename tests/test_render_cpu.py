"""Drawing the decoded people, host side (no GPU): the NumPy restatement tests/render_ref.py against the frames the
reference's own draw_humans produced (tests/golden/draw_cases.npz) and against the installed Pillow, bit for bit; the
binding of the two entry points and the argument checks of pytorch_pose_proposal_network_amd/render.py."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import render_cases as RC
import render_ref as R


def _render():
    from pytorch_pose_proposal_network_amd import render
    return render


# ------------------------------------------------------------------------------------------- restatement vs the reference

def test_restatement_equals_every_frame_the_reference_drew():
    cases, _, order, edges, pillow = RC.fixture()
    from pytorch_pose_proposal_network_amd import config
    assert order == config.kp_paint_order() and [list(e) for e in edges] == config.EDGES
    assert len(cases) >= 20 and pillow
    kinds = {c["name"].rstrip("0123456789") for c in cases}
    assert {"random", "outside", "rootonly", "overlap", "overlap_vis", "zerolimb", "decoded"} <= kinds
    assert {c["base"].shape[:2] for c in cases} == {(96, 96), (64, 96), (96, 64)}
    assert any(c["visbbox"] for c in cases) and any(c["grid"] for c in cases) and any(c["bbox"].min() < 0 for c in cases)
    for c in cases:
        got = RC.ref_draw(c["base"][None], [c["count"]], c["kp_cell"][None], c["bbox"][None], c["visbbox"], c["grid"],
                          c["grid_step"])[0]
        assert int((got != c["expected"]).any(-1).sum()) == 0, c["name"]
        assert (c["expected"] != c["base"]).any(), c["name"]


def test_palette_and_paint_order_follow_the_config():
    from pytorch_pose_proposal_network_amd import config
    _, palette, order, _, _ = RC.fixture()
    assert [tuple(int(v) for v in c) for c in palette] == [config.COLOR_MAP[n] for n in config.KEYPOINT_NAMES]
    assert sorted(order) == list(range(config.K)) and order[0] == config.ROOT_NODE
    # the root, then the targets of DIRECTED_GRAPHS flattened (first insertion fixes a dict key's position)
    flat = [config.ROOT_NODE]
    for _, targets in config.DIRECTED_GRAPHS:
        flat += [t for t in targets if t not in flat]
    assert order == flat


# ----------------------------------------------------------------------------------------------- restatement vs Pillow

def _pil_line(H, W, x0, y0, x1, y1):
    from PIL import Image, ImageDraw
    im = Image.new("L", (W, H), 0)
    ImageDraw.Draw(im).line([x0, y0, x1, y1], fill=255, width=2)
    return np.array(im) > 0


def test_line_equals_pillow_for_every_small_vector():
    pytest.importorskip("PIL")
    bad = [(dx, dy) for dx in range(-24, 25) for dy in range(-24, 25)
           if not np.array_equal(_pil_line(56, 60, 30, 28, 30 + dx, 28 + dy), R.line_mask(56, 60, 30, 28, 30 + dx, 28 + dy))]
    assert not bad, bad[:10]


def test_line_equals_pillow_on_clipped_segments():
    pytest.importorskip("PIL")
    rnd = random.Random(1)
    bad = []
    for H, W, pad, n in ((64, 96, 40, 2400), (96, 64, 40, 600), (384, 384, 20, 300)):
        for _ in range(n):
            x0, x1 = rnd.randint(-pad, W + pad), rnd.randint(-pad, W + pad)
            y0, y1 = rnd.randint(-pad, H + pad), rnd.randint(-pad, H + pad)
            if not np.array_equal(_pil_line(H, W, x0, y0, x1, y1), R.line_mask(H, W, x0, y0, x1, y1)):
                bad.append((H, W, x0, y0, x1, y1))
    assert not bad, bad[:10]


def test_quad_offsets_need_no_square_root():
    """dxmax = RD(dy / hypot) and dymax = RU(dx / hypot) are +-1 exactly when 3 dy^2 > dx^2 (3 dx^2 > dy^2): the kernel's
    integer form of the rule."""
    for dx in range(-70, 71):
        for dy in range(-70, 71):
            if dx or dy:
                v = R.quad(0, 0, dx, dy)
                assert v[3][0] == (int(3 * dy * dy > dx * dx) * (1 if dy > 0 else -1))
                assert v[0][1] == (int(3 * dx * dx > dy * dy) * (1 if dx > 0 else -1))


def test_discs_equal_pillow_at_quarter_pixel_centres():
    pytest.importorskip("PIL")
    from PIL import Image, ImageDraw
    H, W = 14, 18
    bad = []
    for qx in range(-6 * 4, (W + 6) * 4):
        for qy in range(-6 * 4, (H + 6) * 4):
            x, y = np.float32(qx / 4), np.float32(qy / 4)
            im = Image.new("L", (W, H), 0)
            ImageDraw.Draw(im).ellipse((x - 2, y - 2, x + 2, y + 2), fill=255)
            if not np.array_equal(np.array(im) > 0, R.disc_mask(H, W, x, y)):
                bad.append((float(x), float(y)))
    assert not bad, bad[:10]


def test_outlines_equal_pillow_and_degenerate_boxes_draw_nothing():
    pytest.importorskip("PIL")
    from PIL import Image, ImageDraw
    for b in ([2, 5, 2, 9], [2, 5, 3, 6], [2, 5, 6, 6], [-3, -3, 4, 4], [5, 5, 40, 40], [0, 0, 15, 15], [7, -2, 30, 3]):
        im = Image.new("L", (16, 16), 0)
        ImageDraw.Draw(im).rectangle(xy=[float(v) for v in b], fill=None, outline=255)
        assert np.array_equal(np.array(im) > 0, R.rect_mask(16, 16, *b)), b
    assert not R.rect_mask(16, 16, 5, 5, 4, 9).any() and not R.rect_mask(16, 16, 5, 5, 9, 4).any()
    assert int(R.rect_mask(16, 16, 2, 5, 6, 5).sum()) == 5          # zero height: the row itself, no stray pixels


def test_out_of_range_and_absent_keypoints_are_skipped():
    base = RC.gradient(1, 32, 40)
    kp_cell = np.full((1, 2, RC.K), -1, np.int32)
    bbox = np.full((1, 2, RC.K, 4), np.nan, np.float32)
    kp_cell[0, 0, 0], bbox[0, 0, 0] = 3, RC.box(20, 16, 12, 10)
    kp_cell[0, 0, 15], bbox[0, 0, 15] = 3, [np.inf, 1, 2, 3]                    # neck: non-finite -> absent, no limb
    kp_cell[0, 1, 0], bbox[0, 1, 0] = 3, [2.0, 3.0, float(2 ** 20), 9.0]       # |v| >= 2^20 -> skipped
    only_root = RC.ref_draw(base, [2], kp_cell, bbox)
    kp_cell[0, 0, 15] = kp_cell[0, 1, 0] = -1
    assert np.array_equal(only_root, RC.ref_draw(base, [2], kp_cell, bbox))
    assert (only_root != base).any()
    assert np.array_equal(RC.ref_draw(base, [0], kp_cell, bbox), base)
    assert np.array_equal(RC.ref_draw(base, [-3], kp_cell, bbox), base)


# ------------------------------------------------------------------------------------------------------ binding, arguments

def test_draw_entry_points_are_exported_and_bound():
    from pytorch_pose_proposal_network_amd import lib
    assert {"ppn_draw_humans", "ppn_draw_workspace_bytes"} <= set(lib.EXPORTS)
    l = lib.load()
    assert l.ppn_draw_humans.restype is C.c_int and l.ppn_draw_workspace_bytes.restype is C.c_size_t
    c = _render().make_cfg()
    assert (c.K, c.E) == (RC.K, RC.E)
    assert l.ppn_draw_workspace_bytes(C.byref(c), 2, 36) == 2 * 36 * (RC.K + RC.E) * 48
    assert l.ppn_draw_workspace_bytes(C.byref(c), 0, 36) == 0 and l.ppn_draw_workspace_bytes(None, 1, 1) == 0


def test_bad_arguments_are_rejected_without_a_gpu():
    from pytorch_pose_proposal_network_amd import lib
    from pytorch_pose_proposal_network_amd.decode import DecodeResult
    Rn = _render()
    l = lib.load()
    c = Rn.make_cfg()
    buf = (C.c_uint8 * 64)()
    p = C.cast(buf, C.c_void_p)
    args = [p, p, 1, 2, 2, p, p, p, 1, p, None]
    assert l.ppn_draw_humans(None, *args) == -1 and b"NULL" in l.ppn_last_error()
    for i in (0, 1, 5, 6, 7, 9):                                               # each pointer in turn
        a = list(args)
        a[i] = None
        assert l.ppn_draw_humans(C.byref(c), *a) == -1 and b"NULL" in l.ppn_last_error()
    for i, v in ((2, 0), (3, 0), (4, -1), (8, 0)):
        a = list(args)
        a[i] = v
        assert l.ppn_draw_humans(C.byref(c), *a) == -1
    a = list(args)
    a[3] = 40000
    assert l.ppn_draw_humans(C.byref(c), *a) == -3                            # PPN_E_UNSUPPORTED: a documented limit
    bad = Rn.make_cfg()
    bad.kp_order[3] = 18
    assert l.ppn_draw_humans(C.byref(bad), *args) == -1
    bad = Rn.make_cfg(grid=True, grid_step=4)
    bad.grid_step = 0
    assert l.ppn_draw_humans(C.byref(bad), *args) == -1

    res = DecodeResult(count=torch.zeros(1, dtype=torch.int32), kp_cell=torch.zeros(1, 2, RC.K, dtype=torch.int32),
                       limb_arg=torch.zeros(1, 2, RC.E, dtype=torch.int32), bbox=torch.zeros(1, 2, RC.K, 4),
                       score=torch.zeros(1, 2, RC.K), max_humans=2)
    for frames in (torch.zeros(1, 8, 8, 3), torch.zeros(8, 8, 3, dtype=torch.uint8),
                   torch.zeros(1, 8, 8, 4, dtype=torch.uint8), torch.zeros(1, 8, 8, 3, dtype=torch.uint8),   # not on the device
                   np.zeros((1, 8, 8, 3), np.uint8)):
        with pytest.raises(ValueError):
            Rn.draw_people(frames, res)
    with pytest.raises(NotImplementedError):
        Rn.draw_humans(["a"], [], np.zeros((8, 8, 3), np.uint8), [], mask=object())
    with pytest.raises(ValueError):
        Rn.make_cfg(palette=[(0, 0, 0)] * 3)
    with pytest.raises(ValueError):
        Rn.make_cfg(kp_order=[0] * 17)
    with pytest.raises(ValueError):
        Rn.make_cfg(grid=True, grid_step=0)
    with pytest.raises(ValueError):
        Rn.pack_humans([{18: [0, 0, 1, 1]}])


def test_pack_humans_matches_the_compact_layout():
    Rn = _render()
    count, kp_cell, bbox = Rn.pack_humans([{0: [1, 2, 3, 4], 15: np.array([5, 6, 7, 8], np.float32)}, {0: [0, 0, 9, 9]}])
    assert count.tolist() == [2] and kp_cell.shape == (1, 2, RC.K) and bbox.shape == (1, 2, RC.K, 4)
    assert (kp_cell[0, 0] >= 0).nonzero()[0].tolist() == [0, 15] and bbox[0, 0, 15].tolist() == [5, 6, 7, 8]
    count, kp_cell, bbox = Rn.pack_humans([])
    assert count.tolist() == [0] and kp_cell.shape == (1, 1, RC.K)
