"""GPU: the windowed inference's kernels against tests/windows_ref.py, every byte.  ppn_ingest_windows == the whole-picture
ingest on the window's own crop (four formats, borders, the per-window halving path, both store paths, guard bands);
ppn_merge_windows == the restatement's six rules on planted people (all five outputs, untouched rows included); and
rt.inference_windows == the manual composition, feeding Tracker.update and to_humans() as it is."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import track_ref as TR
import windows_cases as WC
import windows_ref as R
import yuv_ref as Y

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, W = 36, 52
GUARD, FILL = 64, 0x5A
# every picture border is touched; per output size one window of exactly twice the output (the halving path beside
# bilinear windows of the same launch): 16 x 24 -> 8 x 12 (twice), 14 x 18 -> 7 x 9, 10 x 2 -> 5 x 1; and a 2 x 2 window
WINDOWS = [(0, 0, 36, 52), (0, 0, 16, 24), (20, 28, 16, 24), (0, 40, 36, 12), (34, 0, 2, 2), (10, 6, 14, 18), (4, 8, 10, 2)]
SIZES = [(8, 12), (7, 9), (5, 1)]               # dword stores; byte stores with a tail thread (9 = 2 * 4 + 1; 1)


def _windows16():
    rng = np.random.default_rng(16)
    out = list(WINDOWS)
    while len(out) < 16:
        h, w = 2 * int(rng.integers(1, 18)), 2 * int(rng.integers(1, 26))
        out.append((2 * int(rng.integers(0, (H - h) // 2 + 1)), 2 * int(rng.integers(0, (W - w) // 2 + 1)), h, w))
    return out


def _frames(fmt, seed, batch=3):
    """(host u8 [F, ...], device tensor as ingest_windows takes it, pitch): a pitch above the row's bytes and a frame stride
    above the plane."""
    rng = np.random.default_rng(seed)
    if fmt == "bgr":
        pitch = 3 * W + 12
        host = rng.integers(0, 256, (batch, H + 1, pitch), dtype=np.uint8)
        return host.reshape(batch, -1), torch.from_numpy(host).cuda()[:, :H], pitch
    pitch = 128 if fmt == "yuyv" else 64
    host = rng.integers(0, 256, (batch, Y.frame_bytes(fmt, H, W, pitch) + 37), dtype=np.uint8)
    return host, torch.from_numpy(host).cuda(), pitch


def _guarded(images, h, w, misalign=0):
    """A destination [images, h, w, 3] inside a buffer of FILL bytes, GUARD of them on either side."""
    n = images * h * w * 3
    big = torch.full((n + 2 * GUARD + 8,), FILL, dtype=torch.uint8, device="cuda")
    base = GUARD + (misalign - (big.data_ptr() + GUARD)) % 4
    out = big[base:base + n].view(images, h, w, 3)
    assert out.data_ptr() % 4 == misalign
    return big, base, out


def _check_ingest(fmt, windows, size, seed, misalign=0, **kw):
    from pytorch_pose_proposal_network_amd import windows as Wn
    host, dev, pitch = _frames(fmt, seed)
    lay = Wn.WindowLayout((H, W), windows)
    big, base, out = _guarded(len(host) * lay.n, size[0], size[1], misalign)
    got = Wn.ingest_windows(dev, fmt, lay, size, out=out, pitch=pitch, **kw)
    assert got.data_ptr() == out.data_ptr()
    exp = R.ingest_windows(host, fmt, H, W, windows, size, pitch, **kw)
    got = got.cpu().numpy()
    for b in range(len(exp)):
        assert np.array_equal(got[b], exp[b]), (fmt, divmod(b, lay.n), windows[b % lay.n], int((got[b] != exp[b]).sum()))
    outside = big.cpu().numpy()
    assert (outside[:base] == FILL).all() and (outside[base + exp.size:] == FILL).all()          # nothing beside the images
    return host, dev, pitch, got


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_ingest_windows_borders_halving_and_store_paths(fmt, size, flip):
    _check_ingest(fmt, WINDOWS, size, 100 + len(fmt) + size[0], flip=flip)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_ingest_sixteen_windows(fmt):
    _check_ingest(fmt, _windows16(), (7, 9), 200 + len(fmt))


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("fmt", R.FORMATS)
def test_one_whole_picture_window_equals_the_whole_frame_entry(fmt, flip):
    from pytorch_pose_proposal_network_amd import lib as L, rt
    size = (8, 12)
    host, dev, pitch, got = _check_ingest(fmt, [(0, 0, H, W)], size, 300 + len(fmt), flip=flip)
    if fmt == "bgr":
        tight = dev[:, :, :3 * W].contiguous()
        old = torch.empty(len(host), size[0], size[1], 3, dtype=torch.uint8, device="cuda")
        L.check(L.load().ppn_ingest_frames(tight.data_ptr(), len(host), H, W, old.data_ptr(), size[0], size[1], int(flip), 1,
                                           L.current_stream_ptr()), "ppn_ingest_frames")
    else:
        old = rt.ingest_yuv(dev, fmt, (H, W), size=size, flip=flip, pitch=pitch)
    assert np.array_equal(got, old.cpu().numpy())


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_ingest_into_a_misaligned_destination(fmt):
    _check_ingest(fmt, WINDOWS, (8, 12), 400 + len(fmt), misalign=1)                     # dst_w % 4 == 0: the address decides


@pytest.mark.parametrize("matrix,full_range", [("bt709", False), ("bt601", True), ("bt709", True)])
def test_ingest_matrices_and_ranges(matrix, full_range):
    _check_ingest("nv12", WINDOWS, (7, 9), 500, matrix=matrix, full_range=full_range)
    _check_ingest("yuyv", WINDOWS[:3], (8, 12), 501, matrix=matrix, full_range=full_range, flip=True)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_ingest_dst_bgr(fmt):
    from pytorch_pose_proposal_network_amd import lib as L, rt, windows as Wn
    host, dev, pitch = _frames(fmt, 600 + len(fmt))
    lay = Wn.WindowLayout((H, W), WINDOWS)
    size = (7, 9)
    out = torch.zeros(len(host) * lay.n, size[0], size[1], 3, dtype=torch.uint8, device="cuda")
    if fmt == "bgr":
        planes = dict(pitch=pitch, pitch_c=0, frame_stride=dev.stride(0), y=dev.data_ptr(), u=None, v=None)
    else:
        n, p, pc, uo, vo = rt.yuv_frame_layout(fmt, (H, W), pitch)
        planes = dict(pitch=p, pitch_c=pc, frame_stride=dev.stride(0), y=dev.data_ptr(),
                      u=None if uo is None else dev.data_ptr() + uo, v=None if vo is None else dev.data_ptr() + vo)
    d = L.IngestDesc(format=R.FORMATS.index(fmt), batch=len(host), src_h=H, src_w=W, matrix=0, full_range=0,
                     dst=out.data_ptr(), dst_h=size[0], dst_w=size[1], flip=1, dst_bgr=1, **planes)
    L.check(L.load().ppn_ingest_windows(C.byref(d), C.byref(lay.struct), L.current_stream_ptr()), "ppn_ingest_windows")
    exp = R.ingest_windows(host, fmt, H, W, WINDOWS, size, pitch, flip=True, dst_bgr=True)
    assert np.array_equal(out.cpu().numpy(), exp)
    assert np.array_equal(exp[..., ::-1], R.ingest_windows(host, fmt, H, W, WINDOWS, size, pitch, flip=True))


# ---- merge ----------------------------------------------------------------------------------------------------------
SENTINEL = 0xC3


def _merger(case, max_out, merge_thr=0.3, fuse=True):
    from pytorch_pose_proposal_network_amd import windows as Wn
    big = max(max(y0 + h for y0, _, h, _ in case.windows), max(x0 + w for _, x0, _, w in case.windows))
    lay = Wn.WindowLayout((big, big), case.windows)
    m = Wn.WindowMerger(lay, case.frames, case.in_hw, case.M, max_out, merge_thr, fuse, K=case.K)
    for t in (m.out.count, m.out.kp_cell, m.out.bbox, m.out.score, m.flags):
        t.view(torch.uint8).fill_(SENTINEL)
    return m


def _result(case):
    from pytorch_pose_proposal_network_amd import decode as D
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()                     # a copy: the cases are read-only
    B = len(case.count)
    return D.DecodeResult(dev(case.count), dev(case.kp_cell), torch.zeros(B, case.M, 1, dtype=torch.int32, device="cuda"),
                          dev(case.bbox), dev(case.score), case.M)


def _same(got, exp, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == exp.shape, what
    a, b = np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(exp).view(np.uint8)
    assert np.array_equal(a, b), (what, int((a != b).sum()))


def _check_merge(case, max_out, merge_thr=0.3, fuse=True):
    m = _merger(case, max_out, merge_thr, fuse)
    res = m(_result(case))
    exp, keeper = case.ref(max_out, merge_thr, fuse, out=R.fresh_outputs(case.frames, max_out, case.K, fill=SENTINEL))
    assert res.max_humans == max_out and res.kp_cell.data_ptr() == m.out.kp_cell.data_ptr()
    _same(res.count, exp["count"], "count")
    _same(m.flags, exp["flags"], "flags")
    _same(res.kp_cell, exp["src"], "src")
    _same(res.bbox, exp["bbox"], "bbox")
    _same(res.score, exp["score"], "score")
    return m, res, exp, keeper


@pytest.fixture(scope="module")
def crowd():
    return WC.crowd()


MERGE_CASES = [
    ("overlap", lambda: WC.overlap_person(), 8), ("overlap-max_out-1", lambda: WC.overlap_person(), 1),
    ("same-window", lambda: WC.same_window_pair(), 4), ("chain", lambda: WC.chain(), 4), ("ties", lambda: WC.equal_scores(), 4),
    ("skipped", lambda: WC.skipped(), 16), ("mixed-M7-K18", lambda: WC.mixed_batch(), 5), ("mixed-roomy", lambda: WC.mixed_batch(), 14),
    ("identity-n1", lambda: WC.identity(), 6), ("planted-n16-K32", lambda: WC.planted(), 5),
    ("planted-roomy", lambda: WC.planted(), 40), ("mapping-sweep", lambda: WC.mapping_sweep(), 200),
]


@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("name,build,max_out", MERGE_CASES, ids=[c[0] for c in MERGE_CASES])
def test_merge_matches_the_restatement(name, build, max_out, fuse):
    case = build()
    m, res, exp, keeper = _check_merge(case, max_out, fuse=fuse)
    if name.startswith("planted"):                       # the case is worth its name: duplicates exist, rows overflow at 5
        assert any(k != c for kp in keeper for c, k in kp.items())
        assert (exp["count"] > 5).all() and ((exp["flags"] & R.OUT_OVERFLOW) != 0).all() == (max_out == 5)


@pytest.mark.parametrize("max_out", [100, 600])
def test_merge_more_than_512_candidates_beside_a_quiet_frame(crowd, max_out):
    m, res, exp, keeper = _check_merge(crowd, max_out)
    assert exp["count"].tolist() == [512, 1]
    assert exp["flags"].tolist() == [R.CAND_OVERFLOW | (R.OUT_OVERFLOW if max_out < 512 else 0), 0]


def test_merge_threshold_sweep():
    case, _ = WC.threshold_sweep()
    m, res, exp, _ = _check_merge(case, 2)
    assert 10 <= int((exp["count"] == 1).sum()) <= case.frames - 10
    # a threshold of 0 merges every pair of windows (iou 0 >= 0), +inf none
    _check_merge(case, 2, merge_thr=0.0)
    _check_merge(case, 2, merge_thr=float("inf"))


def test_merge_twice_gives_the_same_bytes():
    case = WC.planted()
    m, res, exp, _ = _check_merge(case, 12)
    first = [t.clone() for t in (res.count, res.kp_cell, res.bbox, res.score, m.flags)]
    res = m(_result(case))
    for a, b in zip(first, (res.count, res.kp_cell, res.bbox, res.score, m.flags)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_merge_under_graph_capture():
    case, other = WC.planted(), WC.planted(seed=9)
    staged = _result(case)
    m = _merger(case, 12)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _merger(case, 12)(staged)                                            # the module is loaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m(staged)
    for c in (case, other):
        for t in (m.out.count, m.out.kp_cell, m.out.bbox, m.out.score, m.flags):
            t.view(torch.uint8).fill_(SENTINEL)
        for k in ("count", "kp_cell", "bbox", "score"):
            getattr(staged, k).copy_(torch.from_numpy(np.array(getattr(c, k))))
        g.replay()
        torch.cuda.synchronize()
        exp, _ = c.ref(12, out=R.fresh_outputs(c.frames, 12, c.K, fill=SENTINEL))
        for got, key in ((m.out.count, "count"), (m.flags, "flags"), (m.out.kp_cell, "src"), (m.out.bbox, "bbox"),
                         (m.out.score, "score")):
            _same(got, exp[key], key)


def test_merger_checks_its_input():
    from pytorch_pose_proposal_network_amd import decode as D
    case = WC.chain()
    m = _merger(case, 4)
    good = _result(case)
    with pytest.raises(ValueError):
        m(D.DecodeResult(good.count, good.kp_cell, good.limb_arg, good.bbox, good.score, case.M + 1))
    with pytest.raises(ValueError):
        m(D.DecodeResult(good.count[:2], good.kp_cell, good.limb_arg, good.bbox, good.score, case.M))
    with pytest.raises(ValueError):
        m(D.DecodeResult(good.count, good.kp_cell, good.limb_arg, good.bbox.double(), good.score, case.M))


# ---- network level: D-22, float32, 96 x 96 ---------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
def test_inference_windows_equals_the_manual_composition(flip):
    from pytorch_pose_proposal_network_amd import drn, model, rt, synth, track, windows as Wn
    g = np.load(os.path.join(GOLDEN, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    m = model.PoseProposalNet(drn.drn_d_22(), insize=(96, 96), outsize=(6, 6), compute_dtype="float32").cuda()
    m.load_state_dict(synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats))
    m.eval()
    h, w, F_ = 144, 208, 2
    host = np.random.default_rng(700).integers(0, 256, (F_, Y.frame_bytes("nv12", h, w)), dtype=np.uint8)
    raw = torch.from_numpy(host).cuda()
    lay = Wn.WindowLayout.tiles((h, w), 2, 2)

    def whole():
        frames = rt.ingest_yuv(raw, "nv12", (h, w), size=96)
        return frames.clone(), rt.inference_batch(frames, m).to_host()           # the rows of people only

    before = whole()
    for b in range(F_):
        assert np.array_equal(before[0][b].cpu().numpy(), Y.ingest(host[b], "nv12", h, w, (96, 96)))

    merged = rt.inference_windows(raw, "nv12", (h, w), m, lay, size=96, flip=flip)
    got = {k: getattr(merged, k).clone() for k in ("count", "kp_cell", "limb_arg", "bbox", "score")}

    # the manual composition: planes cropped on the host, the whole-picture ingest per window, inference_batch, the
    # restatement's merge
    # (flip: every window image turned by 180 degrees, its people placed by the layout of the turned frame)
    crops = [rt.ingest_yuv(torch.from_numpy(R.crop(host[f], "nv12", h, w, win)).cuda()[None], "nv12", (win[2], win[3]), size=96,
                           flip=flip) for f in range(F_) for win in lay.windows]
    placed = [(h - y0 - wh, w - x0 - ww, wh, ww) for y0, x0, wh, ww in lay.windows] if flip else list(lay.windows)
    res = rt.inference_batch(torch.cat(crops), m)
    assert res.max_humans == 36 and int(res.count.sum()) > 0
    exp, keeper = R.merge(placed, (96, 96), res.count.cpu().numpy(), res.kp_cell.cpu().numpy(),
                          res.bbox.cpu().numpy(), res.score.cpu().numpy(), F_, merged.max_humans)
    assert merged.max_humans == 4 * 36 and int(exp["count"].sum()) > 0
    _same(got["count"], exp["count"], "count")
    _same(got["kp_cell"], exp["src"], "src")
    _same(got["bbox"], exp["bbox"], "bbox")
    _same(got["score"], exp["score"], "score")
    assert (got["limb_arg"] == -1).all()
    # a merger of one's own must stand on the layout the window images lie in
    good = Wn.WindowMerger(Wn.WindowLayout((h, w), placed), F_, (96, 96), 36)
    again = rt.inference_windows(raw, "nv12", (h, w), m, lay, merger=good, size=96, flip=flip)
    _same(again.kp_cell, exp["src"], "src through a merger of one's own")
    if flip:
        with pytest.raises(ValueError):
            rt.inference_windows(raw, "nv12", (h, w), m, lay, merger=Wn.WindowMerger(lay, F_, (96, 96), 36), size=96, flip=True)

    # the merged result feeds the tracker and to_humans() as it is
    tr = track.Tracker(1, F_, merged.max_humans)
    tracks = tr.update(merged)
    ref = TR.track_update(TR.make_cfg(K=18), TR.fresh_state(1, 18), exp["count"], exp["src"], exp["bbox"], exp["score"], 1, F_)
    _same(tracks.ids, ref["ids"], "ids")
    _same(tracks.hits, ref["hits"], "hits")
    humans = merged.to_humans()
    assert [len(hm) for hm, _ in humans] == exp["count"].tolist()
    for f in range(F_):
        for r, (hm, sc) in enumerate(zip(*humans[f])):
            assert sorted(hm) == [j for j in range(18) if exp["src"][f, r, j] >= 0]
            assert all(np.array_equal(hm[j], exp["bbox"][f, r, j]) for j in hm)

    # the whole-frame entry points give the bytes they gave before the windowed call
    after = whole()
    assert torch.equal(before[0], after[0])
    for a, b in zip(before[1], after[1]):
        assert a["n"] == b["n"] and all(np.array_equal(a[k], b[k]) for k in ("kp_cell", "limb_arg", "bbox", "score"))
