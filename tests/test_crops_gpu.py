"""GPU: the person crops' kernels against tests/crops_ref.py, every byte.  ppn_ingest_rois == ppn_ingest_windows on a layout of
that one rectangle and == the restatement (four formats, borders, the per-ROI halving path, both store paths, empty and bad
slots, guard bands); ppn_people_rois == the restatement's eight rules on planted people; rois -> crop under graph capture;
and rt.inference_crops == the manual composition."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import crops_cases as CC
import crops_ref as R
import windows_ref as WR
import yuv_ref as Y

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H, W = 36, 52
GUARD, FILL = 64, 0x5A
SENTINEL = 0xC3
HELD = 0x100                                     # a bit the status table holds before the call: the bits are OR-ed in
# output size -> the ROI of exactly twice that size (the halving path beside bilinear ROIs of the same launch)
SIZES = {(8, 12): (20, 28, 16, 24), (7, 9): (10, 6, 14, 18), (5, 1): (4, 8, 10, 2)}
# dword stores; byte stores with a tail thread (9 = 2 * 4 + 1; 1).  34 / 8, 50 / 12, 34 / 12, 50 / 9, 34 / 7 ...: most scales
# are not representable, so the device's double division has to give the host's bits
GOOD = [(0, 0, 34, 50), (2, 18, 10, 34), (20, 2, 16, 50), (0, 0, 36, 52), (34, 50, 2, 2), (0, 0, 0, 0)]
BAD = [(-2, 0, 4, 4), (0, -2, 4, 4), (4, 4, 0, 4), (4, 4, 4, -2), (-4, -4, -4, -4), (34, 0, 4, 4), (0, 50, 4, 4),
       (2, 2, 2 ** 31 - 2, 4), (2, 2, 4, 2 ** 31 - 2), (0, 0, 0, 2),
       (0, 1, 4, 4), (0, 0, 4, 3), (1, 0, 4, 4), (0, 0, 3, 4)]          # odd: bad where the format shares chroma, good elsewhere


def _table(fmt, size, frames=3):
    """i32 [frames, R, 4]: every frame holds the same rectangles in another order."""
    rows = [SIZES[size]] + GOOD + BAD + ([(35, 51, 1, 1), (1, 3, 33, 47)] if fmt == "bgr" else [])
    rng = np.random.default_rng(len(rows))
    return np.stack([np.array(rows, np.int32)[rng.permutation(len(rows))] for _ in range(frames)])


def _frames(fmt, seed, batch=3):
    """(host u8 [F, ...], device tensor as ingest_rois takes it, pitch): the frames lie inside a larger buffer -- a pitch
    above the row's bytes, a frame stride above the planes."""
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


def _status(frames, rois, value):
    """(the over-allocated buffer, its [frames, rois] head): `value` in the head, the sentinel behind it."""
    big = torch.full((frames * rois + 16,), 0, dtype=torch.int32, device="cuda")
    big.view(torch.uint8).fill_(SENTINEL)
    big[:frames * rois] = value
    return big, big[:frames * rois].view(frames, rois)


def _tail_is_untouched(big, used):
    assert (big[used:].view(torch.uint8) == SENTINEL).all()


def _check_ingest(fmt, size, seed, misalign=0, with_status=True, **kw):
    from pytorch_pose_proposal_network_amd import crops, windows as Wn
    host, dev, pitch = _frames(fmt, seed)
    table = _table(fmt, size)
    F_, Rn, _ = table.shape
    roi = torch.from_numpy(table).cuda()
    big, base, out = _guarded(F_ * Rn, size[0], size[1], misalign)
    sbig, status = _status(F_, Rn, HELD) if with_status else (None, None)
    got = crops.ingest_rois(dev, fmt, (H, W), roi, size, out=out, status=status, pitch=pitch, **kw)
    assert got.data_ptr() == out.data_ptr()
    exp, exp_status = R.ingest_rois(host, fmt, H, W, table, size, pitch, status=np.full((F_, Rn), HELD, np.int32), **kw)
    got = got.cpu().numpy()
    kinds = set()
    for b in range(len(exp)):
        f, r = divmod(b, Rn)
        assert np.array_equal(got[b], exp[b]), (fmt, (f, r), table[f, r].tolist(), int((got[b] != exp[b]).sum()))
        bits = int(exp_status[f, r]) & ~HELD
        kinds.add(bits)
        if bits:
            assert not got[b].any()                                          # bad and empty slots are all zero
    assert kinds == {R.OK, R.EMPTY, R.BAD}
    if with_status:
        assert np.array_equal(status.cpu().numpy(), exp_status)
        _tail_is_untouched(sbig, F_ * Rn)
    outside = big.cpu().numpy()
    assert (outside[:base] == FILL).all() and (outside[base + exp.size:] == FILL).all()          # nothing beside the images
    assert torch.equal(roi.cpu(), torch.from_numpy(table))                                       # the table is only read
    # NORMATIVE: a good ROI is a layout of one window holding that rectangle
    for rect in {tuple(int(v) for v in t) for t in table[0]}:
        if R.judge(rect, fmt, (H, W)) != R.OK:
            continue
        one = Wn.ingest_windows(dev, fmt, Wn.WindowLayout((H, W), [rect]), size, pitch=pitch, **kw).cpu().numpy()
        for f in range(F_):
            r = int(np.flatnonzero((table[f] == np.array(rect)).all(axis=1))[0])
            assert np.array_equal(got[f * Rn + r], one[f]), (fmt, rect, f)
    return host, dev, pitch, table, got


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("size", list(SIZES), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", WR.FORMATS)
def test_ingest_rois_equals_one_window_layouts_and_the_restatement(fmt, size, flip):
    _check_ingest(fmt, size, 100 + len(fmt) + size[0], flip=flip)


@pytest.mark.parametrize("fmt", WR.FORMATS)
def test_ingest_rois_into_a_misaligned_destination_without_a_status_table(fmt):
    _check_ingest(fmt, (8, 12), 400 + len(fmt), misalign=1, with_status=False)          # dst_w % 4 == 0: the address decides


@pytest.mark.parametrize("matrix,full_range", [("bt709", False), ("bt601", True), ("bt709", True)])
def test_ingest_rois_matrices_and_ranges(matrix, full_range):
    _check_ingest("nv12", (7, 9), 500, matrix=matrix, full_range=full_range)
    _check_ingest("yuyv", (8, 12), 501, matrix=matrix, full_range=full_range, flip=True)


@pytest.mark.parametrize("fmt", WR.FORMATS)
def test_ingest_rois_dst_bgr(fmt):
    from pytorch_pose_proposal_network_amd import lib as L, rt
    host, dev, pitch = _frames(fmt, 600 + len(fmt))
    size = (7, 9)
    table = _table(fmt, size)
    F_, Rn, _ = table.shape
    roi = torch.from_numpy(table).cuda()
    out = torch.full((F_ * Rn, size[0], size[1], 3), FILL, dtype=torch.uint8, device="cuda")
    if fmt == "bgr":
        planes = dict(pitch=pitch, pitch_c=0, frame_stride=dev.stride(0), y=dev.data_ptr(), u=None, v=None)
    else:
        n, p, pc, uo, vo = rt.yuv_frame_layout(fmt, (H, W), pitch)
        planes = dict(pitch=p, pitch_c=pc, frame_stride=dev.stride(0), y=dev.data_ptr(),
                      u=None if uo is None else dev.data_ptr() + uo, v=None if vo is None else dev.data_ptr() + vo)
    d = L.IngestDesc(format=WR.FORMATS.index(fmt), batch=F_, src_h=H, src_w=W, matrix=0, full_range=0, dst=out.data_ptr(),
                     dst_h=size[0], dst_w=size[1], flip=1, dst_bgr=1, **planes)
    L.check(L.load().ppn_ingest_rois(C.byref(d), roi.data_ptr(), Rn, None, L.current_stream_ptr()), "ppn_ingest_rois")
    exp, _ = R.ingest_rois(host, fmt, H, W, table, size, pitch, flip=True, dst_bgr=True)
    assert np.array_equal(out.cpu().numpy(), exp)
    assert np.array_equal(exp[..., ::-1], R.ingest_rois(host, fmt, H, W, table, size, pitch, flip=True)[0])


# ---- ppn_people_rois ------------------------------------------------------------------------------------------------
def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                              # a copy: the cases are read-only


def _result(case):
    from pytorch_pose_proposal_network_amd import decode as D
    return D.DecodeResult(_dev(case.count), _dev(case.kp_cell), torch.zeros(case.frames, CC.M, 1, dtype=torch.int32, device="cuda"),
                          _dev(case.bbox), _dev(case.score), CC.M)


def _cfg(mode, margin, keep, align, max_rois, min_size=4):
    from pytorch_pose_proposal_network_amd import lib as L
    sy, sx = R.scales(CC.SRC_HW, CC.COORDS_HW)
    aspect = R.aspect_of(CC.OUT_HW) if keep else np.float32(0)
    return L.RoiCfg(CC.K, CC.M, max_rois, CC.SRC_HW[0], CC.SRC_HW[1], float(sy), float(sx), mode, margin, float(aspect),
                    align[0], align[1], min_size), dict(sy=sy, sx=sx, aspect=aspect)


def _run_people_rois(case, mode, margin, keep, align, max_rois):
    """The C entry on over-allocated tables: (roi, status) as NumPy, the tails checked."""
    from pytorch_pose_proposal_network_amd import lib as L
    cfg, f32 = _cfg(mode, margin, keep, align, max_rois)
    res = _result(case)
    n = case.frames * max_rois
    rbig = torch.zeros(4 * n + 16, dtype=torch.int32, device="cuda")
    rbig.view(torch.uint8).fill_(SENTINEL)
    sbig, status = _status(case.frames, max_rois, -1)
    L.check(L.load().ppn_people_rois(C.byref(cfg), res.count.data_ptr(), res.kp_cell.data_ptr(), res.bbox.data_ptr(),
                                     case.frames, rbig.data_ptr(), sbig.data_ptr(), L.current_stream_ptr()), "ppn_people_rois")
    _tail_is_untouched(rbig, 4 * n)
    _tail_is_untouched(sbig, n)
    exp = R.people_rois(case.count, case.kp_cell, case.bbox, CC.SRC_HW, f32["sy"], f32["sx"], max_rois, mode, margin,
                        f32["aspect"], align, 4)
    return rbig[:4 * n].view(case.frames, max_rois, 4).cpu().numpy(), status.cpu().numpy(), exp


PEOPLE = {"planted": CC.planted, "nan-root": CC.nan_root, "random-11": lambda: CC.random_people(11),
          "random-12": lambda: CC.random_people(12)}


@pytest.mark.parametrize("mode,margin,keep,align,max_rois", CC.CONFIGS)
def test_people_rois_match_the_restatement(mode, margin, keep, align, max_rois):
    seen = set()
    for name, build in PEOPLE.items():
        roi, status, (eroi, estatus) = _run_people_rois(build(), mode, margin, keep, align, max_rois)
        assert np.array_equal(status, estatus), (name, np.argwhere(status != estatus).tolist())
        assert np.array_equal(roi, eroi), (name, np.argwhere((roi != eroi).any(axis=2)).tolist())
        seen |= set(np.unique(estatus).tolist())
    assert seen == {R.OK, R.EMPTY, R.DEGENERATE}


def test_people_rois_twice_give_the_same_bytes():
    a = _run_people_rois(CC.planted(), 1, 0.1, True, (2, 2), 8)
    b = _run_people_rois(CC.planted(), 1, 0.1, True, (2, 2), 8)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _cropper(frames, **kw):
    from pytorch_pose_proposal_network_amd import crops
    args = dict(max_crops=8, min_size=4, coords_hw=CC.COORDS_HW, K=CC.K)
    args.update(kw)
    return crops.PersonCropper(frames, CC.M, CC.SRC_HW, "nv12", CC.OUT_HW, **args)


def _expected_crops(case, host, **kw):
    sy, sx = R.scales(CC.SRC_HW, CC.COORDS_HW)
    roi, status = R.people_rois(case.count, case.kp_cell, case.bbox, CC.SRC_HW, sy, sx, 8, R.MODE_PEOPLE, 0.1,
                                R.aspect_of(CC.OUT_HW), (2, 2), 4)
    crops, status = R.ingest_rois(host, "nv12", CC.SRC_HW[0], CC.SRC_HW[1], roi, CC.OUT_HW, status=status, **kw)
    return roi, status, crops.reshape(case.frames, 8, CC.OUT_HW[0], CC.OUT_HW[1], 3)


def _raw(seed, frames):
    return np.random.default_rng(seed).integers(0, 256, (frames, Y.frame_bytes("nv12", *CC.SRC_HW)), dtype=np.uint8)


def test_cropper_equals_the_restatement_and_reads_back_the_valid_crops():
    case, host = CC.planted(), _raw(70, 3)
    cr = _cropper(3)
    out = cr(torch.from_numpy(host).cuda(), _result(case))
    roi, status, crops = _expected_crops(case, host)
    assert np.array_equal(out.roi.cpu().numpy(), roi) and np.array_equal(out.status.cpu().numpy(), status)
    assert np.array_equal(out.crops.cpu().numpy(), crops)
    assert (status[status != R.OK] & R.EMPTY).all()                          # a degenerate slot is an empty rectangle to the ingest
    back = out.to_host()
    assert [b["slot"].tolist() for b in back] == [np.flatnonzero(status[f] == R.OK).tolist() for f in range(3)]
    assert sum(len(b["slot"]) for b in back) >= 5
    for f, b in enumerate(back):
        assert np.array_equal(b["roi"], roi[f, b["slot"]]) and np.array_equal(b["crops"], crops[f, b["slot"]])


def test_rois_then_crop_under_graph_capture():
    first, second = CC.planted(), CC.random_people(21, frames=3)
    hosts = _raw(71, 3), _raw(72, 3)
    staged, raw = _result(first), torch.from_numpy(hosts[0]).cuda()
    cr = _cropper(3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _cropper(3)(raw, staged)                                             # the module is loaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                # two launches in a row: a linear graph
        cr(raw, staged)
    for case, host in zip((first, second), hosts):
        for t in (cr.roi, cr.status, cr.crops):
            t.view(torch.uint8).fill_(SENTINEL)
        for k in ("count", "kp_cell", "bbox", "score"):                      # the people and the frames change in place
            getattr(staged, k).copy_(torch.from_numpy(np.array(getattr(case, k))))
        raw.copy_(torch.from_numpy(host))
        g.replay()
        torch.cuda.synchronize()
        roi, status, crops = _expected_crops(case, host)
        assert np.array_equal(cr.roi.cpu().numpy(), roi) and np.array_equal(cr.status.cpu().numpy(), status)
        assert np.array_equal(cr.crops.cpu().numpy(), crops)
        assert (status == R.OK).sum() >= 3


def test_cropper_checks_its_input():
    from pytorch_pose_proposal_network_amd import decode as D
    case = CC.planted()
    cr = _cropper(3)
    good = _result(case)
    raw = torch.from_numpy(_raw(73, 3)).cuda()
    cr(raw, good)
    bad = [D.DecodeResult(good.count, good.kp_cell, good.limb_arg, good.bbox, good.score, CC.M + 1),
           D.DecodeResult(good.count[:2], good.kp_cell, good.limb_arg, good.bbox, good.score, CC.M),
           D.DecodeResult(good.count, good.kp_cell[:, :, :4], good.limb_arg, good.bbox, good.score, CC.M),
           D.DecodeResult(good.count, good.kp_cell, good.limb_arg, good.bbox.double(), good.score, CC.M),
           D.DecodeResult(good.count.long(), good.kp_cell, good.limb_arg, good.bbox, good.score, CC.M),
           D.DecodeResult(good.count, good.kp_cell, good.limb_arg, good.bbox.cpu(), good.score, CC.M),
           D.DecodeResult(good.count, good.kp_cell, good.limb_arg, good.bbox.transpose(1, 2), good.score, CC.M)]
    for res in bad:
        with pytest.raises(ValueError):
            cr.rois(res)
    for wrong in (raw[:2], raw.cpu(), raw.float(), raw[:, :100], None):
        with pytest.raises(ValueError):
            cr.crop(wrong)
    from pytorch_pose_proposal_network_amd import crops
    for roi in (cr.roi.long(), cr.roi.cpu(), cr.roi[:2], cr.roi[:, :, :3], cr.roi.float()):
        with pytest.raises(ValueError):
            crops.ingest_rois(raw, "nv12", CC.SRC_HW, roi, CC.OUT_HW)
    with pytest.raises(ValueError):
        crops.ingest_rois(raw, "nv12", CC.SRC_HW, cr.roi, CC.OUT_HW, status=cr.status.long())
    with pytest.raises(ValueError):
        crops.ingest_rois(raw, "nv12", CC.SRC_HW, cr.roi, CC.OUT_HW, out=cr.crops[:, :4])


# ---- network level: D-22, float32, 96 x 96 ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net():
    from pytorch_pose_proposal_network_amd import drn, model, synth
    g = np.load(os.path.join(GOLDEN, "forward_d22_96.npz"))
    stats = {k[3:]: g[k] for k in g.files if k.startswith("bn/")}
    m = model.PoseProposalNet(drn.drn_d_22(), insize=(96, 96), outsize=(6, 6), compute_dtype="float32").cuda()
    m.load_state_dict(synth.make_state_dict("drn_d_22", int(g["seed_w"]), bn_stats=stats))
    m.eval()
    return m


def _same_bytes(a, b, what):
    assert a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), what


@pytest.mark.parametrize("variant", ["plain", "windows", "windows-tracked"])
def test_inference_crops_equals_the_manual_composition(net, variant):
    from pytorch_pose_proposal_network_amd import crops, rt, track, windows as Wn
    h, w, F_ = 64, 96, 2
    host = np.random.default_rng(700).integers(0, 256, (F_, Y.frame_bytes("nv12", h, w)), dtype=np.uint8)
    raw = torch.from_numpy(host).cuda()
    lay = None if variant == "plain" else Wn.WindowLayout.tiles((h, w), 2, 2)
    M = 36 if lay is None else 4 * 36
    make = lambda: crops.PersonCropper(F_, M, (h, w), "nv12", (32, 24), max_crops=8, min_size=4,
                                       coords_hw=(96, 96) if lay is None else None)
    cr = make()
    tracker = track.Tracker(1, F_, M) if variant == "windows-tracked" else None
    got = rt.inference_crops(raw, "nv12", (h, w), net, cr, layout=lay, tracker=tracker, size=96)
    assert len(got) == (3 if tracker else 2)
    res, out = got[0], got[1]
    kept = {k: getattr(res, k).clone() for k in ("count", "kp_cell", "limb_arg", "bbox", "score")}
    kept.update(roi=out.roi.clone(), status=out.status.clone(), crops=out.crops.clone())
    if tracker:
        kept.update(ids=got[2].ids.clone(), hits=got[2].hits.clone())

    # the manual composition: the plain path or inference_windows, then a tracker and a cropper of one's own
    if lay is None:
        res2 = rt.inference_batch(rt.ingest_yuv(raw, "nv12", (h, w), size=96), net)
    else:
        res2 = rt.inference_windows(raw, "nv12", (h, w), net, lay, size=96)
    assert res2.max_humans == M
    _same_bytes(kept["count"], res2.count, "count")
    for f, n in enumerate(res2.count.cpu().tolist()):                        # the rows of people: a decode writes no others
        for k in ("kp_cell", "limb_arg", "bbox", "score"):
            _same_bytes(kept[k][f, :min(n, M)], getattr(res2, k)[f, :min(n, M)], (k, f))
    if tracker:
        tr2 = track.Tracker(1, F_, M).update(res2)
        _same_bytes(kept["ids"], tr2.ids, "ids")
        _same_bytes(kept["hits"], tr2.hits, "hits")
    out2 = make()(raw, res2)
    for k in ("roi", "status", "crops"):
        _same_bytes(kept[k], getattr(out2, k), k)

    # crop r is the whole-picture ingest of the host-cropped planes of roi[f, r]; slot r is person r
    roi, status = kept["roi"].cpu().numpy(), kept["status"].cpu().numpy()
    count, root = kept["count"].cpu().numpy(), kept["kp_cell"][:, :, 0].cpu().numpy()
    assert (status == R.OK).sum() > 0
    for f in range(F_):
        for r in range(8):
            assert (status[f, r] == R.EMPTY) == bool(r >= count[f] or root[f, r] < 0)
            if status[f, r] != R.OK:
                assert not kept["crops"][f, r].any()
                continue
            rect = tuple(int(v) for v in roi[f, r])
            one = rt.ingest_yuv(torch.from_numpy(WR.crop(host[f], "nv12", h, w, rect)).cuda()[None], "nv12", (rect[2], rect[3]),
                                size=(32, 24))
            assert torch.equal(kept["crops"][f, r], one[0]), (f, r, rect)
    # the rectangles are the restatement's on the people that came out
    space = (96, 96) if lay is None else (h, w)
    sy, sx = R.scales((h, w), space)
    eroi, estatus = R.people_rois(count, kept["kp_cell"].cpu().numpy(), kept["bbox"].cpu().numpy(), (h, w), sy, sx, 8,
                                  R.MODE_PEOPLE, 0.1, R.aspect_of((32, 24)), (2, 2), 4)
    assert np.array_equal(roi, eroi)
    assert np.array_equal(status, estatus | np.where((eroi == 0).all(axis=2), R.EMPTY, 0))      # the ingest ORs its own bit in
    # a cropper that stands in another space is refused
    with pytest.raises(ValueError):
        rt.inference_crops(raw, "nv12", (h, w), net, crops.PersonCropper(F_, M, (h, w), "nv12", (32, 24), coords_hw=(50, 50)),
                           layout=lay, size=96)
