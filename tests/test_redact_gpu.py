"""GPU: the redaction's kernels against tests/redact_ref.py, every byte.  ppn_redact_cells == the restatement on planted and
random people and on the hold sequences (masks, flags and ttl, canaries around them, stale garbage overwritten, one call of
S x T frames == T calls == two uneven calls, twice the same bytes); ppn_redact_yuv == the restatement in four formats x three
cell sizes x mosaic / fill, in place and out of place on the byte and the dword path, with canaries beyond every row's
content and behind every frame and garbage in the mask's unused bits; Redactor, cells + apply under graph capture with the
hold state carried over, reset(); and rt.inference_redacted == the manual composition."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import redact_cases as RC
import redact_ref as R
import yuv_ref as Y

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CANARY = 0xC3
FORMATS = ("nv12", "i420", "yuyv", "bgr")                   # lib.PPN_PIX_* in this order
ALIGNED_PITCH = {"nv12": 536, "i420": 536, "yuyv": 1068, "bgr": 1600}      # multiples of 4 (I420: of 8) at and above the row


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                              # a copy: the cases are read-only


def _result(case, idx=None):
    from pytorch_pose_proposal_network_amd import decode as D
    pick = (lambda a: a) if idx is None else (lambda a: a[idx])
    n, M = case.frames if idx is None else len(idx), case.kp_cell.shape[1]
    return D.DecodeResult(_dev(pick(case.count)), _dev(pick(case.kp_cell)), torch.zeros(n, M, 1, dtype=torch.int32, device="cuda"),
                          _dev(pick(case.bbox)), _dev(pick(case.score)), M)


def _canaried(nbytes, dtype):
    """(the over-allocated u8 buffer, its head of `nbytes` bytes viewed as `dtype`): canary bytes everywhere."""
    big = torch.full((nbytes + 64,), CANARY, dtype=torch.uint8, device="cuda")
    return big, big[:nbytes].view(dtype)


def _tail_is_untouched(big, used):
    assert (big[used:] == CANARY).all()


# ---- ppn_redact_cells ---------------------------------------------------------------------------------------------------
def _run_cells(case, S, T, cell, hold, ttl=None, idx=None, kp_mask=RC.HEAD, fallback=R.FALLBACK_PERSON, margin=0.25, fmt="nv12"):
    """The C entry on canaried buffers whose heads hold stale garbage: (mask u32, flags, ttl') as NumPy.  `ttl`: the state
    before (None: fresh), `idx`: the images of `case` that are taken (None: all)."""
    from pytorch_pose_proposal_network_amd import lib as L
    a = RC.cells_args(fmt, cell, kp_mask, fallback, margin, hold)
    CH, CW, MW = R.grid_of(a["src_hw"], cell)
    cfg = L.RedactCellsCfg(RC.K, case.kp_cell.shape[1], a["src_hw"][0], a["src_hw"][1], cell, float(a["sy"]), float(a["sx"]), kp_mask, fallback,
                           margin, hold)
    res = _result(case, idx)
    B = S * T
    mbig, mask = _canaried(B * CH * MW * 4, torch.int32)
    fbig, flags = _canaried(B * 4, torch.int32)
    tbig, life = _canaried(S * CH * CW, torch.uint8)
    life.copy_(torch.from_numpy(np.zeros(S * CH * CW, np.uint8) if ttl is None else np.array(ttl).reshape(-1)))
    L.check(L.load().ppn_redact_cells(C.byref(cfg), tbig.data_ptr() if hold else None, res.count.data_ptr(), res.kp_cell.data_ptr(),
                                      res.bbox.data_ptr(), S, T, mbig.data_ptr(), fbig.data_ptr(), L.current_stream_ptr()),
            "ppn_redact_cells")
    for big, used in ((mbig, B * CH * MW * 4), (fbig, B * 4), (tbig, S * CH * CW)):
        _tail_is_untouched(big, used)
    return (mask.cpu().numpy().view(np.uint32).reshape(B, CH, MW), flags.cpu().numpy(),
            life.cpu().numpy().reshape(S, CH, CW) if hold else None)


def _expect_cells(case, S, T, cell, hold, ttl=None, idx=None, kp_mask=RC.HEAD, fallback=R.FALLBACK_PERSON, margin=0.25, fmt="nv12"):
    pick = (lambda a: a) if idx is None else (lambda a: a[idx])
    CH, CW, _ = R.grid_of(RC.PICTURES[fmt], cell)
    ttl = np.zeros((S, CH, CW), np.uint8) if ttl is None else ttl
    return R.cells(pick(case.count), pick(case.kp_cell), pick(case.bbox), ttl, S, T,
                   **RC.cells_args(fmt, cell, kp_mask, fallback, margin, hold))


def _same_cells(got, exp, what):
    assert np.array_equal(got[0], exp[0]), (what, "mask", np.argwhere(got[0] != exp[0]).tolist()[:8])
    assert np.array_equal(got[1], exp[1]), (what, "flags", got[1].tolist(), exp[1].tolist())
    assert (got[2] is None) == (exp[2] is None) and (got[2] is None or np.array_equal(got[2], exp[2])), (what, "ttl")


PEOPLE = {"planted": (RC.planted, RC.FRAMES, 1), "random-11": (lambda: RC.random_people(11), 1, RC.FRAMES),
          "random-12": (lambda: RC.random_people(12), RC.FRAMES, 1), "hold-sequence": (RC.hold_sequence, RC.STREAMS, RC.STEPS)}


@pytest.mark.parametrize("hold", RC.HOLDS)
@pytest.mark.parametrize("cell", RC.CELLS)
def test_redact_cells_match_the_restatement(cell, hold):
    CH, CW, MW = R.grid_of(RC.PICTURES["nv12"], cell)
    flagged = False
    for name, (build, S, T) in PEOPLE.items():
        case = build()
        stale = np.random.default_rng(cell + hold).integers(1, 6, (S, CH, CW)).astype(np.uint8)      # a state in mid count
        for kw in (dict(), dict(kp_mask=RC.PERSON, margin=0.0), dict(fallback=R.FALLBACK_NONE, ttl=stale),
                   dict(kp_mask=1 << RC.ANKLE | 1 << 31, margin=0.5)):
            got, exp = _run_cells(case, S, T, cell, hold, **kw), _expect_cells(case, S, T, cell, hold, **kw)
            _same_cells(got, exp, (name, kw))
            if CW % 32:                                                      # the canary's bits at and above CW are gone
                assert not (got[0][:, :, -1] >> np.uint32(CW % 32)).any()
            flagged = flagged or bool(exp[1].any())
            assert name != "planted" or exp[0].any()
    assert flagged


@pytest.mark.parametrize("fmt", ["yuyv", "bgr"])
def test_redact_cells_on_the_odd_pictures(fmt):
    case = RC.planted()
    for cell in RC.CELLS:
        _same_cells(_run_cells(case, RC.FRAMES, 1, cell, 1, fmt=fmt), _expect_cells(case, RC.FRAMES, 1, cell, 1, fmt=fmt), (fmt, cell))


@pytest.mark.parametrize("hold", RC.HOLDS)
def test_one_call_equals_frame_by_frame_equals_two_uneven_calls(hold):
    case, S, T = RC.hold_sequence(), RC.STREAMS, RC.STEPS
    whole = _run_cells(case, S, T, 16, hold)
    _same_cells(whole, _expect_cells(case, S, T, 16, hold), "whole")
    assert whole[0].any() and len({whole[0][t].tobytes() for t in range(T)}) > 1
    for cuts in ([1] * T, [2, 3]):
        ttl, t0, masks, flags = None, 0, [], []
        for n in cuts:
            idx = [s * T + t0 + t for s in range(S) for t in range(n)]
            m, f, ttl = _run_cells(case, S, n, 16, hold, ttl=ttl, idx=idx)
            masks.append(m.reshape(S, n, *m.shape[1:]))
            flags.append(f.reshape(S, n))
            t0 += n
        m, f = np.concatenate(masks, axis=1), np.concatenate(flags, axis=1)
        _same_cells((m.reshape(whole[0].shape), f.reshape(-1), ttl), whole, cuts)


class _Crowd:
    """`counts[f]` random people (of `M` slots, a third without neck and top, a share `rooted` with a root) per frame, in
    RC.COORDS_HW."""

    def __init__(self, counts, M, seed, rooted=1.0):
        rng = np.random.default_rng(seed)
        self.frames = len(counts)
        self.count = np.array(counts, np.int32)
        centre = rng.uniform(0, RC.COORDS_HW, (self.frames, M, 1, 2))
        half = rng.uniform(0.05, 0.6, (self.frames, M, RC.K, 2))
        mid = centre + rng.uniform(-1, 1, (self.frames, M, RC.K, 2))
        self.bbox = np.concatenate([mid - half, mid + half], -1).astype(np.float32)
        self.kp_cell = np.zeros((self.frames, M, RC.K), np.int32)
        self.kp_cell[rng.random((self.frames, M)) < 1 / 3, RC.NECK:RC.TOP + 1] = -1
        self.kp_cell[rng.random((self.frames, M)) >= rooted, 0] = -1
        self.score = np.ones((self.frames, M, RC.K), np.float32)


@pytest.mark.parametrize("hold", [0, 2])
def test_redact_cells_take_the_frames_of_a_call_in_groups(hold):
    """The kernel stages as many consecutive frames as hold 1024 people together, at most 64: 600 + 400 + 24 people fill
    the table exactly, the next 600 start a group, 1000 + 25 do not fit; and 70 quiet frames are more than one group."""
    crowd = _Crowd([600, 400, 24, 600, 1000, 25, 0, 3], 1000, 31, rooted=0.01)   # few take part: the masks stay sparse
    exp = _expect_cells(crowd, 2, 4, 8, hold)
    _same_cells(_run_cells(crowd, 2, 4, 8, hold), exp, "crowd")
    assert all(exp[0][b].any() and not (exp[0][b, :, :2] == 0xffffffff).all() for b in (0, 1, 3, 4))
    many = _Crowd([f % 4 for f in range(140)], 3, 32)
    got = _run_cells(many, 2, 70, 8, hold)
    _same_cells(got, _expect_cells(many, 2, 70, 8, hold), "70 frames")
    assert got[0][69].any() and got[0][139].any()


def test_redact_cells_twice_give_the_same_bytes():
    case = RC.random_people(13)
    a, b = (_run_cells(case, 1, RC.FRAMES, 8, 3) for _ in range(2))
    _same_cells(a, b, "twice")


# ---- ppn_redact_yuv -----------------------------------------------------------------------------------------------------
def _host_frames(fmt, seed, pitch):
    """Random frames whose bytes between a row's content and its pitch (and behind the last plane) are canaries."""
    h, w = RC.PICTURES[fmt]
    host = RC.frames_of(fmt, seed, pitch, extra=5)
    pad = np.ones(host.shape[1], bool)
    pad[R.content_offsets(fmt, h, w, pitch)] = False
    host[:, pad] = CANARY
    return host, pad


def _placed(host, stride, misalign):
    """The frames inside a canary buffer: (buffer, view u8 [F, nbytes] with frame stride `stride` at an address that is
    `misalign` modulo 4)."""
    F_, n = host.shape
    big = torch.full((F_ * stride + 136,), CANARY, dtype=torch.uint8, device="cuda")
    base = 64 + (misalign - (big.data_ptr() + 64)) % 4
    view = big[base:base + F_ * stride].view(F_, stride)[:, :n]
    assert view.data_ptr() % 4 == misalign and view.stride(0) == stride
    view.copy_(torch.from_numpy(host))
    return big, view


def _surface(fmt, view, pitch):
    from pytorch_pose_proposal_network_amd import lib as L
    h, w = RC.PICTURES[fmt]
    base, pc = view.data_ptr(), pitch // 2
    u = {"nv12": base + h * pitch, "i420": base + h * pitch}.get(fmt)
    v = base + h * pitch + (h // 2) * pc if fmt == "i420" else None
    return L.YuvSurface(format=FORMATS.index(fmt), height=h, width=w, pitch=pitch, pitch_c={"nv12": pitch, "i420": pc}.get(fmt, 0),
                        frame_stride=view.stride(0), y=base, u=u, v=v, matrix=0, full_range=0)


def _redact(fmt, cell, mode, fill, src, dst, mask, pitch):
    from pytorch_pose_proposal_network_amd import lib as L
    cfg = L.RedactCfg(cell, mode, (C.c_uint8 * 4)(*fill, 0xEE))
    dmask = torch.from_numpy(mask.view(np.int32)).cuda()
    L.check(L.load().ppn_redact_yuv(C.byref(cfg), C.byref(_surface(fmt, src, pitch)), C.byref(_surface(fmt, dst, pitch)), src.shape[0],
                                    dmask.data_ptr(), L.current_stream_ptr()), "ppn_redact_yuv")


def _whole(big, view):
    """(the buffer's bytes, the boolean index of the view's bytes in it), both NumPy."""
    all_ = big.cpu().numpy()
    inside = np.zeros(all_.size, bool)
    off = view.data_ptr() - big.data_ptr()
    for f in range(view.shape[0]):
        inside[off + f * view.stride(0):off + f * view.stride(0) + view.shape[1]] = True
    return all_, inside


def _check_pair(fmt, cell, mode, fill, host, pad, mask, pitch, misalign, stride_extra):
    """In place and out of place on one placement: every byte of both buffers."""
    h, w = RC.PICTURES[fmt]
    exp = R.redact_frames(host, fmt, h, w, mask, cell, mode, fill, pitch)
    n = host.shape[1]
    # in place
    big, view = _placed(host, n + stride_extra[0], misalign[0])
    _redact(fmt, cell, mode, fill, view, view, mask, pitch)
    got, inside = _whole(big, view)
    assert np.array_equal(got[inside].reshape(host.shape), exp), (fmt, cell, "in place", int((got[inside].reshape(host.shape) != exp).sum()))
    assert (got[~inside] == CANARY).all() and (got[inside].reshape(host.shape)[:, pad] == CANARY).all()
    # a second application is the identity
    _redact(fmt, cell, mode, fill, view, view, mask, pitch)
    assert np.array_equal(_whole(big, view)[0], got)
    # out of place: the source keeps its bytes, the destination gets the content and nothing else
    sbig, src = _placed(host, n + stride_extra[0], misalign[0])
    dbig, dst = _placed(np.full_like(host, CANARY), n + stride_extra[1], misalign[1])
    _redact(fmt, cell, mode, fill, src, dst, mask, pitch)
    sgot, sin = _whole(sbig, src)
    assert np.array_equal(sgot[sin].reshape(host.shape), host) and (sgot[~sin] == CANARY).all()
    dgot, din = _whole(dbig, dst)
    frames = dgot[din].reshape(host.shape)
    assert np.array_equal(frames[:, ~pad], exp[:, ~pad]), (fmt, cell, "out of place", int((frames[:, ~pad] != exp[:, ~pad]).sum()))
    assert (frames[:, pad] == CANARY).all() and (dgot[~din] == CANARY).all()
    return exp


@pytest.mark.parametrize("mode", [R.MOSAIC, R.FILL], ids=["mosaic", "fill"])
@pytest.mark.parametrize("cell", RC.CELLS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_redact_yuv_matches_the_restatement_on_both_store_paths(fmt, cell, mode):
    fill = (201, 77, 140)
    mask = RC.random_mask(fmt, cell, 20 + cell)                              # garbage in the bits at and above CW
    CW = R.grid_of(RC.PICTURES[fmt], cell)[1]
    assert (mask[:, :, -1] >> np.uint32(CW % 32)).any()
    mask[0, -1, -1] |= np.uint32(1 << ((CW - 1) & 31))                       # the partial corner cell
    # a padded pitch, odd plane addresses, a frame stride above the frame: bytes
    pitch = RC.padded_pitch(fmt)
    host, pad = _host_frames(fmt, 30 + cell, pitch)
    exp = _check_pair(fmt, cell, mode, fill, host, pad, mask, pitch, (1, 3), (13, 7))
    assert (exp != host).any()
    # everything a multiple of 4: dwords
    pitch = ALIGNED_PITCH[fmt]
    host, pad = _host_frames(fmt, 31 + cell, pitch)
    host = np.ascontiguousarray(host[:, :host.shape[1] // 4 * 4])
    _check_pair(fmt, cell, mode, fill, host, pad[:host.shape[1]], mask, pitch, (0, 0), (12, 24))
    # the same aligned source beside a destination at an address that is 2 modulo 4: bytes again
    _check_pair(fmt, cell, mode, fill, host, pad[:host.shape[1]], mask, pitch, (0, 2), (12, 24))


@pytest.mark.parametrize("fmt", FORMATS)
def test_redact_yuv_all_zero_garbage_only_and_all_ones_masks(fmt):
    h, w = RC.PICTURES[fmt]
    CH, CW, MW = R.grid_of((h, w), 16)
    pitch = RC.padded_pitch(fmt)
    host, pad = _host_frames(fmt, 40, pitch)
    zero = np.zeros((RC.FRAMES, CH, MW), np.uint32)
    junk = zero.copy()
    junk[:, :, -1] = np.uint32((0xffffffff << (CW % 32)) & 0xffffffff)        # only bits that no cell owns
    for mask in (zero, junk):
        exp = _check_pair(fmt, 16, R.MOSAIC, (0, 0, 0), host, pad, mask, pitch, (1, 2), (5, 9))
        assert np.array_equal(exp, host)                                     # in place: untouched; out of place: a copy
    ones = np.full_like(zero, 0xffffffff)
    exp = _check_pair(fmt, 16, R.MOSAIC, (0, 0, 0), host, pad, ones, pitch, (3, 0), (5, 9))
    assert (exp[:, ~pad] != host[:, ~pad]).mean() > 0.9


# ---- Redactor -----------------------------------------------------------------------------------------------------------
def _expected_run(case, host, fmt, S, T, ttl, cell, hold, mode=R.MOSAIC, fill=(0, 0, 0), **kw):
    """(redacted frames, mask, flags, ttl') of the restatement."""
    h, w = RC.PICTURES[fmt]
    mask, flags, ttl = _expect_cells(case, S, T, cell, hold, ttl=ttl, fmt=fmt, **kw)
    return R.redact_frames(host, fmt, h, w, mask, cell, mode, fill), mask, flags, ttl


def _state(red):
    return (red.mask.cpu().numpy().view(np.uint32), red.flags.cpu().numpy(), red.ttl.cpu().numpy())


@pytest.mark.parametrize("fmt,cell,opts", [
    ("nv12", 16, dict()), ("i420", 8, dict(parts="person", margin=0.0)),
    ("yuyv", 32, dict(mode="fill", fill_rgb=(200, 30, 90), fallback="none", matrix="bt709", full_range=True)),
    ("bgr", 16, dict(mode="fill", fill_rgb=(1, 2, 3), parts=("left_ankle", "top")))])
def test_redactor_equals_the_restatement(fmt, cell, opts):
    from pytorch_pose_proposal_network_amd import redact
    case, S, T = RC.hold_sequence(), RC.STREAMS, RC.STEPS
    h, w = RC.PICTURES[fmt]
    host = RC.frames_of(fmt, 50 + cell, frames=S * T)
    raw = torch.from_numpy(host).cuda()
    if fmt == "bgr":
        raw = raw.view(S * T, h, w, 3)
    red = redact.Redactor(S, T, RC.M, (h, w), fmt, cell=cell, hold=3, coords_hw=RC.COORDS_HW, K=RC.K, **opts)
    kw = dict(kp_mask=redact.kp_mask_of(opts.get("parts", "head"), RC.K), margin=opts.get("margin", 0.25),
              fallback=R.FALLBACK_NONE if opts.get("fallback") == "none" else R.FALLBACK_PERSON)
    mode = R.FILL if opts.get("mode") == "fill" else R.MOSAIC
    fill = R.fill_bytes(fmt, opts.get("fill_rgb", (0, 0, 0)), opts.get("matrix", "bt601"), opts.get("full_range", False))
    assert red.fill == fill
    ttl = None
    for turn in range(2):                                                    # the second call starts from the first's state
        exp, mask, flags, ttl = _expected_run(case, host, fmt, S, T, ttl, cell, 3, mode, fill, **kw)
        out = red(raw, _result(case))                                        # out=None: a new tensor
        assert out.shape == raw.shape and out.data_ptr() != raw.data_ptr()
        assert np.array_equal(out.cpu().numpy().reshape(host.shape), exp), (fmt, turn)
        assert np.array_equal(raw.cpu().numpy().reshape(host.shape), host)
        got = _state(red)
        assert np.array_equal(got[0], mask) and np.array_equal(got[1], flags) and np.array_equal(got[2], ttl)
        assert mask.any() and (exp != host).any()
    other = torch.full_like(raw, CANARY)
    assert red.apply(raw, out=other).data_ptr() == other.data_ptr()          # out of place, the masks as they are
    assert np.array_equal(other.cpu().numpy().reshape(host.shape), exp)
    assert red.apply(raw, out=raw).data_ptr() == raw.data_ptr()              # in place
    assert np.array_equal(raw.cpu().numpy().reshape(host.shape), exp)
    red.reset()
    assert not red.ttl.any()
    raw.copy_(torch.from_numpy(host).view(raw.shape))
    exp0 = _expected_run(case, host, fmt, S, T, None, cell, 3, mode, fill, **kw)
    assert np.array_equal(red(raw, _result(case)).cpu().numpy().reshape(host.shape), exp0[0])
    assert np.array_equal(_state(red)[2], exp0[3])
    one = redact.redact_people_yuv(raw, fmt, (h, w), _result(case), streams=S, cell=cell, hold=3, coords_hw=RC.COORDS_HW, K=RC.K, **opts)
    assert np.array_equal(one.cpu().numpy().reshape(host.shape), exp0[0])


def test_cells_then_apply_under_graph_capture_carry_the_hold_state():
    from pytorch_pose_proposal_network_amd import redact
    fmt, cell, hold, S = "nv12", 16, 3, RC.FRAMES
    h, w = RC.PICTURES[fmt]
    people = [RC.planted(), RC.random_people(21), RC.random_people(22), RC.planted()]
    hosts = [RC.frames_of(fmt, 60 + i) for i in range(len(people))]
    make = lambda: redact.Redactor(S, 1, RC.M, (h, w), fmt, cell=cell, hold=hold, coords_hw=RC.COORDS_HW, K=RC.K)
    staged, raw = _result(people[0]), torch.from_numpy(hosts[0]).cuda()
    out = torch.empty_like(raw)
    red = make()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        make()(raw, staged, out=out)                                         # the module is loaded outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                # two launches in a row: a linear graph
        red(raw, staged, out=out)
    red.reset()                                                              # a capture runs nothing; start from a fresh state
    ttl = None
    for case, host in zip(people, hosts):
        for t in (red.mask, red.flags, out):
            t.view(torch.uint8).fill_(CANARY)
        for k in ("count", "kp_cell", "bbox", "score"):                      # the people and the frames change in place
            getattr(staged, k).copy_(torch.from_numpy(np.array(getattr(case, k))))
        raw.copy_(torch.from_numpy(host))
        g.replay()
        torch.cuda.synchronize()
        exp, mask, flags, ttl = _expected_run(case, host, fmt, S, 1, ttl, cell, hold)
        got = _state(red)
        assert np.array_equal(got[0], mask) and np.array_equal(got[1], flags) and np.array_equal(got[2], ttl)
        assert np.array_equal(out.cpu().numpy(), exp)
    fresh = _expected_run(people[-1], hosts[-1], fmt, S, 1, None, cell, hold)
    assert not np.array_equal(fresh[1], mask)                                # the last frame's masks held cells of earlier frames


def test_redactor_checks_its_input():
    from pytorch_pose_proposal_network_amd import decode as D, redact
    case = RC.planted()
    h, w = RC.PICTURES["nv12"]
    red = redact.Redactor(RC.FRAMES, 1, RC.M, (h, w), "nv12", coords_hw=RC.COORDS_HW, K=RC.K)
    good = _result(case)
    raw = torch.from_numpy(RC.frames_of("nv12", 70)).cuda()
    red(raw, good)
    bad = [D.DecodeResult(good.count, good.kp_cell, good.limb_arg, good.bbox, good.score, RC.M + 1),
           D.DecodeResult(good.count[:2], good.kp_cell, good.limb_arg, good.bbox, good.score, RC.M),
           D.DecodeResult(good.count, good.kp_cell[:, :, :4], good.limb_arg, good.bbox, good.score, RC.M),
           D.DecodeResult(good.count, good.kp_cell, good.limb_arg, good.bbox.double(), good.score, RC.M),
           D.DecodeResult(good.count, good.kp_cell, good.limb_arg, good.bbox.cpu(), good.score, RC.M)]
    for res in bad:
        with pytest.raises(ValueError):
            red.cells(res)
    for wrong in (raw[:2], raw.cpu(), raw.float(), raw[:, :100], None):
        with pytest.raises(ValueError):
            red.apply(wrong)
    for out in (raw[:, 1:], raw.cpu(), torch.empty(RC.FRAMES, raw.shape[1] + 1, dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError):
            red.apply(raw, out=out)
    big = torch.zeros(raw.numel() + 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):                                          # overlaps raw's twin without being it
        red.apply(big[:raw.numel()].view(raw.shape), out=big[32:32 + raw.numel()].view(raw.shape))


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
def test_inference_redacted_equals_the_manual_composition(net, variant):
    from pytorch_pose_proposal_network_amd import redact, rt, track, windows as Wn
    h, w, F_ = 64, 96, 2
    host = np.random.default_rng(700).integers(0, 256, (F_, Y.frame_bytes("nv12", h, w)), dtype=np.uint8)
    raw = torch.from_numpy(host).cuda()
    lay = None if variant == "plain" else Wn.WindowLayout.tiles((h, w), 2, 2)
    M = 36 if lay is None else 4 * 36
    space = (96, 96) if lay is None else (h, w)
    make = lambda **kw: redact.Redactor(1, F_, M, (h, w), "nv12", cell=8, parts="person", hold=2, **dict(dict(coords_hw=space), **kw))
    red = make()
    tracker = track.Tracker(1, F_, M) if variant == "windows-tracked" else None
    got = rt.inference_redacted(raw, "nv12", (h, w), net, red, layout=lay, tracker=tracker, size=96)
    assert len(got) == (3 if tracker else 2)
    res, out = got[0], got[1]
    assert out.shape == raw.shape and out.data_ptr() != raw.data_ptr() and torch.equal(raw.cpu(), torch.from_numpy(host))

    # the manual composition: the plain path or inference_windows, then a tracker and a redactor of one's own
    if lay is None:
        res2 = rt.inference_batch(rt.ingest_yuv(raw, "nv12", (h, w), size=96), net)
    else:
        res2 = rt.inference_windows(raw, "nv12", (h, w), net, lay, size=96)
    assert res2.max_humans == M
    _same_bytes(res.count, res2.count, "count")
    for f, n in enumerate(res2.count.cpu().tolist()):                        # the rows of people: a decode writes no others
        for k in ("kp_cell", "limb_arg", "bbox", "score"):
            _same_bytes(getattr(res, k)[f, :min(n, M)], getattr(res2, k)[f, :min(n, M)], (k, f))
    if tracker:
        tr2 = track.Tracker(1, F_, M).update(res2)
        _same_bytes(got[2].ids, tr2.ids, "ids")
        _same_bytes(got[2].hits, tr2.hits, "hits")
    red2 = make()
    out2 = red2(raw, res2)
    _same_bytes(out, out2, "frames")
    for k in ("mask", "flags", "ttl"):
        _same_bytes(getattr(red, k), getattr(red2, k), k)

    # and the restatement on the people that came out
    sy, sx = R.scales((h, w), space)
    mask, flags, ttl = R.cells(res.count.cpu().numpy(), res.kp_cell.cpu().numpy(), res.bbox.cpu().numpy(), np.zeros((1, 8, 12), np.uint8),
                               1, F_, (h, w), 8, sy, sx, (1 << 18) - 1, R.FALLBACK_PERSON, 0.25, 2)
    assert mask.any() and np.array_equal(red.mask.cpu().numpy().view(np.uint32), mask) and np.array_equal(red.ttl.cpu().numpy(), ttl)
    exp = R.redact_frames(host, "nv12", h, w, mask, 8)
    assert np.array_equal(out.cpu().numpy(), exp) and (exp != host).any()
    # in place, from the same state as the first call
    red3 = make()
    same = rt.inference_redacted(raw.clone(), "nv12", (h, w), net, red3, layout=lay, size=96)[1]
    assert np.array_equal(same.cpu().numpy(), exp)
    inplace = raw.clone()
    assert rt.inference_redacted(inplace, "nv12", (h, w), net, make(), layout=lay, size=96, out=inplace)[1].data_ptr() == inplace.data_ptr()
    assert np.array_equal(inplace.cpu().numpy(), exp)
    # a redactor that stands in another space, and a turned frame, are refused
    with pytest.raises(ValueError):
        rt.inference_redacted(raw, "nv12", (h, w), net, make(coords_hw=(50, 50)), layout=lay, size=96)
    with pytest.raises(ValueError):
        rt.inference_redacted(raw, "nv12", (h, w), net, make(), layout=lay, size=96, flip=True)
