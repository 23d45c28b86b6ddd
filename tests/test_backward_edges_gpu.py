"""The backward convolutions (csrc/wgrad.hip, csrc/stem_wgrad.hip, train.conv_dgrad with ppn_pack_weight_dgrad,
ppn_upsample_zero and the parity interleavers) against an f64 autograd reference on the cases of tests/backward_cases.py:
off-square images, several pixel splits with a ragged last one, the fold kernel's tail, idle work-groups, one-pixel-wide
outputs, the stem kernels' persistent loop, ragged channels, stride-2 remainders on one axis -- and one off-square training
iteration against the CPU oracle.

Tolerances are the project's own (tests/test_train_gpu.py): dW to 3e-5 * sqrt(B * Ho * Wo) absolute, dX to 3e-5 (f32) / 2e-2
(bf16) of max(1, max |ref|) in max norm, plus a per-element bound on dX that an error confined to small border values cannot
hide behind (backward_cases.dgrad_tols).  Every test prints what it measured next to its bound (lines starting BWD_EDGE;
profiles/backward_edge_errors.txt holds one run's)."""
import numpy as np
import pytest
import torch

import backward_cases as BC

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _run_wgrad(tag, table, name, dtype, c, parts):
    from pytorch_pose_proposal_network_amd import train as T
    dev = torch.device("cuda")
    x, dy = (t.to(dev) for t in BC.wgrad_operands(table, name, dtype))
    ref = BC.wgrad_ref(table, name, dtype)
    pre = torch.randn(c.co, c.ci, c.k, c.k, generator=torch.Generator().manual_seed(17))        # a non-constant `out`
    dw = T.conv_wgrad(x, dy, c.k, c.s, c.dil, c.pad)
    acc = T.conv_wgrad(x, dy, c.k, c.s, c.dil, c.pad, out=pre.to(dev), accumulate=True)
    again = T.conv_wgrad(x, dy, c.k, c.s, c.dil, c.pad)
    torch.cuda.synchronize()
    tol = BC.wgrad_tol(c)
    e0 = float((dw.cpu().double() - ref).abs().max())
    e1 = float((acc.cpu().double() - pre.double() - ref).abs().max())
    same = torch.equal(_bits(dw), _bits(again))
    print(f"BWD_EDGE {tag} {name} {dtype}: {parts}, max|ref| {float(ref.abs().max()):.2f}, err {e0:.3e}, accumulate err "
          f"{e1:.3e}, tol {tol:.3e}, second run {'bitwise equal' if same else 'DIFFERS'}")
    assert dw.shape == ref.shape and torch.isfinite(dw).all()
    assert e0 <= tol, (e0, tol)
    assert e1 <= tol, (e1, tol)
    if dtype == "bf16":
        assert same                      # no atomics, a fixed fold order: run-to-run reproducible


@pytest.mark.parametrize("name,dtype", BC.wgrad_runs())
def test_generic_wgrad(name, dtype):
    """wgrad_kernel (128 / 256 tile, f32 / bf16) + wgrad_fold_kernel; the split count comes from the library and is held
    to what the case is for, so that a retuned geometry() cannot silently empty it."""
    c, _ = BC.WGRAD_CASES[name]
    nsplit = BC.partials(c, dtype)
    assert BC.check_wgrad_purpose(name, dtype, nsplit) is None
    _run_wgrad("wgrad", "wgrad", name, dtype, c, f"nsplit {nsplit}, items {BC.wgrad_items(c, nsplit)}")


@pytest.mark.parametrize("name", list(BC.STEM_CASES))
def test_stem_wgrad(name):
    """stem_wgrad_kernel x 3 and stem_wgrad7_kernel: the persistent loop with one and two tiles per work-group (grid ==
    cap < tiles), and a tall image below the cap."""
    c = BC.STEM_CASES[name]
    grid, tiles, cap = BC.partials(c, "bf16"), BC.stem_tiles(c), BC.stem_cap(c)
    if name.endswith("/persistent"):
        assert grid == cap and cap < tiles < 2 * cap, (grid, tiles, cap)
    else:
        assert grid == tiles < cap, (grid, tiles, cap)
    _run_wgrad("stem_wgrad", "stem", name, "bf16", c, f"grid {grid}, tiles {tiles}")


def _check_dgrad(tag, dtype, got, ref):
    """Max-norm and per-element bounds; returns the list of failures."""
    if tuple(got.shape) != tuple(ref.shape):
        return [f"{tag} {dtype}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"]
    mx, rel, ab = BC.dgrad_tols(dtype)
    scale = max(1.0, float(ref.abs().max()))
    err = (got.cpu().double() - ref).abs()
    bound = rel * ref.abs() + ab * scale
    worst = float((err / bound).max())
    print(f"BWD_EDGE dgrad {tag} {dtype}: max|ref| {float(ref.abs().max()):.3f}, max err {float(err.max()):.3e} (tol {mx * scale:.3e}), "
          f"worst err / per-element bound {worst:.3f}")
    bad = []
    if not float(err.max()) <= mx * scale:
        bad.append(f"{tag} {dtype}: max err {float(err.max()):.3e} > {mx * scale:.3e}")
    if not bool((err <= bound).all()):
        i = int((err / bound).argmax())
        bad.append(f"{tag} {dtype}: element {np.unravel_index(i, ref.shape)}: got {got.cpu().double().flatten()[i]!r}, "
                   f"ref {ref.flatten()[i]!r}, {worst:.2f} x its bound")
    return bad


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(BC.DGRAD_CASES))
def test_conv_dgrad(name, dtype):
    """train.conv_dgrad end to end, with and without a skip-path gradient to add.  Stride 2: the input pixels no output
    reads hold `add` (or zero) exactly.  Paths by case: cin <= 16 3x3 -> stacked parity (f32, or no add) / zero-upsampled
    (bf16 + add); cin > 16 3x3 -> zero-upsampled; 1x1 -> half-resolution convolution + ppn_upsample_zero (f32, or no add) /
    zero-upsampled.  The torch copies that train.py keeps for pixels of cin * elemsize % 16 != 0 bytes cannot be reached
    through conv_dgrad: the convolution kernels take channel counts that are multiples of 8 only (16 bytes in bf16), so
    test_data_movement_off_square calls upsample_zero on such a tensor directly.  ragged/d4 has a cout (72) that is neither
    a multiple of the convolution's K step nor a power of two: conv_dgrad pads it with zero channels."""
    from pytorch_pose_proposal_network_amd import train as T
    c = BC.DGRAD_CASES[name]
    dev = torch.device("cuda")
    dy, w, add = BC.dgrad_operands(name, dtype)
    ref = BC.dgrad_ref(name, dtype)
    dyd, wd, addd = dy.to(dev), w.to(dev), add.to(dev)
    with_add = T.conv_dgrad(dyd, wd, (c.H, c.W), c.s, c.dil, c.pad, add=addd)
    plain = T.conv_dgrad(dyd, wd, (c.H, c.W), c.s, c.dil, c.pad)
    torch.cuda.synchronize()
    assert torch.equal(addd.cpu(), add)                        # the operand is not written
    bad = _check_dgrad(f"{name} +add", dtype, with_add, ref + add.double())
    bad += _check_dgrad(f"{name}", dtype, plain, ref)
    if c.s == 2:
        idle = torch.from_numpy(~BC.touched(c))
        assert bool((ref[:, idle] == 0).all())
        if not torch.equal(_bits(with_add.cpu()[:, idle]), _bits(add[:, idle])):
            bad.append(f"{name} {dtype}: pixels without a gradient differ from `add`")
        if not bool((plain.cpu()[:, idle] == 0).all()):
            bad.append(f"{name} {dtype}: pixels without a gradient are not zero")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["s2/3x3/ci64", "s2/3x3/ci16", "s2/3x3/ci16/t"])
def test_stride2_parity_forms(name, dtype, monkeypatch):
    """train._dgrad_stride2 called directly -- conv_dgrad sends only cin <= 16 there for a 3x3, so the four-launch form with
    ppn_interleave_parity is reached with cin = 64 (and with cin = 16 by switching the stacked form off) -- and the
    zero-upsampled form with the parity forms switched off: all against the f64 reference, and equal to each other."""
    from pytorch_pose_proposal_network_amd import train as T
    c = BC.DGRAD_CASES[name]
    dev = torch.device("cuda")
    dy, w, add = BC.dgrad_operands(name, dtype)
    ref = BC.dgrad_ref(name, dtype)
    dyd, wd = dy.to(dev), w.to(dev)
    bad = []
    stacked = T._dgrad_stride2(dyd, wd, c.H, c.W, None)
    bad += _check_dgrad(f"{name} _dgrad_stride2", dtype, stacked, ref)
    monkeypatch.setattr(T, "_S2_STACKED", False)
    four = T._dgrad_stride2(dyd, wd, c.H, c.W, None)
    bad += _check_dgrad(f"{name} four launches", dtype, four, ref)
    monkeypatch.setattr(T, "_S2_PARITY", False)
    up = T.conv_dgrad(dyd, wd, (c.H, c.W), 2, 1, 1)
    bad += _check_dgrad(f"{name} zero-upsampled", dtype, up, ref)
    torch.cuda.synchronize()
    # what tests/test_train_gpu.py holds the forms to on square images: the same numbers
    assert torch.equal(stacked, four) and torch.equal(four, up)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_data_movement_off_square(dtype):
    """ppn_upsample_zero, ppn_interleave_parity and ppn_interleave_parity_stacked against the torch indexing they replace
    (bitwise), H odd with W even and the reverse, one pixel wide, and one tensor large enough for the grid-stride loop
    (more than 4096 x 256 items)."""
    from pytorch_pose_proposal_network_amd import train as T, lib as L
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(4)
    tdt = BC.DTYPES[dtype]
    code = L.PPN_F32 if dtype == "f32" else L.PPN_BF16
    lib, st = L.load(), L.current_stream_ptr()
    #                                  B  h   w   ch  s  dst_h dst_w
    for (B, h, w, ch, s, dh, dw) in [(2, 5, 8, 16, 2, 9, 16), (2, 8, 5, 16, 2, 16, 9), (1, 7, 4, 8, 2, 13, 8), (3, 1, 9, 32, 2, 1, 18),
                                      (2, 9, 1, 8, 2, 18, 1), (2, 4, 7, 8, 3, 11, 20), (2, 151, 150, 64, 2, 301, 300)]:
        src = torch.randn(B, h, w, ch, generator=g).to(tdt).to(dev)
        want = torch.zeros(B, dh, dw, ch, dtype=tdt, device=dev)
        want[:, ::s, ::s][:, :h, :w] = src
        assert torch.equal(_bits(T.upsample_zero(src, s, dh, dw)), _bits(want)), (B, h, w, ch, s)
    # a pixel that is no multiple of 16 bytes takes the torch path inside train.upsample_zero; the kernel refuses it
    src = torch.randn(2, 3, 4, 4, generator=g).to(torch.bfloat16).to(dev)
    want = torch.zeros(2, 5, 8, 4, dtype=torch.bfloat16, device=dev)
    want[:, ::2, ::2] = src
    assert torch.equal(T.upsample_zero(src, 2, 5, 8), want)
    assert lib.ppn_upsample_zero(L.PPN_BF16, src.data_ptr(), 2, 3, 4, 4, 2, 5, 8, want.data_ptr(), st) != 0
    for (B, H, W, ch) in [(2, 9, 12, 16), (2, 12, 9, 16), (1, 7, 10, 8), (3, 10, 7, 32), (2, 5, 1, 8), (1, 1, 6, 8), (2, 301, 300, 64)]:
        Ho1, Wo1 = (H + 2 - 3) // 2 + 2, (W + 2 - 3) // 2 + 2
        o4 = torch.randn(B, Ho1, Wo1, 4 * ch, generator=g).to(tdt).to(dev)                # channel block 2 py + px
        o = [[o4[..., (2 * py + px) * ch:(2 * py + px + 1) * ch].contiguous() for px in (0, 1)] for py in (0, 1)]
        want = torch.full((B, H, W, ch), 7.0, dtype=tdt, device=dev)
        for py in (0, 1):
            for px in (0, 1):
                ny, nx = (H - py + 1) // 2, (W - px + 1) // 2
                if ny > 0 and nx > 0:
                    want[:, py::2, px::2] = o[py][px][:, py:py + ny, px:px + nx]
        dx = torch.full_like(want, -3.0)
        L.check(lib.ppn_interleave_parity(code, o[0][0].data_ptr(), o[0][1].data_ptr(), o[1][0].data_ptr(), o[1][1].data_ptr(),
                                          B, H, W, ch, dx.data_ptr(), st), "interleave")
        assert torch.equal(_bits(dx), _bits(want)), (B, H, W, ch)
        dx = torch.full_like(want, -3.0)
        L.check(lib.ppn_interleave_parity_stacked(code, o4.data_ptr(), B, H, W, ch, dx.data_ptr(), st), "interleave stacked")
        assert torch.equal(_bits(dx), _bits(want)), (B, H, W, ch)
    torch.cuda.synchronize()


def _rel(a, b):
    """tests/test_trainer_gpu.py's measure: relative L2 error, absolute where the exact value is ~0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(1e-4, np.sqrt((b ** 2).sum())))


def test_trainer_off_square_f32_matches_oracle():
    """One DRN-D-22 iteration on 112 x 80 images (a grid of 7 rows x 5 columns): head, losses and every parameter gradient
    against the f64 CPU oracle, by test_trainer_other_basicblock_depth's criterion."""
    from pytorch_pose_proposal_network_amd import lib as L
    from pytorch_pose_proposal_network_amd.trainer import PPNTrainer
    sd, x, tg = BC.train_inputs()
    torch.set_num_threads(8)
    r64, r32 = BC.train_ref("f64"), BC.train_ref("f32")
    assert r64["head"].shape[2:] == (BC.TRAIN_H // 16, BC.TRAIN_W // 16) == (7, 5)
    dev = torch.device("cuda")
    tr = PPNTrainer(BC.TRAIN_ARCH, sd, compute_dtype=L.PPN_F32, insize=BC.TRAIN_INSIZE)
    head = tr.forward(torch.as_tensor(x).to(dev))
    assert tuple(head.shape) == r64["head"].shape
    ehead = float(np.abs(head.cpu().numpy() - r64["head"]).max())
    tgd = {k: torch.from_numpy(v).to(dev) for k, v in tg.items()}
    losses, gh = tr.criterion.forward_backward(head, tgd, coeff=[0.2] * 5)
    tr.backward(gh)
    torch.cuda.synchronize()
    rows = [(n, _rel(tr.G[n].cpu().numpy(), r64["grads"][n]), _rel(r32["grads"][n], r64["grads"][n])) for n in tr.param_names]
    worst = max(rows, key=lambda r: r[1] / max(3 * r[2], 1e-2))
    print(f"BWD_EDGE trainer f32 {BC.TRAIN_H}x{BC.TRAIN_W}: head max err {ehead:.2e} (tol 1e-4), losses rel err "
          f"{float(np.abs(losses.cpu().numpy() / r64['losses'] - 1).max()):.2e} (tol 1e-4), worst gradient {worst[0]}: rel L2 err "
          f"{worst[1]:.2e}, oracle f32 noise {worst[2]:.2e}, bound {max(3 * worst[2], 1e-2):.2e}")
    assert ehead <= 1e-4
    assert np.allclose(losses.cpu().numpy(), r64["losses"], rtol=1e-4)
    assert len(tr.param_names) == len(r64["grads"])
    bad = [r for r in rows if r[1] > max(3 * r[2], 1e-2)]
    assert not bad, bad[:6]


def test_trainer_off_square_bf16_tracks_f32():
    """The bf16 trainer on the same 112 x 80 input, by the criterion of test_bf16_gradients_track_f32."""
    from test_trainer_gpu import _check_bf16_gradients_track_f32
    sd, x, tg = BC.train_inputs()
    dev = torch.device("cuda")
    tgd = {k: torch.from_numpy(v).to(dev) for k, v in tg.items()}
    _check_bf16_gradients_track_f32(sd, torch.as_tensor(x).to(dev), tgd, BC.TRAIN_INSIZE)
