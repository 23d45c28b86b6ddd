"""The loss / target kernels (csrc/loss.hip, csrc/encode.hip, ppn_head_grad and ppn_gradnorm_probe_stats of csrc/train.hip)
against the f64 oracle on the cases of tests/loss_cases.py: off-square grids, H*W % 4 != 0 (the scalar instantiations),
limb windows other than 21x21, saturated heads, exact ties of the box edges, touching and disjoint boxes.

One tolerance for every comparison with f64 (loss_cases.tol):  err <= max(2e-5 * scale, 4 * e32), scale = |ref| for a loss
and the channel group's max|ref| for a gradient, e32 = what the oracle itself loses when it runs in f32 on that case.  Each
test prints err / e32 per group (lines starting LOSS_EDGE; profiles/loss_edge_errors.txt holds one run's)."""
import numpy as np
import pytest
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu

K = LC.K
ALL7 = ("mix", "e0", "e1", "e2", "e3", "e4", "zn")
SENTINEL = 123.25


def _crit(name):
    from pytorch_pose_proposal_network_amd import loss
    _, _, insize, outsize, local_grid = LC.build(name)
    return loss.PPNLoss(insize=insize, outsize=outsize, local_grid_size=local_grid)


def _dev(name):
    head, tg = LC.build(name)[:2]
    return LC.tt(head).cuda(), {k: LC.tt(v).cuda() for k, v in tg.items()}


def _limb_c(tg):
    return ((tg["te"] == 1).to(torch.uint8) | ((tg["weight_ij"] == 1).to(torch.uint8) << 1)).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nchw(x, Cn):
    """NHWC [B, H, W, cpad] device tensor -> f64 NumPy [B, Cn, H, W]."""
    return x[..., :Cn].permute(0, 3, 1, 2).double().cpu().numpy()


def _check_losses(tag, got, r):
    bad, parts = [], []
    got = got.double().cpu().numpy()
    for i in range(5):
        err, e32 = abs(got[i] - r["l64"][i]), float(r["e32_loss"][i])
        parts.append(f"{err / e32:.2f}" if e32 > 0 else ("0.00" if err == 0 else "inf"))
        if not err <= LC.tol(abs(r["l64"][i]), e32):
            bad.append(f"{tag} loss {i}: {got[i]!r} vs {r['l64'][i]!r}, e32 {e32:.3e}")
    print(f"LOSS_EDGE {tag}: losses err/e32 " + ", ".join(parts))
    return bad


def _col(v):
    return np.asarray(v, np.float64)[None, :, None, None]


@pytest.mark.parametrize("name", LC.CASES)
def test_forward_backward(name):
    """PPNLoss.forward_backward, coefficients by value and read on the device: five losses and the whole gradient."""
    crit = _crit(name)
    head, tg = _dev(name)
    bad = []
    for ckey in ALL7:
        r, coeff = LC.first_order(name, ckey), LC.COEFFS[ckey]
        l0, g0 = crit.forward_backward(head, tg, coeff)
        cw = torch.tensor([c * 4.0 for c in coeff], dtype=torch.float32).cuda()        # c_i = cw[i] / 4, exact
        l1, g1 = crit.forward_backward(head, tg, coeff_dev=(cw, 4.0))
        l2, none = crit.forward_backward(head, tg, want_grad=False)
        assert none is None and _same_bits(l0, l2) and _same_bits(l0, l1), (ckey, l0, l1, l2)
        bad += _check_losses(f"{name} {ckey} forward_backward", l0, r)
        bad += LC.check_groups(f"{name} {ckey} grad", g0.cpu().numpy(), r["g64"], r["e32"])
        bad += LC.check_groups(f"{name} {ckey} grad(coeff_dev)", g1.cpu().numpy(), r["g64"], r["e32"])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", LC.CASES)
def test_unary_backward(name):
    """PPNLoss.unary_backward = the first 6K channels of the oracle gradient with coeff[4] = 0; limb channels untouched."""
    crit = _crit(name)
    head, tg = _dev(name)
    bad = []
    for ckey in ("unary", "e1"):
        r = LC.first_order(name, ckey)
        out = torch.full_like(head, SENTINEL)
        assert crit.unary_backward(head, tg, LC.COEFFS[ckey][:4], out) is out
        torch.cuda.synchronize()
        assert bool((out[:, 6 * K:] == SENTINEL).all())
        bad += LC.check_groups(f"{name} {ckey} unary_backward", out[:, :6 * K].cpu().numpy(), r["g64"][:, :6 * K], r["e32"])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", LC.CASES)
def test_forward_backward_dz(name):
    """PPNLoss.forward_backward_dz: dz = grad * s (1 - s) as NHWC, zero padding channels, bias partial sums; bf16 = the f32
    run rounded to nearest even; compact limb targets = f32 limb targets."""
    crit = _crit(name)
    head, tg = _dev(name)
    Cn = head.shape[1]
    tgc = dict(tg, limb_c=_limb_c(tg))
    bad = []
    for ckey in ALL7:
        r, coeff = LC.first_order(name, ckey), LC.COEFFS[ckey]
        cw = torch.tensor([c * 4.0 for c in coeff], dtype=torch.float32).cuda()
        l, dz, dbsum = crit.forward_backward_dz(head, tg, (cw, 4.0), torch.float32)
        torch.cuda.synchronize()
        assert dz.shape[-1] % 64 == 0 and dz.shape[-1] >= Cn
        assert bool((_bits(dz[..., Cn:]) == 0).all()) and bool((_bits(dbsum[:, Cn:]) == 0).all())
        bad += _check_losses(f"{name} {ckey} forward_backward_dz", l, r)
        bad += LC.check_groups(f"{name} {ckey} dz", _nchw(dz, Cn), LC.dz64(name, ckey), r["e32_dz"])
        bad += LC.check_groups(f"{name} {ckey} dbsum", _col(dbsum.double().sum(0)[:Cn].cpu().numpy()), _col(r["db64"]),
                               r["e32_db"])
        if ckey in ("mix", "zn"):
            lb, dzb, dbb = crit.forward_backward_dz(head, tg, (cw, 4.0), torch.bfloat16)
            assert _same_bits(dzb, dz.to(torch.bfloat16)) and _same_bits(lb, l) and _same_bits(dbb, dbsum), ckey
            for dtype, want in ((torch.float32, (l, dz, dbsum)), (torch.bfloat16, (lb, dzb, dbb))):
                got = crit.forward_backward_dz(head, tgc, (cw, 4.0), dtype)
                assert all(_same_bits(a, b) for a, b in zip(got, want)), (ckey, dtype)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", LC.CASES)
def test_limb_dual_nhwc(name):
    """PPNLoss.limb_dual_nhwc against torch double backward of the limb loss alone (f64), NHWC; bf16 = RNE of f32."""
    crit = _crit(name)
    head, tg = _dev(name)
    Cn = head.shape[1]
    tz = LC.tt(LC.tangent(name)).cuda()
    r, c4 = LC.second_order(name, "limb"), LC.COEFFS["limb"][4]
    zb, tzb, zsum = crit.limb_dual_nhwc(head, tz, tg, c4, torch.float32)
    torch.cuda.synchronize()
    for x in (zb, tzb):
        assert bool((_bits(x[..., Cn:]) == 0).all()) and bool((x[..., :6 * K] == 0).all())
    assert bool((_bits(zsum[:, Cn:]) == 0).all())
    bad = LC.check_groups(f"{name} limb_dual_nhwc zb", _nchw(zb, Cn), r["zbar64"], r["e32_zbar"])
    bad += LC.check_groups(f"{name} limb_dual_nhwc tzb", _nchw(tzb, Cn), r["tzbar64"], r["e32_tzbar"])
    bad += LC.check_groups(f"{name} limb_dual_nhwc zsum", _col(zsum.double().sum(0)[:Cn].cpu().numpy()), _col(r["zsum64"]),
                           r["e32_zsum"])
    zbb, tzbb, zsb = crit.limb_dual_nhwc(head, tz, tg, c4, torch.bfloat16)
    assert _same_bits(zbb, zb.to(torch.bfloat16)) and _same_bits(tzbb, tzb.to(torch.bfloat16)) and _same_bits(zsb, zsum)
    tgc = dict(tg, limb_c=_limb_c(tg))
    for dtype, want in ((torch.float32, (zb, tzb, zsum)), (torch.bfloat16, (zbb, tzbb, zsb))):
        got = crit.limb_dual_nhwc(head, tz, tgc, c4, dtype)
        assert all(_same_bits(a, b) for a, b in zip(got, want)), dtype
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", LC.CASES)
def test_head_grad(name):
    """ppn_head_grad directly: dz[b, hw, c] = g[b, c, hw] * s (1 - s) in f64 for an f32 gradient g (the oracle's, rounded),
    with all channels + dbias and with channels_used < channels and no dbias."""
    from pytorch_pose_proposal_network_amd import lib as L
    head_np = LC.build(name)[0]
    B, Cn, H, W = head_np.shape
    g_np = LC.first_order(name, "mix")["g64"].astype(np.float32)
    s64 = head_np.astype(np.float64)
    ref = g_np.astype(np.float64) * (s64 * (1.0 - s64))
    ref32 = g_np * (head_np * (np.float32(1.0) - head_np))
    e32 = LC.group_e32(ref32, ref, Cn)
    db64 = ref.sum((0, 2, 3))
    e32_db = LC.group_e32(_col(ref32.sum((0, 2, 3), dtype=np.float32)), _col(db64), Cn)
    head, g = LC.tt(head_np).cuda(), LC.tt(g_np).cuda()
    lib, bad, f32run = L.load(), [], {}
    for used, with_bias in ((Cn, True), (Cn, False), (6 * K, False)):
        cpad = (used + 63) // 64 * 64
        for dtype, code in ((torch.float32, L.PPN_F32), (torch.bfloat16, L.PPN_BF16)):
            dz = torch.full((B, H, W, cpad), SENTINEL, dtype=dtype, device="cuda")
            db = torch.full((Cn,), SENTINEL, dtype=torch.float32, device="cuda")
            L.check(lib.ppn_head_grad(code, head.data_ptr(), g.data_ptr(), B, Cn, H * W, used, cpad, dz.data_ptr(),
                                      db.data_ptr() if with_bias else None, L.current_stream_ptr()), "ppn_head_grad")
            torch.cuda.synchronize()
            assert bool((_bits(dz[..., used:]) == 0).all())
            tag = f"{name} head_grad used={used} bias={int(with_bias)}"
            if dtype == torch.float32:
                f32run[(used, with_bias)] = dz
                bad += LC.check_groups(tag + " dz", _nchw(dz, used), ref[:, :used], e32)
            else:
                assert _same_bits(dz, f32run[(used, with_bias)].to(torch.bfloat16)), tag
            if with_bias:
                bad += LC.check_groups(tag + " dbias", _col(db.double().cpu().numpy()), _col(db64), e32_db)
            else:
                assert bool((db == SENTINEL).all())
    # dbias needs all channels
    rc = lib.ppn_head_grad(L.PPN_F32, head.data_ptr(), g.data_ptr(), B, Cn, H * W, 6 * K, 128, f32run[(6 * K, False)].data_ptr(),
                           g.data_ptr(), L.current_stream_ptr())
    assert rc != 0
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", LC.CASES)
def test_dual(name):
    """PPNLoss.dual, full and unary_only, against torch double backward in f64 (loss_cases.second_order)."""
    crit = _crit(name)
    head, tg = _dev(name)
    tz = LC.tt(LC.tangent(name)).cuda()
    ties = LC.parse(name)[1] in ("fit", "edge_ties", "zero_area")
    bad = []
    for ckey, unary_only in (("mix", False), ("unary", True)) + ((("e1", True), ("e1", False)) if ties else ()):
        r = LC.second_order(name, ckey)
        sl = slice(0, 6 * K) if unary_only else slice(None)
        zbar, tzbar = crit.dual(head, tz[:, sl].contiguous(), tg, LC.COEFFS[ckey], unary_only=unary_only)
        torch.cuda.synchronize()
        tag = f"{name} {ckey} dual{'(unary_only)' if unary_only else ''}"
        bad += LC.check_groups(tag + " zbar", zbar.cpu().numpy(), r["zbar64"][:, sl], r["e32_zbar"])
        bad += LC.check_groups(tag + " tzbar", tzbar.cpu().numpy(), r["tzbar64"][:, sl], r["e32_tzbar"])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("geom", list(LC.GEOMS))
def test_encode_targets(geom):
    """targets.encode_targets: the ten tensors bit-equal to the oracle, limb_c bit-equal to its definition; the batch holds
    an image without people, a person duplicated with another size, and the bounding-box-only people of edge_ties."""
    from oracle import targets_ref as T
    from pytorch_pose_proposal_network_amd import targets
    insize, outsize, local_grid = LC.GEOMS[geom]
    lists = LC.people_lists(geom, "plain", 3) + [LC.tie_people(insize, outsize)]
    twin = dict(lists[0][0])
    twin["size"] = np.float32(19.5)
    lists[0] = list(lists[0]) + [twin]
    lists[1] = []
    ref = [T.encode_targets(p, insize, outsize, local_grid) for p in lists]
    got = targets.encode_targets(targets.pack_people(lists), insize, outsize, local_grid)
    for k in targets.TARGET_KEYS:
        exp = LC.tt(np.stack([r[k] for r in ref])).cuda()
        assert _same_bits(got[k], exp), k
    assert float(got["te"].sum()) > 0 and float(got["delta"].sum()) > 0 and float(got["delta"][1].sum()) == 0
    assert got["limb_c"].dtype == torch.uint8 and torch.equal(got["limb_c"], _limb_c(got))
    (W, H), (sW, sH) = outsize, local_grid
    assert got["te"].shape == (4, LC.E, sH, sW, H, W) and got["delta"].shape == (4, K, H, W)


def _shift(t, elems=1):
    """The same values `elems` elements into a larger buffer: aligned to the element, not to 16 bytes."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    out = buf[elems:elems + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == elems * t.element_size()
    return out


@pytest.mark.parametrize("geom", ["g60", "stock"])
def test_scalar_instantiations_equal_vector(geom):
    """limb_kernel<1>, limb_loss_dz_kernel<T, 1> and limb_dual_nhwc_kernel<T, 1> (selected by a head / tangent that is not
    16-byte aligned, or a compact target that is not 4-byte aligned) give the bits of the <., 4> forms; only loss_limb is
    summed in another order."""
    from pytorch_pose_proposal_network_amd import loss, targets, prng, synth
    if geom == "stock":
        insize, outsize, local_grid, B = (384, 384), (24, 24), (21, 21), 1
    else:
        (insize, outsize, local_grid), B = LC.GEOMS[geom], 2
    lists = [synth.synthetic_people(31 + i, insize=insize) for i in range(B)]
    tg = targets.encode_targets(targets.pack_people(lists), insize, outsize, local_grid)
    plain = {k: v for k, v in tg.items() if k != "limb_c"}
    crit = loss.PPNLoss(insize=insize, outsize=outsize, local_grid_size=local_grid)
    Cn, (W, H) = LC.channels(local_grid), outsize
    assert (H * W) % 4 == 0
    n = B * Cn * H * W
    head = LC.tt(prng.uniform(prng.stream_seed(77, 1), n, 0.02, 0.98).reshape(B, Cn, H, W)).cuda()
    tz = LC.tt(prng.uniform(prng.stream_seed(77, 2), n, -1.0, 1.0).reshape(B, Cn, H, W)).cuda()
    head1, tz1 = _shift(head), _shift(tz)
    coeff = LC.COEFFS["mix"]
    cw = torch.tensor([c * 4.0 for c in coeff], dtype=torch.float32).cuda()

    def limb_close(a, b):
        return _same_bits(a[:4], b[:4]) and abs(float(a[4]) - float(b[4])) <= 1e-6 * abs(float(b[4]))

    l0, g0 = crit.forward_backward(head, plain, coeff)
    l1, g1 = crit.forward_backward(head1, plain, coeff)
    assert _same_bits(g0, g1) and limb_close(l1, l0), (l0, l1)
    for dtype in (torch.float32, torch.bfloat16):
        for t0 in (plain, tg):                                                # f32 limb targets, compact limb targets
            l0, dz0, db0 = crit.forward_backward_dz(head, t0, (cw, 4.0), dtype)
            l1, dz1, db1 = crit.forward_backward_dz(head1, t0, (cw, 4.0), dtype)
            assert _same_bits(dz0, dz1) and _same_bits(db0, db1) and limb_close(l1, l0), (dtype, l0, l1)
            a = crit.limb_dual_nhwc(head, tz, t0, -0.37, dtype)
            for h_, tz_ in ((head1, tz1), (head1, tz), (head, tz1)):
                b = crit.limb_dual_nhwc(h_, tz_, t0, -0.37, dtype)
                assert all(_same_bits(x, y) for x, y in zip(a, b)), dtype
        # aligned head, compact targets one byte off: the scalar compact path
        tg1 = dict(tg, limb_c=_shift(tg["limb_c"]))
        l0, dz0, db0 = crit.forward_backward_dz(head, tg, (cw, 4.0), dtype)
        l1, dz1, db1 = crit.forward_backward_dz(head, tg1, (cw, 4.0), dtype)
        assert _same_bits(dz0, dz1) and _same_bits(db0, db1) and limb_close(l1, l0), (dtype, l0, l1)
        a, b = crit.limb_dual_nhwc(head, tz, tg, -0.37, dtype), crit.limb_dual_nhwc(head, tz, tg1, -0.37, dtype)
        assert all(_same_bits(x, y) for x, y in zip(a, b)), dtype
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_gradnorm_probe_stats(n):
    """ppn_gradnorm_probe_stats: gw4 bit-equal to the f32 expression in the kernel's order, the seven sums within 1e-6 of
    f64 and bit-equal to train.sumsq of the matching tensor (what the kernel's comment promises)."""
    from pytorch_pose_proposal_network_amd import train as TR, prng, lib as L
    g = [prng.normalish(prng.stream_seed(900 + n % 997, k), n) for k in range(5)]
    g4, total = [LC.tt(v).cuda() for v in g[:4]], LC.tt(g[4]).cuda()
    for ckey in ("mix", "e4", "zn"):
        c = np.array(LC.COEFFS[ckey], np.float32)
        s = np.zeros(n, np.float32)
        for k in range(4):
            s = s + c[k] * g[k]                                               # f32: ((((0 + c0 g0) + c1 g1) + c2 g2) + c3 g3)
        rest = g[4] - s
        want = rest / c[4]
        assert s.dtype == rest.dtype == want.dtype == np.float32
        gw4, st = TR.probe_stats(g4, total, LC.COEFFS[ckey])
        torch.cuda.synchronize()
        assert _same_bits(gw4, LC.tt(want).cuda()), ckey
        tensors = g[:4] + [want, rest, g[4]]
        for i, v in enumerate(tensors):
            ref = float((v.astype(np.float64) ** 2).sum())
            assert abs(float(st[i]) - ref) <= 1e-6 * ref, (ckey, i, float(st[i]), ref)
            assert _same_bits(st[i:i + 1], TR.sumsq(LC.tt(v).cuda())), (ckey, i)
    with pytest.raises(L.PPNError):                                           # the remainder cannot be divided by c4 = 0
        TR.probe_stats(g4, total, LC.COEFFS["e0"])
