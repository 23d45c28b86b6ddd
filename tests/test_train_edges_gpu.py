"""The streaming training kernels of csrc/train.hip on the cases of tests/train_cases.py: train-mode BatchNorm forward and
backward, its tangent and dual backward (widths 8 - 2048, one and two pixels, a ragged second work-group, the 1024-block cap,
channels offset by 100 and 1000 sigma, constant / zero / tiny-variance channels, gamma <= 0, the kink z == 0), the pointwise
tails, FlatAdam off its defaults, sumsq, colsum, nchw_to_nhwc and GradNorm's two kernels on their own.

Every BatchNorm output is held to a bound computed from the f64 reference's intermediates by counting f32 roundings
(train_cases.py); the tests print the worst err / bound of every output (lines starting TRAIN_EDGE;
profiles/train_edge_errors.txt holds one run's) and assert that none exceeds 1."""
import numpy as np
import pytest
import torch

import train_cases as TC

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _dev(o):
    return {k: v.cuda() for k, v in o.items()}


def _report(tag, ratios, extra=""):
    print(f"TRAIN_EDGE {tag}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + extra)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (tag, bad)


def _bn_gpu(o, act, eps, mom):
    """Every single-stream BatchNorm entry point once; returns (name -> CPU tensor, device extras)."""
    from pytorch_pose_proposal_network_amd import train as T
    d = _dev(o)
    x, ga, be = d["x"], d["gamma"], d["beta"]
    rm, rv = d["rm"].clone(), d["rv"].clone()
    y, saved = T.bn_train_forward(x, ga, be, rm, rv, act=act, eps=eps, momentum=mom)
    dx_add, dg, db = T.bn_train_backward(x, d["dy"], ga, be, saved, act=act, dx_add=d["add"])
    dx, dg2, db2 = T.bn_train_backward(x, d["dy"], ga, be, saved, act=act)
    tan = T.bn_tangent(x, d["xdot"], ga, be, saved, act)
    ddx, ddxdot, ddg, ddb = T.bn_dual_backward(x, d["xdot"], d["dy"], d["dyt"], ga, be, saved, act)
    # a second launch of everything: bitwise equal (fixed fold order, no atomics)
    y_b, saved_b = T.bn_train_forward(x, ga, be, act=act, eps=eps, momentum=mom)
    dx_b, dg_b, db_b = T.bn_train_backward(x, d["dy"], ga, be, saved_b, act=act, dx_add=d["add"])
    e_dx, e_dxdot, e_dg, e_db = T.bn_dual_backward(x, d["xdot"], d["dy"], d["dyt"], ga, be, saved_b, act)
    torch.cuda.synchronize()
    assert _same(y, y_b) and _same(saved.mean, saved_b.mean) and _same(saved.rstd, saved_b.rstd)
    assert _same(dx_add, dx_b) and _same(dg, dg_b) and _same(db, db_b)
    assert _same(ddx, e_dx) and _same(ddxdot, e_dxdot) and _same(ddg, e_dg) and _same(ddb, e_db)
    assert _same(dg, dg2) and _same(db, db2) and _same(db, ddb)              # dx_add touches neither parameter gradient
    for k in ("x", "dy", "add", "xdot", "dyt"):
        assert _same(d[k].cpu(), o[k])                                       # no operand is written
    got = dict(mean=saved.mean, rstd=saved.rstd, y=y, rm=rm, rv=rv, dbeta=db, dgamma=dg, dx=dx, dx_add=dx_add, tan=tan,
               dual_dx=ddx, dual_dxdot=ddxdot, dual_dgamma=ddg, dual_dbeta=ddb)
    return {k: v.cpu() for k, v in got.items()}, (d, saved)


def _bn_reference(o, act, eps, mom, lo, cap, branch=None):
    r = TC.bn_ref(o["x"], o["gamma"], o["beta"], o["rm"], o["rv"], eps, mom, act, o["dy"], o["add"], branch=branch)
    d = TC.bn_dual_ref(r, o["xdot"], o["dyt"])
    amb = TC.ambiguous(r) if cap else None
    return r, d, amb, TC.bn_references(r, d), TC.bn_bounds(r, d, lo, amb)


@pytest.mark.parametrize("name,act,dtype", TC.bn_runs())
def test_bn_edges(name, act, dtype):
    """bn_train_forward, bn_train_backward with and without dx_add, bn_tangent and bn_dual_backward on one case."""
    o = TC.bn_operands(name, dtype)
    eps, mom = TC.case_eps_momentum(name)
    cap = name in TC.CAP_CASES
    got, _ = _bn_gpu(o, act, eps, mom)
    r, d, amb, refs, bounds = _bn_reference(o, act, eps, mom, dtype == "bf16", cap)
    ratios = TC.bn_ratios(got, refs, bounds, amb)
    extra = ""
    if cap:
        share = int(amb.sum()) / amb.numel() if amb is not None else 0.0
        extra = f", ambiguous {int(amb.sum()) if amb is not None else 0} of {r.x.numel()} ({share:.1e})"
        assert share <= TC.AMBIGUOUS_SHARE_MAX
    if name in TC.BN_VALUES:
        # exact, from the kernels' own arithmetic
        assert _same(got["dx_add"][:, 10], o["add"][:, 10])                  # gamma = 0, beta = -1: every coefficient is 0
        b = o["beta"][6]
        want = {"none": b, "relu": b.clamp(min=0), "lrelu": b if b > 0 else b * torch.tensor(0.1)}[act]
        assert _same(got["y"][:, 6], want.to(got["y"].dtype).expand(TC.VALUE_P).contiguous())       # x = 0: z = beta
        if act == "relu":                                                    # z == 0: the kink has the slope of the left side
            assert float(got["dbeta"][9]) == 0.0 and float(got["dgamma"][9]) == 0.0
    _report(f"bn {name} {act} {dtype}", ratios, extra)


@pytest.mark.parametrize("name,dtype", [(n, d) for n in TC.STREAM_CASES for d in TC.BN_SHAPES[n]["dtypes"]])
def test_bn_stream_forms(name, dtype):
    """Two streams over one x -- (xdot, dy, dyt) and (2 xdot, dy, dyt / 2) -- through the multi-stream entry points: every
    stream bitwise equal to the single-stream call on its slices; bn_dual_backward_summed (whose dual terms then are equal:
    the term is bilinear in (xdot, dyt)) against the f64 reference dx(dy) + 2 dual."""
    from pytorch_pose_proposal_network_amd import train as T
    act = "relu" if name in TC.CAP_CASES else "lrelu"
    o = TC.bn_operands(name, dtype)
    d = _dev(o)
    x, ga, be = d["x"], d["gamma"], d["beta"]
    P = x.shape[0]
    _, saved = T.bn_train_forward(x, ga, be, act=act)
    xdot2, dy2, dyt2 = torch.cat([d["xdot"], d["xdot"] * 2]), torch.cat([d["dy"], d["dy"]]), torch.cat([d["dyt"], d["dyt"] * 0.5])
    add2 = torch.cat([d["add"], d["xdot"]])
    sl = [slice(0, P), slice(P, 2 * P)]
    dx_m, dg_m, db_m = T.bn_train_backward(x, dyt2, ga, be, saved, act=act, dx_add=add2, nstreams=2)
    t_m = T.bn_tangent(x, xdot2, ga, be, saved, act, nstreams=2)
    a_m = T.bn_dual_backward(x, xdot2, dy2, dyt2, ga, be, saved, act, nstreams=2)
    b_m = T.bn_dual_backward(x, xdot2, None, None, ga, be, saved, act, nstreams=2, dy_dyt=torch.cat([dy2, dyt2]))
    singles = []
    for j in range(2):
        dx, dg, db = T.bn_train_backward(x, dyt2[sl[j]], ga, be, saved, act=act, dx_add=add2[sl[j]])
        assert _same(dx, dx_m[sl[j]]) and _same(dg, dg_m[j]) and _same(db, db_m[j]), j
        assert _same(T.bn_tangent(x, xdot2[sl[j]], ga, be, saved, act), t_m[sl[j]]), j
        ref = T.bn_dual_backward(x, xdot2[sl[j]], dy2[sl[j]], dyt2[sl[j]], ga, be, saved, act)
        for m in (a_m, b_m):
            assert _same(ref[0], m[0][sl[j]]) and _same(ref[1], m[1][sl[j]]), j
            assert _same(ref[2], m[2][j]) and _same(ref[3], m[3][j]), j
        singles.append(ref)
    sdx, sdxdot, sdg, sdb = T.bn_dual_backward_summed(x, xdot2, torch.cat([d["dy"], dyt2]), ga, be, saved, act, 2)
    torch.cuda.synchronize()
    assert _same(sdxdot, a_m[1]) and _same(sdb, singles[0][3])
    lo = dtype == "bf16"
    r = TC.bn_ref(o["x"], o["gamma"], o["beta"], act=act, dy=o["dy"])
    dd = TC.bn_dual_ref(r, o["xdot"], o["dyt"])
    amb = TC.ambiguous(r) if name in TC.CAP_CASES else None
    b = TC.dual_bounds(r, dd, lo, amb, streams=2)
    ratios = dict(summed_dx=TC.worst_ratio(sdx.cpu(), r.dx + 2 * dd.dual, b["dx"], amb),
                  summed_dgamma=TC.worst_ratio(sdg.cpu(), r.dgamma + 2 * dd.dg_tan, b["dgamma"]))
    _report(f"bn streams {name} {act} {dtype}", ratios)


def _act_mask_of_ones(T, x, ga, be, saved, act):
    import ctypes as C
    from pytorch_pose_proposal_network_amd import lib as L
    out = torch.empty_like(x)
    d = T._bwd_desc(x, torch.ones_like(x), ga, be, saved, act, out)
    L.check(L.load().ppn_bn_act_mask(C.byref(d), L.current_stream_ptr()), "ppn_bn_act_mask")
    return out


@pytest.mark.parametrize("act", ["relu", "lrelu"])
def test_backward_kernels_take_the_forward_branch(act):
    """Half of the elements lie within 16 single-ulp steps of the x at which z = 0 (train_cases.kink_operands).  The side the
    forward kernel took is read off its stored y; ppn_bn_act_mask of an all-ones tensor must give exactly that slope at EVERY
    element, and the backward, tangent and dual kernels -- which recompute z = x*sc + sh, each in its own code -- must stay
    inside their bounds around the reference evaluated on the forward's side: one element on the other side is off by its whole
    gradient, thousands of bounds."""
    from pytorch_pose_proposal_network_amd import train as T
    o = TC.kink_operands(act)
    o["rm"], o["rv"] = torch.zeros(16), torch.ones(16)
    got, (d, saved) = _bn_gpu(o, act, 1e-5, 0.1)
    pos = got["y"] > 0
    slope = _act_mask_of_ones(T, d["x"], d["gamma"], d["beta"], saved, act).cpu()
    torch.cuda.synchronize()
    want = torch.where(pos, torch.tensor(1.0), torch.tensor(0.0 if act == "relu" else 0.1))
    assert _same(slope, want), int((slope != want).sum())
    r, dd, _, refs, bounds = _bn_reference(o, act, 1e-5, 0.1, False, False, branch=pos)
    flipped = int((pos != (r.z > 0)).sum())
    near = int((r.z.abs() <= 20 * 2.0 ** -24 * r.sc.abs()).sum())
    _report(f"bn kink {act} f32", TC.bn_ratios(got, refs, bounds),
            f", {near} elements within 20 steps of z = 0, forward on the other side than the f64 z at {flipped}")


# ---- pointwise tails ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n", [8, 2040, 2056, 8388632])
def test_add_relu_and_relu_mask_bitwise(n, dtype):
    """n = 8 * 1048579 takes a second trip through the grid-stride loop (4096 work-groups x 256 threads x 8 elements)."""
    from pytorch_pose_proposal_network_amd import train as T
    t = TC.DTYPES[dtype]
    g = torch.Generator().manual_seed(n)
    z, r = torch.randn(n, generator=g).to(t), torch.randn(n, generator=g).to(t)
    r[1::5] = -z[1::5]                                                       # exact cancellations
    vz, vr = TC.pointwise_values(dtype)
    k = min(n, vz.numel())
    z[:k], r[:k] = vz[:k], vr[:k]
    z[n - k:], r[n - k:] = vz[:k], vr[:k]                                    # ... and in the last (second-trip) items
    dout, add = torch.randn(n, generator=g).to(t), torch.randn(n, generator=g).to(t)
    add[::7] = -0.0
    zd, rd, dd, ad = z.cuda(), r.cuda(), dout.cuda(), add.cuda()
    out = T.add_relu(zd, rd)
    dz, dza = T.relu_mask(out, dd), T.relu_mask(out, dd, ad)
    torch.cuda.synchronize()
    want = TC.add_relu_ref(z, r)
    assert _same(out.cpu(), want)
    assert _same(dz.cpu(), TC.relu_mask_ref(want, dout))
    assert _same(dza.cpu(), TC.relu_mask_ref(want, dout, add))
    assert _same(zd.cpu(), z) and _same(rd.cpu(), r) and _same(dd.cpu(), dout) and _same(ad.cpu(), add)


def test_pointwise_refusals_and_empty():
    from pytorch_pose_proposal_network_amd import train as T, lib as L
    dev = torch.device("cuda")
    for n in (4, 12, 2047):
        z = torch.zeros(n, device=dev)
        with pytest.raises(L.PPNError):
            T.add_relu(z, z)
        with pytest.raises(L.PPNError):
            T.relu_mask(z, z)
    e = torch.zeros(0, device=dev, dtype=torch.bfloat16)
    assert T.add_relu(e, e).numel() == 0 and T.relu_mask(e, e, e).numel() == 0
    torch.cuda.synchronize()


# ---- Adam -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 1048575, 1048577])
def test_flat_adam_off_defaults(n):
    """weight_decay 0.01, betas (0.8, 0.99), eps 1e-3, a step count resumed at 200 000, sizes on both sides of the grid cap
    (4096 work-groups x 256 threads = 1 048 576), against torch.optim.Adam on the CPU at the tolerances of test_train_gpu.py."""
    from pytorch_pose_proposal_network_amd import train as T
    kw = dict(lr=7e-4, betas=(0.8, 0.99), eps=1e-3, weight_decay=0.01)
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], **kw)
    dev = torch.device("cuda")
    pd = p0.to(dev)
    lp = torch.empty(n, dtype=torch.bfloat16, device=dev)
    mine = T.FlatAdam(pd, param_lp=lp, **kw)
    for it in range(4):
        if it == 1:                                                          # resume: both sides continue at step 200 001
            mine.step_count = 200000
            opt.state[ref]["step"] = torch.tensor(200000.0)
        grad = torch.randn(n, generator=g) * (10.0 ** (it - 2))
        if it == 2:
            grad.zero_()                                                     # weight decay alone drives this step
        ref.grad = grad.clone() / 2
        opt.step()
        mine.step(grad.to(dev), grad_scale=0.5)
    torch.cuda.synchronize()
    assert mine.step_count == 200003 and int(opt.state[ref]["step"]) == 200003
    assert torch.allclose(pd.cpu(), ref.detach(), rtol=2e-6, atol=2e-7)
    st = opt.state[ref]
    assert torch.allclose(mine.exp_avg.cpu(), st["exp_avg"], rtol=2e-6, atol=1e-9)
    assert torch.allclose(mine.exp_avg_sq.cpu(), st["exp_avg_sq"], rtol=2e-6, atol=1e-12)
    assert _same(lp.cpu(), pd.cpu().to(torch.bfloat16))
    p64, m64, v64 = TC.adam_ref(p0, [torch.zeros(n)], first_step=1, **kw)    # and one step against the plain f64 restatement
    one = T.FlatAdam(p0.to(dev), **kw)
    one.step(torch.zeros(n, device=dev))
    assert torch.allclose(one.param.cpu().double(), p64, rtol=2e-6, atol=2e-7)
    assert float((one.param.cpu() - p0).abs().max()) > 0                     # weight decay did move them


@pytest.mark.parametrize("n", [0, 1, 1048577])
def test_flat_adam_zero_gradient_and_empty(n):
    """Without weight decay an all-zero gradient on fresh moments leaves the parameters bitwise unchanged (0 / eps = 0);
    n == 0 is a no-op that still counts the step."""
    from pytorch_pose_proposal_network_amd import train as T
    dev = torch.device("cuda")
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(3))
    pd = p0.to(dev)
    lp = torch.full((n,), 7.0, dtype=torch.bfloat16, device=dev)
    mine = T.FlatAdam(pd, lr=7e-4, betas=(0.8, 0.99), eps=1e-3, param_lp=lp)
    for _ in range(2):
        mine.step(torch.zeros(n, device=dev))
    torch.cuda.synchronize()
    assert mine.step_count == 2
    assert _same(pd.cpu(), p0) and _same(lp.cpu(), p0.to(torch.bfloat16))
    assert float(mine.exp_avg.abs().sum()) == 0.0 and float(mine.exp_avg_sq.abs().sum()) == 0.0


# ---- reductions and relayout ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 255, 2049, 2097157])
def test_sumsq_sizes_and_magnitudes(n):
    """Magnitudes from 1e15 down to 1e-20 in one tensor (the first element is the largest, so n = 1 is not a subnormal sum);
    n = 2 097 157 is 1024 work-groups of 8 elements per thread and a ragged remainder."""
    from pytorch_pose_proposal_network_amd import train as T
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(n, generator=g).double() * 10.0 ** torch.linspace(15, -20, n, dtype=torch.float64)).float()
    got = float(T.sumsq(x.cuda()).cpu())
    ref = float((x.double() ** 2).sum())
    if n == 0:
        assert got == 0.0 and not np.signbit(got)
        return
    print(f"TRAIN_EDGE sumsq n {n}: ref {ref:.6e}, err / bound {abs(got - ref) / TC.sumsq_bound(ref):.3f}")
    assert abs(got - ref) <= TC.sumsq_bound(ref)


def _colsum_ratio(x):
    from pytorch_pose_proposal_network_amd import train as T
    out = torch.full((x.shape[-1],), 7.0, device="cuda")
    T.colsum(x.cuda(), out)
    x64 = x.double()
    return TC.worst_ratio(out.cpu(), x64.sum(0), TC.colsum_bound(x64))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_colsum_values(dtype):
    ratios = {}
    for C in (8, 64, 2048):
        for P in (1, 70, 513):
            g = torch.Generator().manual_seed(C + P)
            x = (torch.randn(P, C, generator=g) * 1.7 + 0.6).to(TC.DTYPES[dtype])
            ratios[f"{C}x{P}"] = _colsum_ratio(x)
    _report(f"colsum {dtype}", ratios)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_colsum_at_the_block_cap(dtype):
    _report(f"colsum cap16 {dtype}", {"cap16": _colsum_ratio(TC.bn_operands("cap16", dtype)["x"])})


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_nchw_to_nhwc_equals_permute(dtype):
    from pytorch_pose_proposal_network_amd import train as T, config as cfg
    t = TC.DTYPES[dtype]
    g = torch.Generator().manual_seed(9)
    runs = [(ch, hw, None) for ch in (1, 64, 65, cfg.lastsize()) for hw in ((1, 1), (8, 8), (5, 13))]
    runs += [(65, (5, 13), 64), (cfg.lastsize(), (8, 8), 108), (130, (1, 1), 1)]          # channels_used < channels
    for ch, (H, W), used in runs:
        src = torch.randn(2, ch, H, W, generator=g)
        got = T.nchw_to_nhwc(src.cuda(), t, used)
        u = ch if used is None else used
        cpad = (u + 63) // 64 * 64
        want = torch.zeros(2, H, W, cpad, dtype=t)
        want[..., :u] = src.permute(0, 2, 3, 1)[..., :u].to(t)
        assert _same(got.cpu(), want), (ch, H, W, used)


# ---- GradNorm's two kernels on their own --------------------------------------------------------------------------------------

def _gradnorm(w0, gn, alpha, world, steps=2):
    from pytorch_pose_proposal_network_amd import train as T
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(2)
    losses = torch.rand(5, generator=g) * 3 + 0.1
    base = torch.rand(5, generator=g) * 3 + 0.1
    lr, betas, eps = 0.025, (0.8, 0.99), 1e-6
    mine = T.GradNormWeights(dev, lr=lr, alpha=alpha, betas=betas, eps=eps)
    mine.w.copy_(torch.tensor(w0))
    mine.step_count = 6
    w, m, v = np.array(w0, np.float64), np.zeros(5), np.zeros(5)
    gnt = torch.tensor(gn, dtype=torch.float32)
    for it in range(steps):
        log = mine.local_step(losses.to(dev), gnt.to(dev), base.to(dev)).cpu().double().numpy()
        w_in = w
        w, m, v, G, Cc, dw, lgrad = TC.gradnorm_step_ref(w, losses.numpy(), gnt.numpy(), base.numpy(), alpha, m, v, lr, betas, eps,
                                                         7 + it)
        np.testing.assert_allclose(log[0:5], G, rtol=1e-5)
        np.testing.assert_allclose(log[5:10], Cc, rtol=1e-5)
        assert np.array_equal(log[10:15], dw), (log[10:15], dw, w_in)        # signs times gn: exact
        assert abs(log[15] - lgrad) <= 1e-5 * max(1.0, abs(lgrad))
        np.testing.assert_allclose(mine.w.cpu().numpy(), w, rtol=2e-5, atol=1e-6)
        mine.renorm(world)
        clamped = int((w / world < 0).sum())
        w = TC.gradnorm_renorm_ref(w, world)
        np.testing.assert_allclose(mine.w.cpu().numpy(), w, rtol=2e-5, atol=1e-6)
        assert mine.host_weights() == mine.w.cpu().tolist()
        w = mine.w.cpu().double().numpy()                                    # both sides go on from the f32 weights
    return clamped


def test_gradnorm_signs_zero_weight_and_world_2():
    """sign(w) at a negative and at a zero weight (alpha = 2 keeps (lhat / mean)^alpha real for a negative lhat), world = 2,
    the negative weight clamped to 0 by renorm."""
    assert _gradnorm([1.2, -0.4, 1.0, 0.0, 2.0], [0.7, 1.9, 0.4, 1.1, 0.9], 2.0, 2, steps=1) == 1


def test_gradnorm_tasks_on_target():
    """alpha = 0: C_i = mean(G) exactly; tasks 0, 3 and 4 have G_i == C_i, so d == 0 and their dw is 0, not +-gn."""
    _gradnorm([1.0, 1.0, 1.0, 1.0, 1.0], [2.0, 1.0, 3.0, 2.0, 2.0], 0.0, 1, steps=1)
