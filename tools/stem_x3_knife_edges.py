"""Where the float16 + exact-prefix people count moves when the stem changes by ~1e-7: the split-f16 fused stem
(fuse_stem="all", csrc/stem012_x3.hip) against the three exact-f32 stem launches, on the calibrated D-22 stem and the frames of
tests/golden/e2e_d22_384 (and e2e_tuned_d22_384).

(1) stem accuracy on the REAL stem (folded BN of the calibrated checkpoint, the e2e frames): x3 stem and f32 launches vs an
    fp64 evaluation of the three layers, relative to the output scale;
(2) the people the float16 + exact_prefix=3 net reproduces with the f32 stem when the stem's conv weights are perturbed by
    relative noise of the size of (1) (w * (1 + eps * N(0,1)), eps = 2^-22, a few seeds): the spread of that count is the
    knife-edge noise of the f16 trunk behind the prefix, and the same seeds with the x3 stem;
(3) the same counts on e2e_tuned_d22_384."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from pytorch_pose_proposal_network_amd import decode, drn, lib as L, model, prng, rt, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -22
SEEDS = range(6)


def calib_sd(arch, seed):
    st = np.load(os.path.join(ROOT, "pytorch_pose_proposal_network_amd", "data", f"bn_calib_{arch}_seed0.npz"))
    return synth.make_state_dict(arch, seed, bn_stats={k: st[k] for k in st.files})


def fixture(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    sd = calib_sd(str(g["arch"]), int(g["seed_w"]))
    for k in g.files:
        if k.startswith("override/"):
            sd[k[len("override/"):]] = g[k]
    frames = torch.from_numpy(prng.u8_frames(int(g["seed_in"]), int(g["batch"]), (384, 384))).cuda()
    return g, sd, frames


def perturbed(sd, seed):
    out = dict(sd)
    gen = torch.Generator().manual_seed(1000 + seed)
    for k, v in sd.items():
        if k.startswith(("backbone.0.", "backbone.1.", "backbone.2.")) and k.endswith(".weight") and np.ndim(v) == 4:
            t = torch.as_tensor(np.asarray(v), dtype=torch.float32)
            out[k] = (t.double() * (1.0 + EPS * torch.randn(t.shape, generator=gen, dtype=torch.float64))).float().numpy()
    return out


def people(g, sd, frames, **kw):
    net = model.PoseProposalNet(drn.drn_d_22(), compute_dtype="float16", **kw).cuda()
    net.load_state_dict(sd)
    got = rt.inference_batch(frames, net).to_host()
    tot = np.zeros(5, np.int64)
    for i in range(int(g["batch"])):
        tot += np.array(decode.people_agreement({k: g[f"{i}/{k}"] for k in ("n", "kp_cell", "limb_arg")}, got[i]))
    del net
    return tot


def stem_accuracy(sd, frames, nimg=8):
    """x3 stem and f32 launches vs fp64 on the calibrated stem, relative to max(1, max|ref|)."""
    lib = L.load()
    net = model.PoseProposalNet(drn.drn_d_22(), compute_dtype="float16", exact_prefix=3, fuse_stem="all").cuda()
    net.load_state_dict(sd)
    op = net._ops[0]
    p = lambda k: net._dev[op.name + k]
    w0, s0, b0, w1, s1, b1, w2, s2, b2, s3, b3 = (p(k) for k in (".w", ".s1", ".b1", ".w1", ".s1b", ".b1b", ".w2", ".s1c",
                                                                 ".b1c", ".s2", ".b2"))
    x = frames[:nimg].contiguous()
    B, H, W = x.shape[0], 384, 384
    st = torch.cuda.current_stream().cuda_stream
    m3, s3c = (C.c_float * 3)(*net._mean), (C.c_float * 3)(*net._std)
    raw, act = torch.empty(B, 192, 192, 32, device="cuda"), torch.empty(B, 192, 192, 32, device="cuda")
    L.check(lib.ppn_stem012_dt(L.PPN_STEM_X3_F32, 1, x.data_ptr(), B, H, W, w0.data_ptr(), s0.data_ptr(), b0.data_ptr(), m3,
                               s3c, w1.data_ptr(), s1.data_ptr(), b1.data_ptr(), w2.data_ptr(), s2.data_ptr(), b2.data_ptr(),
                               s3.data_ptr(), b3.data_ptr(), raw.data_ptr(), act.data_ptr(), st), "ppn_stem012_dt")
    # the three f32 launches
    t0, t1 = torch.empty(B, H, W, 16, device="cuda"), torch.empty(B, H, W, 16, device="cuda")
    fr, fa = torch.empty_like(raw), torch.empty_like(act)
    L.check(lib.ppn_stem7x7(L.PPN_F32, 1, x.data_ptr(), B, H, W, w0.data_ptr(), s0.data_ptr(), b0.data_ptr(), m3, s3c,
                            t0.data_ptr(), st), "ppn_stem7x7")
    zero = torch.zeros(64, device="cuda")
    for src, wd, cout, stride, sc, sh, o_raw, o_act in ((t0, w1, 16, 1, s1, b1, t1, None), (t1, w2, 32, 2, s2, b2, fr, fa)):
        _, _, _, ktot, cpad = L.conv_tiling(L.PPN_F32, 16, cout, 3)
        d = L.ConvDesc()
        d.dtype, d.batch, d.in_h, d.in_w, d.cin = L.PPN_F32, B, H, W, 16
        d.out_h, d.out_w, d.cout = o_raw.shape[1], o_raw.shape[2], cout
        d.ksize, d.stride, d.dilation, d.pad = 3, stride, 1, 1
        d.k_total, d.cout_pad, d.act1, d.act2 = ktot, cpad, 1, (1 if o_act is not None else 0)
        d.src, d.weight, d.zero_page = src.data_ptr(), wd.data_ptr(), zero.data_ptr()
        d.scale1, d.shift1, d.out_raw = sc.data_ptr(), sh.data_ptr(), o_raw.data_ptr()
        if o_act is not None:
            d.scale2, d.shift2, d.out_act = s3.data_ptr(), b3.data_ptr(), o_act.data_ptr()
        L.check(lib.ppn_conv2d_fused(C.byref(d), st), "ppn_conv2d_fused")
    torch.cuda.synchronize()
    # fp64 (on the device)
    mean = torch.tensor(list(net._mean), dtype=torch.float64, device="cuda").view(1, 3, 1, 1)
    std = torch.tensor(list(net._std), dtype=torch.float64, device="cuda").view(1, 3, 1, 1)
    xn = (x.permute(0, 3, 1, 2).double() - mean) / std
    v = lambda t: t.double().view(1, -1, 1, 1)
    y = F.relu(F.conv2d(xn, w0.double(), None, 1, 3) * v(s0) + v(b0))
    y = F.relu(F.conv2d(y, w1.double(), None, 1, 1) * v(s1) + v(b1))
    y = F.relu(F.conv2d(y, w2.double(), None, 2, 1) * v(s2) + v(b2))
    u = F.relu(y * v(s3) + v(b3))
    ref = {"raw": y.permute(0, 2, 3, 1), "act": u.permute(0, 2, 3, 1)}
    for tag, a_, f_ in (("raw", raw, fr), ("act", act, fa)):
        r = ref[tag]
        scale = max(1.0, float(r.abs().max()))
        ex, ef, exf = ((a_.double() - r).abs(), (f_.double() - r).abs(), (a_ - f_).double().abs())
        print(f"calibrated stem, {nimg} e2e frames, {tag}: scale {scale:.3g}; max / mean |.| / scale: x3 vs fp64 "
              f"{float(ex.max()) / scale:.2e} / {float(ex.mean()) / scale:.2e}, f32 launches vs fp64 {float(ef.max()) / scale:.2e} / "
              f"{float(ef.mean()) / scale:.2e}, x3 vs f32 {float(exf.max()) / scale:.2e} / {float(exf.mean()) / scale:.2e}", flush=True)
    del net


def main():
    g, sd, frames = fixture("e2e_d22_384")
    stem_accuracy(sd, frames)
    for name in ("e2e_d22_384", "e2e_tuned_d22_384"):
        g, sd, frames = fixture(name)
        for tag, kw in (("f32 stem", {}), ("x3 stem", dict(fuse_stem="all"))):
            t = people(g, sd, frames, exact_prefix=3, **kw)
            print(f"{name} exact_prefix=3 {tag}: {t[1]}/{t[0]} exact, same root {t[2]}", flush=True)
        if name != "e2e_d22_384":
            continue
        for tag, kw in (("f32 stem", {}), ("x3 stem", dict(fuse_stem="all"))):
            counts = []
            for s in SEEDS:
                t = people(g, perturbed(sd, s), frames, exact_prefix=3, **kw)
                counts.append(int(t[1]))
                print(f"{name} exact_prefix=3 {tag}, stem weights x (1 + 2^-22 N(0,1)) seed {s}: {t[1]}/{t[0]} exact, "
                      f"same root {t[2]}", flush=True)
            print(f"{name} exact_prefix=3 {tag}, perturbed stems: exact people {counts} (min {min(counts)}, max {max(counts)})",
                  flush=True)


if __name__ == "__main__":
    main()
