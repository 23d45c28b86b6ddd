"""The split-f16 fused stem (csrc/stem012_x3.hip, PPN_STEM_IO(PPN_F16X3, PPN_F32)) against what it replaces and what it
resembles, batch 32, 384x384 u8 frames: (1) the three exact-f32 launches of the float16x3 / exact-prefix modes (ppn_stem7x7 +
two 3x3 launches), (2) the fused x3 stem, (3) the 16-bit fused stem as the bf16 plan runs it (PPN_STEM_IO(PPN_F16,
PPN_BF16)).  Then the one-lane float16x3 step (forward_u8 + fused decode) with and without fuse_stem="all"."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pytorch_pose_proposal_network_amd import decode, drn, lib as L, model, prng, synth

B, H, W = 32, 384, 384
Ho, Wo = 192, 192


def timed(fn, reps=10, rounds=3):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(e) * 1e3 / reps)
    return out


def kernels():
    lib = L.load()
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    frames = torch.from_numpy(prng.u8_frames(1, B, (H, W))).to(dev)
    g = torch.Generator().manual_seed(0)
    w0 = (torch.randn(16, 3, 7, 7, generator=g) * 0.002).to(dev)
    w1 = (torch.randn(16, 16, 3, 3, generator=g) * 0.1).to(dev)
    w2 = (torch.randn(32, 16, 3, 3, generator=g) * 0.1).to(dev)
    s = [torch.rand(n, generator=g).to(dev) + 0.5 for n in (16, 16, 32, 32)]
    b = [torch.randn(n, generator=g).to(dev) * 0.3 for n in (16, 16, 32, 32)]
    m3, s3 = (C.c_float * 3)(0.485, 0.456, 0.406), (C.c_float * 3)(0.229, 0.224, 0.225)
    raw32, act32 = torch.empty(B, Ho, Wo, 32, device=dev), torch.empty(B, Ho, Wo, 32, device=dev)
    raw16, act16 = torch.empty(B, Ho, Wo, 32, dtype=torch.bfloat16, device=dev), torch.empty(B, Ho, Wo, 32, dtype=torch.bfloat16, device=dev)
    t0, t1 = torch.empty(B, H, W, 16, device=dev), torch.empty(B, H, W, 16, device=dev)
    zero = torch.zeros(64, device=dev)

    def fused(dt, raw, act):
        def run():
            L.check(lib.ppn_stem012_dt(dt, 1, frames.data_ptr(), B, H, W, w0.data_ptr(), s[0].data_ptr(), b[0].data_ptr(), m3,
                                       s3, w1.data_ptr(), s[1].data_ptr(), b[1].data_ptr(), w2.data_ptr(), s[2].data_ptr(),
                                       b[2].data_ptr(), s[3].data_ptr(), b[3].data_ptr(), raw.data_ptr(), act.data_ptr(), st),
                    "ppn_stem012_dt")
        return run

    descs = []
    for x, wd, cout, stride, i, out_raw, out_act in ((t0, w1, 16, 1, 1, t1, None), (t1, w2, 32, 2, 2, raw32, act32)):
        _, _, _, ktot, cpad = L.conv_tiling(L.PPN_F32, 16, cout, 3)
        d = L.ConvDesc()
        d.dtype, d.batch, d.in_h, d.in_w, d.cin = L.PPN_F32, B, H, W, 16
        d.out_h, d.out_w, d.cout = out_raw.shape[1], out_raw.shape[2], cout
        d.ksize, d.stride, d.dilation, d.pad = 3, stride, 1, 1
        d.k_total, d.cout_pad, d.act1, d.act2 = ktot, cpad, 1, (1 if out_act is not None else 0)
        d.src, d.weight, d.zero_page = x.data_ptr(), wd.data_ptr(), zero.data_ptr()
        d.scale1, d.shift1, d.out_raw = s[i].data_ptr(), b[i].data_ptr(), out_raw.data_ptr()
        if out_act is not None:
            d.scale2, d.shift2, d.out_act = s[3].data_ptr(), b[3].data_ptr(), out_act.data_ptr()
        descs.append(d)

    def f32_layer0():
        L.check(lib.ppn_stem7x7(L.PPN_F32, 1, frames.data_ptr(), B, H, W, w0.data_ptr(), s[0].data_ptr(), b[0].data_ptr(),
                                m3, s3, t0.data_ptr(), st), "ppn_stem7x7")

    def f32_conv(d):
        return lambda: L.check(lib.ppn_conv2d_fused(C.byref(d), st), "ppn_conv2d_fused")

    parts = [("f32 layer0 (stem7x7)", f32_layer0), ("f32 layer1 (3x3)", f32_conv(descs[0])),
             ("f32 layer2 (3x3 s2)", f32_conv(descs[1]))]
    tot = np.zeros(3)
    for name, fn in parts:
        t = timed(fn)
        tot += np.array(t)
        print(f"{name:34s} " + "  ".join(f"{v:7.1f}" for v in t) + " us", flush=True)
    print(f"{'three f32 launches (sum)':34s} " + "  ".join(f"{v:7.1f}" for v in tot) + " us", flush=True)
    for name, dt, r, a in (("fused x3 stem (stem012_x3)", L.PPN_STEM_X3_F32, raw32, act32),
                           ("16-bit fused stem (stem012)", L.PPN_STEM_IO(L.PPN_F16, L.PPN_BF16), raw16, act16)):
        t = timed(fused(dt, r, a))
        print(f"{name:34s} " + "  ".join(f"{v:7.1f}" for v in t) + " us", flush=True)


def steps():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    stt = np.load(os.path.join(root, "pytorch_pose_proposal_network_amd", "data", "bn_calib_drn_d_22_seed0.npz"))
    sd = synth.make_state_dict("drn_d_22", 0, bn_stats={k: stt[k] for k in stt.files})
    frames = torch.from_numpy(prng.u8_frames(1234, B, (H, W))).cuda()
    for fuse in (None, "all"):
        net = model.PoseProposalNet(drn.drn_d_22(), compute_dtype="float16x3", fuse_stem=fuse).cuda()
        net.load_state_dict(sd)
        d = decode.Decoder(B)

        def step():
            u, k = net.forward_u8(frames, fused_decode=True)
            d.decode_fused(u, k)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 20
        print(f"float16x3 fuse_stem={fuse}: {B / dt:.0f} images/s one lane ({dt * 1e3:.3f} ms)", flush=True)
        for name, kern, ms, fl in net.profile_layers(frames, src_is_u8=True, fused_decode=True)[:6]:
            print(f"   {name:34s} {ms * 1e3:8.1f} us  {kern}")
        del net


if __name__ == "__main__":
    kernels()
    if "--kernels-only" not in sys.argv:
        steps()
