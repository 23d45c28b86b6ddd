"""Time the frame ingest launches and the PCIe-inclusive pipeline fed with raw video frames.

    python tools/bench_ingest.py [--out profiles/ingest_yuv.txt] [--windows 12] [--calls 200] [--steps 12]

One process, every shape warmed, the variants taking turns window by window (the box is shared), median and min..max over
the windows; device events around the launch windows, a host clock around pipeline windows that end in a synchronise.

1. Launch time of ppn_ingest_frames (packed BGR) and of ppn_ingest_yuv for NV12, I420 and YUYV at batch 32, for
   1920 x 1080 -> 384 x 384 and for 384 x 384 -> 384 x 384.  GATE: the NV12 median at 1080p is at most 1.10 x the BGR median of
   the same run (the same 4-tap gather over fewer bytes with wider stores; 10 % for noise: back-to-back windows of launches
   this small measure the enqueue path as much as the kernel).  A missed gate is written down and exits with status 1.
2. rt.MultiLaneInference fed from pinned host memory: submit of 384 x 384 RGB (the baseline), submit_raw of 384 x 384 NV12,
   submit_raw of 1920 x 1080 NV12 -- images/s and bytes per image over PCIe.  Reported, not gated.
Needs a GPU; there is no fallback."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GATE = 1.10


def launch_window(fn, calls):
    """us per call of `calls` back-to-back launches between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def alternated(fns, window, windows, warmup):
    """`windows` windows of every fn, the fns taking turns; each fn warmed first.  Returns one list of results per fn."""
    for fn in fns:
        window(fn, warmup)
    out = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            out[i].append(window(fn, None))
    return out


def spread(v):
    return statistics.median(v), min(v), max(v)


def random_bytes(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_yuv.txt"))
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--calls", type=int, default=200, help="launches per window (part 1)")
    ap.add_argument("--steps", type=int, default=12, help="batches per window (part 2)")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--skip-pipeline", action="store_true")
    a = ap.parse_args()
    if a.windows < 10:
        sys.exit("at least 10 windows")
    if not torch.cuda.is_available():
        sys.exit("bench_ingest.py needs a GPU")
    from pytorch_pose_proposal_network_amd import rt

    B, S = a.batch, 384
    out = torch.empty(B, S, S, 3, dtype=torch.uint8, device="cuda")
    lines = [f"ingest bench: batch {B}, output {S}x{S} u8 RGB, {a.windows} windows per variant taking turns, "
             f"{a.calls} launches per window after a warm-up of 20, device events, one process, "
             f"{torch.cuda.get_device_name(0)}",
             "ONE run on a shared box; us per launch: median (min .. max) over the windows.  Random bytes."]
    gate_ok = True
    for hs, ws in ((1080, 1920), (S, S)):
        bgr = random_bytes(1, B, hs, ws, 3).cuda()
        raws = {f: random_bytes(2 + i, B, rt.yuv_frame_layout(f, (hs, ws))[0]).cuda()
                for i, f in enumerate(("nv12", "i420", "yuyv"))}
        names = ["ppn_ingest_frames  bgr "] + [f"ppn_ingest_yuv     {f}" for f in raws]
        fns = [lambda: rt.ingest_frames(bgr, S, out=out, flip=False)] + [
            (lambda f=f: rt.ingest_yuv(raws[f], f, (hs, ws), S, out=out)) for f in raws]
        res = alternated(fns, lambda fn, n: launch_window(fn, n or a.calls), a.windows, 20)
        base = spread(res[0])[0]
        lines.append(f"{ws}x{hs} -> {S}x{S}:")
        for name, r, nbytes in zip(names, res, [bgr[0].numel()] + [v.shape[1] for v in raws.values()]):
            med, lo, hi = spread(r)
            lines.append(f"  {name}: {med:8.1f} us ({lo:7.1f} .. {hi:7.1f})  {med / base:5.2f} x bgr   "
                         f"{nbytes / 1e6:6.3f} MB source per image, {(B * nbytes + out.numel()) / med / 1e6:7.2f} TB/s if "
                         f"every source byte were read")
        if hs == 1080:
            ratio = spread(res[1])[0] / base
            gate_ok = ratio <= GATE
            lines.append(f"  GATE nv12 median <= {GATE:.2f} x bgr median: {ratio:.3f} -> {'met' if gate_ok else 'MISSED'}")
        del bgr, raws, fns
        torch.cuda.empty_cache()

    if not a.skip_pipeline:
        import bench
        from pytorch_pose_proposal_network_amd import drn, model, synth
        net = model.PoseProposalNet(drn.drn_d_22(), insize=(S, S), outsize=(S // 16, S // 16), compute_dtype="bfloat16").cuda()
        net.load_state_dict(synth.make_state_dict("drn_d_22", 0, bn_stats=bench.load_bn_stats("drn_d_22")))
        net.eval()
        pipe = rt.MultiLaneInference(net, B, (S, S), lanes=a.lanes)
        nv_s = random_bytes(7, B, rt.yuv_frame_layout("nv12", (S, S))[0]).pin_memory()
        nv_hd = random_bytes(8, B, rt.yuv_frame_layout("nv12", (1080, 1920))[0]).pin_memory()
        # the baseline's RGB frames are the 384 x 384 NV12 frames converted (by the ingest itself), so that the two 384 x 384
        # feeds put the same pictures through the network and the decode, whose time depends on the people it finds
        rgb = rt.ingest_yuv(nv_s.cuda(), "nv12", (S, S), S).cpu().pin_memory()
        people = [0, 0, 0]
        feeds = [("submit      384x384 RGB   ", rgb, lambda: pipe.submit(rgb, to_host=True)),
                 ("submit_raw  384x384 NV12  ", nv_s, lambda: pipe.submit_raw(nv_s, "nv12", (S, S), to_host=True)),
                 ("submit_raw  1920x1080 NV12", nv_hd, lambda: pipe.submit_raw(nv_hd, "nv12", (1080, 1920), to_host=True))]

        def pipeline_window(fn, n):
            """images/s of n batches: pinned frames -> H2D -> (ingest) -> forward -> decode -> compact result into pinned
            buffers, the host unpacking a batch while the later ones run (bench.py's PCIe-inclusive loop)."""
            n = n or a.steps
            pending = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            in_submit = 0.0
            for _ in range(n):
                ta = time.perf_counter()
                pending.append(fn())
                in_submit += time.perf_counter() - ta
                if len(pending) == a.lanes:
                    r = pending.pop(0)
                    r.ready.synchronize()
                    hosted = r.hosted.unpack()
            for r in pending:
                r.ready.synchronize()
                hosted = r.hosted.unpack()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            people[[f[2] for f in feeds].index(fn)] = sum(h["n"] for h in hosted)
            return B * n / dt, in_submit / n * 1e3

        res = alternated([f[2] for f in feeds], pipeline_window, a.windows, 2 * a.lanes + 2)
        submit_ms = [statistics.median(x[1] for x in r) for r in res]
        res = [[x[0] for x in r] for r in res]
        pipe.close()
        lines.append(f"PCIe-inclusive pipeline (MultiLaneInference, {a.lanes} lanes, bf16, fused decode, compact result back to "
                     f"pinned host memory): {a.windows} windows of {a.steps} batches per feed taking turns, host clock around a "
                     f"window that ends in a synchronise; images/s: median (min .. max).  Reported, not gated.")
        base = spread(res[0])[0]
        for (name, host, _), r, ms, n in zip(feeds, res, submit_ms, people):
            med, lo, hi = spread(r)
            per = host.shape[1] if host.dim() == 2 else host[0].numel()
            lines.append(f"  {name}: {med:8.0f} images/s ({lo:7.0f} .. {hi:7.0f})  {med / base:5.2f} x baseline   "
                         f"{per / 1e6:6.3f} MB per image over PCIe = {med * per / 1e9:6.2f} GB/s   host {ms:.3f} ms in the "
                         f"submit call per batch, {n} people in a batch")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")
    if not gate_ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
