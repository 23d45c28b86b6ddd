"""Single-frame latency of the inference path: DRN-D-22 at 384 x 384, batches 1 / 2 / 4, bfloat16 and float32.

    python tools/bench_latency.py [--root OTHER_CHECKOUT] [--latency 0|1] [--reps 300] [--out FILE]

For each dtype and batch it builds one model, warms the plan up (the first two runs launch directly, the third captures the
hipGraph) and reports, over `--reps` repetitions on a side stream (the legacy default stream is never captured):

  * forward: HIP-event time of `forward_u8` (the plan's graph launch), median and p90 in microseconds;
  * batch 1 only: the wall time of `rt.inference(frame, ...)` -- upload excluded (the frame is on the device), forward +
    decode + the read-back of the people list, host clock around a call that ends in a device synchronise;
  * a per-launch table from HIP events (`profile_layers`, 20 back-to-back launches per entry): every launch of the plan,
    `*` in front of the ones that ran as split-K pairs.

`--root` imports the package from another checkout (e.g. the parent commit with its library built), so the same script
measures both sides of a change in one session on one box; `--latency 1` asks for latency plans where the package has them.
Weights are the seeded synthetic checkpoint with calibrated BatchNorm statistics; the frame is seeded noise.
"""
import argparse
import inspect
import os
import sys
import time

import numpy as np


def pct(v, p):
    return float(np.percentile(np.asarray(v), p))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--latency", type=int, default=1)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--dtypes", default="bfloat16,float32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from pytorch_pose_proposal_network_amd import model as M, prng, rt, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_latency.py measures on the GPU: none found")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    has_latency = "latency" in inspect.signature(M.PoseProposalNet.__init__).parameters
    want = bool(args.latency) and has_latency
    say(f"# bench_latency: {torch.cuda.get_device_name(0)}, package {os.path.abspath(args.root)}, "
        f"latency plans {'ON' if want else 'off'}{'' if has_latency else ' (this tree has none)'}, reps {args.reps}")
    data = os.path.join(os.path.abspath(args.root), "pytorch_pose_proposal_network_amd", "data", "bn_calib_drn_d_22_seed0.npz")
    st_ = np.load(data)
    sd = synth.make_state_dict("drn_d_22", 0, bn_stats={k: st_[k] for k in st_.files})
    stream = torch.cuda.Stream()
    for dtype in args.dtypes.split(","):
        kw = dict(compute_dtype=dtype)
        if has_latency:
            kw["latency"] = want
        net = M.PoseProposalNet("drn_d_22", insize=(384, 384), outsize=(24, 24), **kw).cuda()
        net.load_state_dict(sd)
        net.eval()
        for batch in (int(b) for b in args.batches.split(",")):
            u8 = torch.from_numpy(prng.u8_frames(1000 + batch, batch, (384, 384))).cuda()
            with torch.cuda.stream(stream):
                buf = net.input_buffer(batch, 384, 384)
                buf.copy_(u8)
                for _ in range(10):                                # direct, direct, capture, replays
                    net.forward_u8(buf)
                stream.synchronize()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
                for a, b in ev:
                    a.record(stream)
                    net.forward_u8(buf)
                    b.record(stream)
                    stream.synchronize()                          # one frame at a time: no queueing behind the previous one
                fwd = [a.elapsed_time(b) * 1e3 for a, b in ev]
                caps = sum(net.graph_captures().values())
                say(f"{dtype:9s} batch {batch}  forward_u8 (graph, {caps} capture(s))  median {pct(fwd, 50):8.1f} us  "
                    f"p90 {pct(fwd, 90):8.1f} us  min {min(fwd):8.1f} us")
                if batch == 1:
                    for _ in range(5):
                        rt.inference(buf, net, (24, 24), (21, 21))
                    wall = []
                    for _ in range(args.reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        rt.inference(buf, net, (24, 24), (21, 21))   # ends in the read-back of the people list
                        wall.append((time.perf_counter() - t0) * 1e6)
                    say(f"{dtype:9s} batch 1  rt.inference (forward + decode + read-back, wall)  median {pct(wall, 50):8.1f} us  "
                        f"p90 {pct(wall, 90):8.1f} us")
                rows = net.profile_layers(buf, src_is_u8=True, repeats=20)
                rows = [min(r, key=lambda x: x[2]) for r in zip(*[rows] + [net.profile_layers(buf, src_is_u8=True, repeats=20)
                                                                          for _ in range(2)])]
                say(f"  per-launch (HIP events, best of 3 x 20 back-to-back launches), {dtype} batch {batch}: "
                    f"sum {sum(r[2] for r in rows) * 1e3:.1f} us")
                for name, kern, ms, _ in rows:
                    say(f"   {'*' if 'conv_splitk' in kern else ' '} {name:34s} {ms * 1e3:8.2f} us  {kern}")
        del net
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
