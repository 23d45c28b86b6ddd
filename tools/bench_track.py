"""Time the device tracker (track.Tracker.update, csrc/track.hip) at the serving batch: 32 images of 384 x 384 as 32 streams of
one frame and as one stream of 32 frames, on the decode of planted crowds and on a sparse cut of it (at most 8 people per
image).

    python tools/bench_track.py [--out profiles/track_bench.txt] [--calls 200] [--batch 32]

Device events around N calls after a warm-up.  Writes, per layout and data set: us per update; the only route there was
before it -- a D2H of the people lists plus the association on the host, here the NumPy restatement of the rules
(tests/track_ref.py), wall clock, one run; and rt.inference_batch with and without tracking in the same run.
No threshold: the file is the record.  Without a GPU the file says "not measured"."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls          # us per call


def host_route(result, streams, frames, cfg):
    """What a caller had to do before: the people lists to the host, the association there.  Returns seconds."""
    import track_ref as R
    t0 = time.perf_counter()
    count = result.count.cpu().numpy()
    top = int(min(max(count.max(initial=0), 1), result.max_humans))
    kp, bb, sc = (t[:, :top].cpu().numpy() for t in (result.kp_cell, result.bbox, result.score))
    R.track_update(cfg, R.fresh_state(streams, cfg["K"]), count, kp, bb, sc, streams, frames)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_bench.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (tens of seconds of NumPy loops)")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not torch.cuda.is_available():
        text = (f"track bench: batch {a.batch}, {a.size}x{a.size}: not measured (no GPU in this run; "
                f"python tools/bench_track.py on an MI355X fills this file)\n")
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    import track_ref as R
    from pytorch_pose_proposal_network_amd import decode as D, prng, rt, synth, track

    B, S = a.batch, a.size
    g = S // 16
    heads = np.stack([synth.planted_crowd_head(7 + i, out_hw=(g, g)) for i in range(min(B, 4))])
    head = torch.from_numpy(heads).cuda().repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous()
    crowd = D.decode_heads(head, insize_hw=(S, S))
    del head
    sparse = D.DecodeResult(crowd.count.clamp(max=8), crowd.kp_cell, crowd.limb_arg, crowd.bbox, crowd.score,
                            crowd.max_humans)
    lines = [f"track bench: batch {B}, {S}x{S}, max_humans {crowd.max_humans}, K 18, Tracker defaults (iou_thr 0.3, kp_gate "
             f"0.1, min_close 3, max_age 15, alpha 1.0), {a.calls} calls after {a.warmup} warm-up, device events, one run, "
             f"{torch.cuda.get_device_name(0)}",
             "  the same batch is fed at every call: as 32 streams every stream sees its image again (all people matched); as "
             "one stream of 32 frames consecutive frames are different crowds (4 distinct images in turn: matching, ageing and "
             "births at every frame)"]
    cfg = R.make_cfg()
    for name, res in (("planted crowds", crowd), ("sparse (<= 8 people)", sparse)):
        counts = res.count.cpu().numpy()
        lines.append(f"{name}: {int(counts.sum())} people in the batch, {int(counts.min())}..{int(counts.max())} per image")
        for streams, frames in ((B, 1), (1, B)):
            tr = track.Tracker(streams, frames, res.max_humans)
            t_xy = timed(lambda: tr.update(res), a.calls, a.warmup)
            t_no = timed(lambda: tr.update(res, want_xy=False), a.calls, a.warmup)
            live = tr.live.cpu().numpy()
            line = (f"  (S={streams:2d}, T={frames:2d}) update: {t_xy:8.1f} us per batch ({t_xy / B:6.2f} us per image), without "
                    f"out_xy {t_no:8.1f} us; live tracks after the last frame {int(live.min())}..{int(live.max())}, flags "
                    f"{sorted(set(tr.flags().tolist()))}")
            if not a.no_host:
                host = host_route(res, streams, frames, cfg)
                line += f"; host route (to_host + NumPy restatement, fresh tracker, wall clock): {host * 1e6:11.0f} us"
            lines.append(line)

    # beside the pipeline step: forward + fused decode, with and without tracking (synthetic weights; one stream)
    frames_u8 = torch.from_numpy(prng.u8_frames(3, B, (S, S))).cuda()
    model, _, _ = rt.network(image_size=S, state_dict=synth.make_state_dict("drn_d_22", 0), compute_dtype="bfloat16")
    dec = D.Decoder(B, (g, g), (S, S), model.local_grid_size)
    with torch.no_grad():
        t_plain = timed(lambda: rt.inference_batch(frames_u8, model, dec), a.calls, a.warmup)
        pc = rt.inference_batch(frames_u8, model, dec).count.cpu().numpy()
        lines.append(f"pipeline (rt.inference_batch, drn_d_22 bf16, synthetic weights, random frames: {int(pc.min())}..{int(pc.max())} "
                     f"people per image, one stream): {t_plain:9.1f} us per batch = {B / (t_plain * 1e-6):8.0f} images/s")
        for streams, frames in ((B, 1), (1, B)):
            tr = track.Tracker(streams, frames, dec.out.max_humans)
            t = timed(lambda: rt.inference_batch_tracked(frames_u8, model, tr, dec), a.calls, a.warmup)
            lines.append(f"pipeline with tracking (rt.inference_batch_tracked, S={streams:2d}, T={frames:2d})          : {t:9.1f} us "
                         f"per batch = {B / (t * 1e-6):8.0f} images/s")
    lines.append("not profiled: no rocprofv3 kernel trace or counter run of track_kernel was taken; the times above are call "
                 "times (launch included), not kernel times")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
