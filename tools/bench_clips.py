"""Time the per-track skeleton clips (clips.PoseClips, csrc/clips.hip) at the serving batch: 32 images of 384 x 384 as 32 streams
of one frame and as one stream of 32 frames, T = 32, K = 18, on the decode of planted crowds as tools/bench_track.py plants
them.

    python tools/bench_clips.py [--out profiles/clips_bench.txt] [--calls 200] [--batch 32]

Device events around N calls after a warm-up.  Writes, per layout: us per ppn_clip_push beside ppn_track_update on the same
batch; us per ppn_clip_gather (as pushed, and with all 64 slots of every stream live and full) beside out.copy_() of a tensor
of the same size, the traffic floor; the only route there was before -- TrackResult.to_host() plus the bookkeeping on the
host, here the NumPy restatement of the rules (tests/clips_ref.py), wall clock, one run; and rt.inference_batch_clips beside
rt.inference_batch_tracked in the same run.  No threshold: the file is the record.  Without a GPU the file says "not
measured"."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_track import timed  # noqa: E402


def host_route(result, tracks, streams, frames, cfg):
    """What a caller had to do before: ids and centres to the host, the clips kept there.  Returns seconds."""
    import clips_ref as R
    t0 = time.perf_counter()
    rows = tracks.to_host()
    count = result.count.cpu().numpy()
    top = int(min(max(count.max(initial=0), 1), result.max_humans))
    kp, bb, sc = (t[:, :top].cpu().numpy() for t in (result.kp_cell, result.bbox, result.score))
    ids = np.full((len(rows), top), -1, np.int32)
    xy = np.zeros((len(rows), top, cfg["K"], 2), np.float32)
    for b, r in enumerate(rows):
        ids[b, :len(r["ids"])], xy[b, :len(r["ids"])] = r["ids"], r["xy"]
    st = R.fresh_state(streams, cfg["K"], cfg["length"])
    R.clip_push(cfg, st, count, kp, bb, sc, ids, xy, streams, frames)
    R.clip_gather(cfg, st, streams)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clips_bench.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (NumPy loops)")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not torch.cuda.is_available():
        text = (f"clips bench: batch {a.batch}, {a.size}x{a.size}: not measured (no GPU in this run; "
                f"python tools/bench_clips.py on an MI355X fills this file)\n")
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    import clips_ref as R
    from pytorch_pose_proposal_network_amd import clips, config, decode as D, prng, rt, synth, track

    B, S, T, K = a.batch, a.size, a.length, config.K
    g = S // 16
    heads = np.stack([synth.planted_crowd_head(7 + i, out_hw=(g, g)) for i in range(min(B, 4))])
    head = torch.from_numpy(heads).cuda().repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous()
    crowd = D.decode_heads(head, insize_hw=(S, S))
    del head
    counts = crowd.count.cpu().numpy()
    lines = [f"clips bench: batch {B}, {S}x{S}, max_humans {crowd.max_humans}, K {K}, T {T}, PoseClips defaults (max_gap 15, norm "
             f"root) behind Tracker defaults, {a.calls} calls after {a.warmup} warm-up, device events, one run, "
             f"{torch.cuda.get_device_name(0)}",
             "  the same batch is fed at every call, as in tools/bench_track.py (4 distinct planted crowds in turn); call times of "
             "back-to-back launches include the enqueue path, they are not kernel times",
             f"planted crowds: {int(counts.sum())} people in the batch, {int(counts.min())}..{int(counts.max())} per image"]
    cfg = R.make_cfg(K, T)
    for streams, frames in ((B, 1), (1, B)):
        tr = track.Tracker(streams, frames, crowd.max_humans)
        pc = clips.PoseClips(streams, frames, crowd.max_humans, length=T)
        t_track = timed(lambda: tr.update(crowd), a.calls, a.warmup)
        tracks = tr.update(crowd)
        t_push = timed(lambda: pc.push(crowd, tracks), a.calls, a.warmup)
        t_raw = timed(lambda: pc.push(crowd, tracks, smoothed=False), a.calls, a.warmup)
        live = (pc.state["id"] != 0).sum(1).cpu().numpy()
        lines.append(f"  (S={streams:2d}, frames={frames:2d}) ppn_clip_push: {t_push:8.1f} us per batch ({t_push / B:6.2f} us per image), "
                     f"without xy (box centres) {t_raw:8.1f} us; ppn_track_update on the same batch {t_track:8.1f} us; live clips "
                     f"{int(live.min())}..{int(live.max())} per stream, flags {sorted(set(pc.flags().tolist()))}")
        nbytes = pc.x.numel() * 4
        other = torch.empty_like(pc.x)
        t_copy = timed(lambda: other.copy_(pc.x), a.calls, a.warmup)
        t_g = timed(pc.gather, a.calls, a.warmup)
        pc.state["id"].copy_(torch.arange(1, 65, dtype=torch.int32).expand(streams, 64))     # every slot live and full
        pc.state["len"].fill_(T)
        pc.state["mask"].fill_((1 << K) - 1)
        pc.state["ring"].uniform_(0.0, float(S))
        pc.state["ref"].copy_(torch.tensor((10.0, 20.0, 200.0, 120.0)).cuda().expand(streams, 64, 4))
        t_full = timed(pc.gather, a.calls, a.warmup)
        pc.cfg.norm = clips.NORMS["none"]
        t_none = timed(pc.gather, a.calls, a.warmup)
        lines.append(f"  (S={streams:2d}, frames={frames:2d}) ppn_clip_gather of {nbytes / 1e6:6.2f} MB: as pushed {t_g:7.1f} us; all {streams * 64} "
                     f"slots live and full {t_full:7.1f} us = {2 * nbytes / t_full * 1e-6:5.2f} TB/s read + written (norm none: "
                     f"{t_none:7.1f} us); out.copy_() of the same size {t_copy:7.1f} us = {2 * nbytes / t_copy * 1e-6:5.2f} TB/s: "
                     f"the full gather is {t_full / t_copy:4.2f} x the copy")
        if not a.no_host:
            host = host_route(crowd, tracks, streams, frames, cfg)
            lines.append(f"  (S={streams:2d}, frames={frames:2d}) host route (TrackResult.to_host + NumPy restatement of push and gather, fresh "
                         f"clips, wall clock): {host * 1e6:11.0f} us")

    # beside the pipeline step: forward + fused decode + tracking, with and without the clips (synthetic weights; one stream)
    frames_u8 = torch.from_numpy(prng.u8_frames(3, B, (S, S))).cuda()
    model, _, _ = rt.network(image_size=S, state_dict=synth.make_state_dict("drn_d_22", 0), compute_dtype="bfloat16")
    dec = D.Decoder(B, (g, g), (S, S), model.local_grid_size)
    with torch.no_grad():
        for streams, frames in ((B, 1), (1, B)):
            tr = track.Tracker(streams, frames, dec.out.max_humans)
            pc = clips.PoseClips(streams, frames, dec.out.max_humans, length=T)
            t0 = timed(lambda: rt.inference_batch_tracked(frames_u8, model, tr, dec), a.calls, a.warmup)
            t1 = timed(lambda: rt.inference_batch_clips(frames_u8, model, tr, pc, dec, gather=False), a.calls, a.warmup)
            t2 = timed(lambda: rt.inference_batch_clips(frames_u8, model, tr, pc, dec), a.calls, a.warmup)
            lines.append(f"pipeline (drn_d_22 bf16, synthetic weights, random frames, S={streams:2d}, frames={frames:2d}): "
                         f"rt.inference_batch_tracked {t0:9.1f} us per batch = {B / (t0 * 1e-6):8.0f} images/s; "
                         f"rt.inference_batch_clips push only {t1:9.1f} us = {B / (t1 * 1e-6):8.0f} images/s, push + gather "
                         f"{t2:9.1f} us = {B / (t2 * 1e-6):8.0f} images/s; clip flags {sorted(set(pc.flags().tolist()))}")
    lines.append("not profiled: no rocprofv3 kernel trace or counter run of clip_push_kernel / clip_gather_kernel was taken; the "
                 "times above are call times (launch included), not kernel times")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
