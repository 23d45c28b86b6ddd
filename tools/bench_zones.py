"""Time the zones and counting lines (zones.Zones, csrc/zones.hip) at the serving batch: 32 images of 384 x 384 as 32 streams
of one frame and as one stream of 32 frames, K = 18, 4 zones and 4 lines per stream, on the decode of planted crowds as
tools/bench_track.py plants them.

    python tools/bench_zones.py [--out profiles/zones_bench.txt] [--calls 200] [--batch 32]

Device events around N calls after a warm-up.  Writes, per layout: us per ppn_zone_update beside ppn_clip_push and
ppn_track_update on the same batch in the same run (the yardsticks: it does the clips' match plus a few hundred flops per
slot); the only route there was before -- TrackResult.to_host() plus the bookkeeping on the host, here the NumPy restatement
of the rules (tests/zones_ref.py), wall clock, one run; and rt.inference_batch_zones beside rt.inference_batch_tracked in the
same run.  No threshold: the file is the record.  Without a GPU the file says "not measured"."""
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


def geometry(size):
    """Four zones (a quadrant, a triangle, a concave 8-gon, the whole image) and four lines (a horizontal, a vertical, two
    diagonals), in pixels of a size x size image."""
    u = size / 8.0
    zones = [[(0, 0), (4 * u, 0), (4 * u, 4 * u), (0, 4 * u)],
             [(4 * u, u), (7.5 * u, 7 * u), (u, 6.5 * u)],
             [(u, u), (7 * u, u), (7 * u, 7 * u), (5 * u, 7 * u), (5 * u, 3 * u), (3 * u, 3 * u), (3 * u, 7 * u), (u, 7 * u)],
             [(0, 0), (size, 0), (size, size), (0, size)]]
    lines = [(0, 4 * u, size, 4 * u), (4 * u, 0, 4 * u, size), (0, 0, size, size), (0, size, size, 0)]
    return zones, lines


def host_route(result, tracks, streams, frames, cfg, geom):
    """What a caller had to do before: ids and centres to the host, the zones kept there.  Returns seconds."""
    import zones_ref as R
    t0 = time.perf_counter()
    rows = tracks.to_host()
    count = result.count.cpu().numpy()
    top = int(min(max(count.max(initial=0), 1), result.max_humans))
    kp, bb = (t[:, :top].cpu().numpy() for t in (result.kp_cell, result.bbox))
    ids = np.full((len(rows), top), -1, np.int32)
    xy = np.zeros((len(rows), top, cfg["K"], 2), np.float32)
    for b, r in enumerate(rows):
        ids[b, :len(r["ids"])], xy[b, :len(r["ids"])] = r["ids"], r["xy"]
    R.zone_update(cfg, geom, R.fresh_state(streams), count, kp, bb, ids, xy, streams, frames)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zones_bench.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (NumPy loops)")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not torch.cuda.is_available():
        text = (f"zones bench: batch {a.batch}, {a.size}x{a.size}: not measured (no GPU in this run; "
                f"python tools/bench_zones.py on an MI355X fills this file)\n")
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    import zones_ref as R
    from pytorch_pose_proposal_network_amd import clips, config, decode as D, prng, rt, synth, track, zones

    B, S, K = a.batch, a.size, config.K
    g = S // 16
    heads = np.stack([synth.planted_crowd_head(7 + i, out_hw=(g, g)) for i in range(min(B, 4))])
    head = torch.from_numpy(heads).cuda().repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous()
    crowd = D.decode_heads(head, insize_hw=(S, S))
    del head
    counts = crowd.count.cpu().numpy()
    zone_list, line_list = geometry(S)
    lines = [f"zones bench: batch {B}, {S}x{S}, max_humans {crowd.max_humans}, K {K}, {len(zone_list)} zones (4, 3, 8 and 4 "
             f"vertices) and {len(line_list)} lines per stream, Zones defaults (max_gap 15, anchor center, loiter 1) behind Tracker "
             f"defaults, {a.calls} calls after {a.warmup} warm-up, device events, one run, {torch.cuda.get_device_name(0)}",
             "  the same batch is fed at every call, as in tools/bench_track.py (4 distinct planted crowds in turn); call times of "
             "back-to-back launches include the enqueue path, they are not kernel times",
             f"planted crowds: {int(counts.sum())} people in the batch, {int(counts.min())}..{int(counts.max())} per image"]

    def make(streams, frames, max_humans):
        z = zones.Zones(streams, frames, max_humans)
        for s in range(streams):
            z.set_zones(s, zone_list)
            z.set_lines(s, line_list)
        return z

    cfg = R.make_cfg(K)
    for streams, frames in ((B, 1), (1, B)):
        tr = track.Tracker(streams, frames, crowd.max_humans)
        pc = clips.PoseClips(streams, frames, crowd.max_humans)
        z = make(streams, frames, crowd.max_humans)
        t_track = timed(lambda: tr.update(crowd), a.calls, a.warmup)
        tracks = tr.update(crowd)
        t_push = timed(lambda: pc.push(crowd, tracks), a.calls, a.warmup)
        t_zone = timed(lambda: z.update(crowd, tracks), a.calls, a.warmup)
        t_raw = timed(lambda: z.update(crowd, tracks, smoothed=False), a.calls, a.warmup)
        res = z.update(crowd, tracks)
        live = (z.state["id"] != 0).sum(1).cpu().numpy()
        occ = res.zone[:, :len(zone_list), 0].sum(0).tolist()
        lines.append(f"  (S={streams:2d}, frames={frames:2d}) ppn_zone_update: {t_zone:8.1f} us per batch ({t_zone / B:6.2f} us per image), "
                     f"without xy (box centres) {t_raw:8.1f} us; on the same batch ppn_clip_push {t_push:8.1f} us, ppn_track_update "
                     f"{t_track:8.1f} us: {t_zone / t_push:4.2f} x the push, {t_zone / t_track:4.2f} x the tracker; live slots "
                     f"{int(live.min())}..{int(live.max())} per stream, occupancy of the batch per zone {occ}, flags "
                     f"{sorted(set(z.flags().tolist()))}")
        if not a.no_host:
            geom = R.make_geom([zone_list] * streams, [line_list] * streams)
            host = host_route(crowd, tracks, streams, frames, cfg, geom)
            lines.append(f"  (S={streams:2d}, frames={frames:2d}) host route (TrackResult.to_host + NumPy restatement of the update, fresh "
                         f"state, wall clock): {host * 1e6:11.0f} us")

    # beside the pipeline step: forward + fused decode + tracking, with and without the zones (synthetic weights)
    frames_u8 = torch.from_numpy(prng.u8_frames(3, B, (S, S))).cuda()
    model, _, _ = rt.network(image_size=S, state_dict=synth.make_state_dict("drn_d_22", 0), compute_dtype="bfloat16")
    dec = D.Decoder(B, (g, g), (S, S), model.local_grid_size)
    with torch.no_grad():
        for streams, frames in ((B, 1), (1, B)):
            tr = track.Tracker(streams, frames, dec.out.max_humans)
            z = make(streams, frames, dec.out.max_humans)
            t0 = timed(lambda: rt.inference_batch_tracked(frames_u8, model, tr, dec), a.calls, a.warmup)
            t1 = timed(lambda: rt.inference_batch_zones(frames_u8, model, tr, z, dec), a.calls, a.warmup)
            lines.append(f"pipeline (drn_d_22 bf16, synthetic weights, random frames, S={streams:2d}, frames={frames:2d}): "
                         f"rt.inference_batch_tracked {t0:9.1f} us per batch = {B / (t0 * 1e-6):8.0f} images/s; "
                         f"rt.inference_batch_zones {t1:9.1f} us = {B / (t1 * 1e-6):8.0f} images/s; zone flags "
                         f"{sorted(set(z.flags().tolist()))}")
    lines.append("not profiled: no rocprofv3 kernel trace or counter run of zone_update_kernel was taken; the times above are "
                 "call times (launch included), not kernel times")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
