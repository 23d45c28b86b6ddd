"""Time the re-identification (reid.ReId; csrc/reid.hip ppn_people_descr, ppn_reid_update).

    python tools/bench_reid.py [--out profiles/reid_bench.txt] [--calls 200]

Device events around N back-to-back calls after a warm-up (tools/bench_track.py's `timed`).  Writes:
  * the descriptor launch on 8 frames of 1080p NV12 with 16 people each (tools/bench_crops.py's planted people) beside
    ppn_ingest_rois on the same rectangle table, in the same process;
  * the gallery launch at the serving batch (32 images of 384 x 384, tools/bench_zones.py's planted crowds), as 32 streams of
    one frame and as one stream of 32 frames, beside ppn_zone_update and ppn_track_update on the same batch;
  * rt.inference_reid beside rt.inference_crops(..., tracker=) on the same frames;
  * the host route: ReIdResult.to_host() plus the NumPy restatement (tests/reid_ref.py), wall clock.
No threshold: the file is the record.  Without a GPU the file says "not measured"."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
sys.path.insert(2, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_crops import planted_people  # noqa: E402
from bench_track import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reid_bench.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--people", type=int, default=16)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (NumPy loops)")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    Fr, P, S, B, (H, W), out_hw = a.frames, a.people, a.size, a.batch, (1080, 1920), (256, 128)
    head = f"reid bench: {Fr} frames of {W}x{H} NV12 with {P} people each; gallery at batch {B} of {S}x{S}"
    if not torch.cuda.is_available():
        text = f"{head}: not measured (no GPU in this run; python tools/bench_reid.py on an MI355X fills this file)\n"
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    import reid_ref as R
    from pytorch_pose_proposal_network_amd import config, crops as Cr, decode as D, reid as Re, rt, synth, track, windows as Wn, zones

    lines = [f"{head}, {a.calls} back-to-back calls after a warm-up of {a.warmup}, device events, one process, "
             f"{torch.cuda.get_device_name(0)}",
             "ONE run on a shared box; us per call.  These are call times of back-to-back launches (launch and ctypes overhead "
             "included), not kernel times; no kernel trace was taken.  Nothing here says anything about identification accuracy."]

    # ---- the descriptor launch beside ppn_ingest_rois on the same table
    nbytes = rt.yuv_frame_layout("nv12", (H, W))[0]
    gen = torch.Generator(device="cuda").manual_seed(1)
    raw = torch.randint(0, 256, (Fr, nbytes), dtype=torch.uint8, device="cuda", generator=gen)
    M, K = 576, 18
    count, kp, bb, sc = planted_people(Fr, (H, W), M, K, P, 7)
    res = D.DecodeResult(torch.from_numpy(count).cuda(), torch.from_numpy(kp).cuda(),
                         torch.zeros(Fr, M, 1, dtype=torch.int32, device="cuda"), torch.from_numpy(bb).cuda(),
                         torch.from_numpy(sc).cuda(), M)
    r = Re.ReId(1, Fr, M, (H, W), "nv12", max_rois=P)
    r.rects(res)
    roi = r.roi.cpu().numpy()
    assert (r.status.cpu().numpy() == 0).all(), "the planted people must all give a rectangle"
    crops_out = torch.empty(Fr * P, out_hw[0], out_hw[1], 3, dtype=torch.uint8, device="cuda")
    t_rect = timed(lambda: r.rects(res), a.calls, a.warmup)
    t_descr = timed(lambda: r.describe(raw), a.calls, a.warmup)
    t_ing = timed(lambda: Cr.ingest_rois(raw, "nv12", (H, W), r.roi, out_hw, crops_out), a.calls, a.warmup)
    t_descr2 = timed(lambda: r.describe(raw), a.calls, a.warmup)
    r.roi.zero_()
    r.status.fill_(1)
    t_empty = timed(lambda: r.describe(raw), a.calls, a.warmup)
    r.rects(res)
    r.describe(raw)
    assert int(r.valid.sum()) == Fr * P
    lines += [f"descriptors of {Fr} x {P} rectangles ({int(roi[..., 2].min())}..{int(roi[..., 2].max())} rows x "
              f"{int(roi[..., 3].min())}..{int(roi[..., 3].max())} columns), 3072 samples each, random bytes:",
              f"  ppn_people_rois (mode people, max_humans {M})            : {t_rect:8.1f} us",
              f"  ppn_people_descr                                        : {t_descr:8.1f} us, again after the ingest {t_descr2:8.1f} us",
              f"  ppn_people_descr, every slot empty (no read)            : {t_empty:8.1f} us",
              f"  ppn_ingest_rois, the same table, crops of {out_hw[1]}x{out_hw[0]}      : {t_ing:8.1f} us",
              f"  ratio descr / ingest_rois: {t_descr / t_ing:.3f}"]
    if t_descr > 2.0 * t_ing:
        lines.append("  the descriptor launch is above twice the ingest although it reads fewer bytes and writes almost nothing; "
                     "SUPPOSED, not measured: its 36 byte loads per work item are scattered over the rectangle's rows (one "
                     "cache line per few samples), so the launch waits for latency, not bandwidth")

    # ---- the gallery launch at the serving batch
    g = S // 16
    heads = np.stack([synth.planted_crowd_head(7 + i, out_hw=(g, g)) for i in range(min(B, 4))])
    hd = torch.from_numpy(heads).cuda().repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous()
    crowd = D.decode_heads(hd, insize_hw=(S, S))
    del hd
    counts = crowd.count.cpu().numpy()
    frames_bgr = torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=gen)
    lines.append(f"gallery: batch {B}, {S}x{S} packed BGR, max_humans {crowd.max_humans}, max_rois 64, ReId defaults behind Tracker "
                 f"defaults, planted crowds of {int(counts.min())}..{int(counts.max())} people per image, the same batch at every call:")
    for streams, frames in ((B, 1), (1, B)):
        tr = track.Tracker(streams, frames, crowd.max_humans)
        z = zones.Zones(streams, frames, crowd.max_humans)
        rg = Re.ReId(streams, frames, crowd.max_humans, (S, S), "bgr")
        t_track = timed(lambda: tr.update(crowd), a.calls, a.warmup)
        tracks = tr.update(crowd)
        rg.rects(crowd)
        rg.describe(frames_bgr)
        t_zone = timed(lambda: z.update(crowd, tracks), a.calls, a.warmup)
        t_reid = timed(lambda: rg.update(crowd, tracks), a.calls, a.warmup)
        t_d = timed(lambda: rg.describe(frames_bgr), a.calls, a.warmup)
        out = rg.update(crowd, tracks)
        live = out.live.cpu().numpy()
        lines.append(f"  (S={streams:2d}, frames={frames:2d}) ppn_reid_update {t_reid:8.1f} us per batch; on the same batch ppn_zone_update "
                     f"{t_zone:8.1f} us, ppn_track_update {t_track:8.1f} us: {t_reid / t_zone:4.2f} x the zones, "
                     f"{t_reid / t_track:4.2f} x the tracker; ppn_people_descr of {B} x 64 slots ({int(rg.valid.sum())} valid) "
                     f"{t_d:8.1f} us; live entries {int(live.min())}..{int(live.max())}, flags {sorted(set(rg.flags().tolist()))}")
        if not a.no_host:
            t0 = time.perf_counter()
            host = out.to_host()
            ids = tracks.ids.cpu().numpy()
            cnt = crowd.count.cpu().numpy()
            t1 = time.perf_counter()
            R.reid_update(R.make_cfg(thr=rg.thr), R.fresh_state(streams), cnt, ids, host["descr"], host["valid"], streams, frames)
            t2 = time.perf_counter()
            lines.append(f"  (S={streams:2d}, frames={frames:2d}) host route, wall clock: to_host {1e6 * (t1 - t0):9.0f} us + NumPy restatement "
                         f"of the update on a fresh state {1e6 * (t2 - t1):11.0f} us")
    if not a.no_host:
        t0 = time.perf_counter()
        R.people_descr(raw[:1].cpu().numpy(), "nv12", H, W, roi[:1], np.zeros((1, P), np.int32))
        lines.append(f"  host route of the descriptors, wall clock: NumPy restatement of ONE frame's {P} rectangles "
                     f"{1e6 * (time.perf_counter() - t0):11.0f} us")

    # ---- beside the pipeline step (synthetic weights; one stream)
    model, _, _ = rt.network(image_size=S, state_dict=synth.make_state_dict("drn_d_22", 0), compute_dtype="bfloat16")
    tiles = Wn.WindowLayout.tiles((H, W), 2, 2)
    dec = D.Decoder(Fr * tiles.n, (g, g), (S, S), model.local_grid_size)
    merger = Wn.WindowMerger(tiles, Fr, (S, S), dec.out.max_humans)
    cropper = Cr.PersonCropper(Fr, merger.max_out, (H, W), "nv12", out_hw, max_crops=P)
    rp = Re.ReId(1, Fr, merger.max_out, (H, W), "nv12", max_rois=P)
    tr_c, tr_r = track.Tracker(1, Fr, merger.max_out), track.Tracker(1, Fr, merger.max_out)
    with torch.no_grad():
        t_c = timed(lambda: rt.inference_crops(raw, "nv12", (H, W), model, cropper, tiles, tracker=tr_c, decoder=dec,
                                               merger=merger, size=S), a.calls, a.warmup)
        t_r = timed(lambda: rt.inference_reid(raw, "nv12", (H, W), model, tr_r, rp, tiles, decoder=dec, merger=merger, size=S),
                    a.calls, a.warmup)
        t_c2 = timed(lambda: rt.inference_crops(raw, "nv12", (H, W), model, cropper, tiles, tracker=tr_c, decoder=dec,
                                                merger=merger, size=S), a.calls, a.warmup)
    lines += [f"pipeline (drn_d_22 bf16, synthetic weights, random frames, 2 x 2 layout, fused decode, one stream of {Fr} frames):",
              f"  rt.inference_crops(..., tracker=): {t_c:9.1f} us, again after the other {t_c2:9.1f} us",
              f"  rt.inference_reid                : {t_r:9.1f} us ({int(rp.valid.sum())} of {Fr * P} slots described); ratio reid / "
              f"crops {t_r / t_c:.3f}",
              "not profiled: no rocprofv3 kernel trace or counter run of people_descr_kernel or reid_update_kernel was taken"]
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
