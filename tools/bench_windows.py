"""Time the windowed inference (windows.py; csrc/ingest.hip ppn_ingest_windows, csrc/windows.hip ppn_merge_windows) at the
serving batch: 8 frames of 1080p NV12 under a 2 x 2 layout = 32 images of 384 x 384.

    python tools/bench_windows.py [--out profiles/windows_bench.txt] [--calls 200] [--rounds 6]

Device events around N back-to-back calls after a warm-up; two variants that are compared take turns, `rounds` windows each,
and the file gives the median (min .. max) over the windows.  Writes:
  * the window ingest launch beside ppn_ingest_yuv on 32 whole 1080p frames (the same 14.2 MB of output; the whole-frame
    entry, unchanged bytes);
  * the merge launch on planted crowds that stand in the overlaps of the windows, with and without keypoint fusion;
  * rt.inference_windows beside rt.ingest_yuv + rt.inference_batch on the same batch.
No threshold: the file is the record.  Without a GPU the file says "not measured"."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls          # us per call


def in_turns(fns, calls, warmup, rounds):
    """Per fn the us per call of `rounds` windows, the fns taking turns."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            times[i].append(window(fn, calls))
    return times


def fmt(ts):
    return f"{statistics.median(ts):9.1f} us ({min(ts):8.1f} .. {max(ts):8.1f})"


def planted_overlap_crowd(layout, frames, in_hw, M, K, people, seed):
    """A DecodeResult's arrays: per frame `people` people whose root boxes lie in the bands that windows share; every
    window that holds a root box sees a copy (moved by up to a pixel, its own scores, a random half of the keypoints)."""
    rng = np.random.default_rng(seed)
    n = layout.n
    count = np.zeros(frames * n, np.int32)
    kp = np.full((frames * n, M, K), -1, np.int32)
    bb = np.zeros((frames * n, M, K, 4), np.float32)
    sc = np.zeros((frames * n, M, K), np.float32)
    H, W = layout.src_hw
    ys = sorted({w[0] for w in layout.windows})
    xs = sorted({w[1] for w in layout.windows})
    wh, ww = layout.windows[0][2], layout.windows[0][3]
    band_y = (ys[1], ys[0] + wh) if len(ys) > 1 else (0, H)          # rows that two window rows share
    band_x = (xs[1], xs[0] + ww) if len(xs) > 1 else (0, W)
    for f in range(frames):
        for _ in range(people):
            h, w = rng.integers(60, 160), rng.integers(30, 80)
            if rng.random() < 0.5:                                    # in the horizontal band, anywhere along it
                y, x = rng.integers(band_y[0], max(band_y[1] - h, band_y[0] + 1)), rng.integers(0, W - w)
            else:
                y, x = rng.integers(0, H - h), rng.integers(band_x[0], max(band_x[1] - w, band_x[0] + 1))
            for i, (wy, wx, hh, wd) in enumerate(layout.windows):
                b = f * n + i
                if not (wy <= y and y + h <= wy + hh and wx <= x and x + w <= wx + wd) or count[b] >= M:
                    continue
                sy, sx = in_hw[0] / hh, in_hw[1] / wd
                j = rng.random(4) * 2 - 1
                root = np.array([(y - wy + j[0]) * sy, (x - wx + j[1]) * sx, (y + h - wy + j[2]) * sy, (x + w - wx + j[3]) * sx])
                p = count[b]
                count[b] += 1
                kp[b, p, 0], bb[b, p, 0], sc[b, p, 0] = 1, root, rng.random()
                for k in rng.choice(np.arange(1, K), (K - 1) // 2, False):
                    kp[b, p, k], sc[b, p, k] = 1, rng.random()
                    bb[b, p, k] = (root[0] + k, root[1] + k % 4, root[0] + k + 6, root[1] + k % 4 + 6)
    for b in range(frames * n):                                       # the decode lists people by descending root score
        o = np.argsort(-sc[b, :count[b], 0], kind="stable")
        kp[b, :count[b]], bb[b, :count[b]], sc[b, :count[b]] = kp[b, :count[b]][o], bb[b, :count[b]][o], sc[b, :count[b]][o]
    return count, kp, bb, sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_bench.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=384)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    Fr, S, (H, W) = a.frames, a.size, (1080, 1920)
    head = f"windows bench: {Fr} frames of {W}x{H} NV12, 2 x 2 layout, batch {4 * Fr} at {S}x{S}"
    if not torch.cuda.is_available():
        text = f"{head}: not measured (no GPU in this run; python tools/bench_windows.py on an MI355X fills this file)\n"
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    from pytorch_pose_proposal_network_amd import decode as D, rt, synth, windows as Wn

    lay = Wn.WindowLayout.tiles((H, W), 2, 2)
    B = Fr * lay.n
    nbytes = rt.yuv_frame_layout("nv12", (H, W))[0]
    gen = torch.Generator(device="cuda").manual_seed(1)
    raw = torch.randint(0, 256, (B, nbytes), dtype=torch.uint8, device="cuda", generator=gen)      # B whole frames; the first Fr feed the windows
    lines = [f"{head}, {a.calls} back-to-back calls per window after a warm-up of {a.warmup}, {a.rounds} windows per variant "
             f"taking turns, device events, one process, {torch.cuda.get_device_name(0)}",
             "ONE run on a shared box; us per call: median (min .. max) over the windows.  Random bytes.",
             f"layout: {list(lay.windows)}"]

    # ---- the ingest launch
    out_w = torch.empty(B, S, S, 3, dtype=torch.uint8, device="cuda")
    out_y = torch.empty(B, S, S, 3, dtype=torch.uint8, device="cuda")
    t_w, t_y = in_turns([lambda: Wn.ingest_windows(raw[:Fr], "nv12", lay, S, out_w),
                         lambda: rt.ingest_yuv(raw, "nv12", (H, W), S, out_y)], a.calls, a.warmup, a.rounds)
    lines += [f"ingest, {B} images of {S}x{S} out ({out_w.numel() / 1e6:.1f} MB written):",
              f"  ppn_ingest_windows  {Fr} frames x {lay.n} windows of {lay.windows[0][3]}x{lay.windows[0][2]}: {fmt(t_w)}   "
              f"{Fr * nbytes / 1e6:7.1f} MB of source",
              f"  ppn_ingest_yuv      {B} whole frames (the whole-frame entry, unchanged bytes): {fmt(t_y)}   {B * nbytes / 1e6:7.1f} MB of source",
              f"  ratio of the medians windows / whole frames: {statistics.median(t_w) / statistics.median(t_y):.3f}"]

    # ---- the merge launch
    M, K = (S // 16) ** 2, 18
    for people in (12, 60):
        count, kp, bb, sc = planted_overlap_crowd(lay, Fr, (S, S), M, K, people, 100 + people)
        res = D.DecodeResult(torch.from_numpy(count).cuda(), torch.from_numpy(kp).cuda(),
                             torch.zeros(B, M, 1, dtype=torch.int32, device="cuda"), torch.from_numpy(bb).cuda(),
                             torch.from_numpy(sc).cuda(), M)
        fused, plain = (Wn.WindowMerger(lay, Fr, (S, S), M, fuse=fz) for fz in (True, False))
        t_f, t_p = in_turns([lambda: fused(res), lambda: plain(res)], a.calls, a.warmup, a.rounds)
        kept = fused.out.count.cpu().numpy()
        cand = count.reshape(Fr, lay.n).sum(1)
        lines += [f"merge, {people} planted people per frame in the overlaps: {int(cand.min())}..{int(cand.max())} candidates per "
                  f"frame, {int(kept.min())}..{int(kept.max())} kept, flags {sorted(set(fused.flags.cpu().tolist()))}, max_humans {M}, "
                  f"max_out {fused.max_out}, one workgroup per frame:",
                  f"  ppn_merge_windows fuse=1: {fmt(t_f)} per call of {Fr} frames",
                  f"  ppn_merge_windows fuse=0: {fmt(t_p)}"]

    # ---- beside the pipeline step (synthetic weights; one stream)
    model, _, _ = rt.network(image_size=S, state_dict=synth.make_state_dict("drn_d_22", 0), compute_dtype="bfloat16")
    g = S // 16
    dec = D.Decoder(B, (g, g), (S, S), model.local_grid_size)
    merger = Wn.WindowMerger(lay, Fr, (S, S), dec.out.max_humans)
    with torch.no_grad():
        def whole():
            return rt.inference_batch(rt.ingest_yuv(raw, "nv12", (H, W), S, model.input_buffer(B, S, S, True, True)), model, dec)

        def windowed():
            return rt.inference_windows(raw[:Fr], "nv12", (H, W), model, lay, dec, merger, size=S)

        t_b, t_i = in_turns([whole, windowed], a.calls, a.warmup, a.rounds)
        pc = windowed().count.cpu().numpy()
    lines += [f"pipeline (drn_d_22 bf16, synthetic weights, random frames, fused decode, one stream), batch {B}:",
              f"  rt.ingest_yuv of {B} whole frames + rt.inference_batch: {fmt(t_b)} = {B / (statistics.median(t_b) * 1e-6):8.0f} images/s",
              f"  rt.inference_windows of {Fr} frames ({int(pc.min())}..{int(pc.max())} people per frame after the merge)  : {fmt(t_i)} = "
              f"{B / (statistics.median(t_i) * 1e-6):8.0f} images/s = {Fr / (statistics.median(t_i) * 1e-6):7.0f} frames/s",
              "not profiled: no rocprofv3 kernel trace or counter run of ingest_windows_kernel or merge_kernel was taken; the times "
              "above are call times of back-to-back launches (launch and ctypes overhead included), not kernel times"]
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
