"""Time drawing onto raw video surfaces (render.Renderer.draw_yuv over ppn_draw_humans_yuv) at 1080p.

    python tools/bench_render_yuv.py [--out profiles/render_yuv.txt] [--frames 8] [--calls 200] [--windows 7]

Workload: 8 frames of 1920 x 1080 with 12 and with 60 planted people per frame; NV12, I420 and YUYV, in place and out of
place.  Beside them, in the same run and on the same people, ppn_draw_humans in place on RGB frames of that size: the
comparison, since before this there was no route from a drawn RGB frame back to YUV.  Each figure is the median over
`windows` windows of `calls` back-to-back calls between two device events, after a warm-up of every variant, the variants
taking turns window by window.  At this size a call's two launches take a few tens of microseconds, so such a window also
measures the enqueue path (ctypes, the argument checks, two launches), not the kernels alone.  Beside the times: the bytes
each variant must move (in place the painted samples, counted by drawing on an all-0 and an all-255 surface; out of place
1.5 or 2 bytes per pixel read and written).  On top, computed on the host: how a drawn colour looks after the ingest's
YUV -> RGB rule (ppn_rgb_to_yuv, then ppn_ingest_yuv's pixel rule; the two tables come from different constants).
No threshold: the file is the record.  Without a GPU the timing part says "not measured"."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SETS = [("bt601", False), ("bt709", False), ("bt601", True), ("bt709", True)]


def round_trip_lines():
    """|ingest rule(forward rule(c)) - c| per channel over the default palette and the grid's grey, per colour set."""
    from pytorch_pose_proposal_network_amd import lib as L, render as R
    l = L.load()
    rgb = np.array(list(R.default_palette()) + [(110, 110, 110)], np.uint8)
    lines = [f"colour round trip (host): {len(rgb) - 1} palette colours + the grid's grey through ppn_rgb_to_yuv, then ppn_ingest_yuv's "
             "pixel rule; |difference| per channel (R, G, B)"]
    for matrix, full in SETS:
        m = 0 if matrix == "bt601" else 1
        yuv = np.empty_like(rgb)
        L.check(l.ppn_rgb_to_yuv(m, int(full), rgb.ctypes.data, yuv.ctypes.data, len(rgb)), "ppn_rgb_to_yuv")
        k = (C.c_int32 * 6)()
        L.check(l.ppn_yuv_coefficients(m, int(full), k), "ppn_yuv_coefficients")
        cy, cvr, cvg, cug, cub, yoff = (int(v) for v in k)
        y = np.maximum(0, yuv[:, 0].astype(np.int64) - yoff) * cy + (1 << 19)
        uu, vv = yuv[:, 1].astype(np.int64) - 128, yuv[:, 2].astype(np.int64) - 128
        back = np.clip(np.stack([(y + cvr * vv) >> 20, (y + cvg * vv + cug * uu) >> 20, (y + cub * uu) >> 20], -1), 0, 255)
        err = np.abs(back - rgb.astype(np.int64))
        lines.append(f"  {matrix} {'full   ' if full else 'limited'}: max {err.max(0).tolist()}, mean "
                     f"{[round(float(v), 2) for v in err.mean(0)]}, grey -> {back[-1].tolist()}")
    return lines


def planted(frames, people, H, W, seed):
    """`people` skeletons per frame, every keypoint present, about 300 pixels tall, anywhere in the frame."""
    from pytorch_pose_proposal_network_amd import config as cfg
    rng = np.random.default_rng(seed)
    centre = np.stack([rng.uniform(0, H, (frames, people, 1)), rng.uniform(0, W, (frames, people, 1))], -1)
    mid = centre + rng.uniform(-150, 150, (frames, people, cfg.K, 2)) * np.array([1.0, 0.5])
    half = rng.uniform(4, 20, (frames, people, cfg.K, 2))
    half[:, :, 0] = rng.uniform(60, 160, (frames, people, 2))                     # the person's own box
    bbox = np.concatenate([mid - half, mid + half], -1).astype(np.float32)      # ymin, xmin, ymax, xmax
    return np.full(frames, people, np.int32), np.zeros((frames, people, cfg.K), np.int32), bbox


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_yuv.txt"))
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lines = round_trip_lines()
    F, H, W = a.frames, a.height, a.width
    if not torch.cuda.is_available():
        lines.append(f"surface drawing bench: {F} frames of {H}x{W}: not measured (no GPU in this run; "
                     "python tools/bench_render_yuv.py on an MI355X fills this part)")
    else:
        from pytorch_pose_proposal_network_amd import config as cfg, decode as D, render as R, rt
        dev = torch.device("cuda")
        lines.append(f"surface drawing bench: {F} frames of {H}x{W}, planted people with all {cfg.K} keypoints, median of "
                     f"{a.windows} windows of {a.calls} back-to-back calls (device events; the windows include the enqueue "
                     f"path), {a.warmup} warm-up calls per variant, {torch.cuda.get_device_name(0)}")
        for people in (12, 60):
            count, kp_cell, bbox = planted(F, people, H, W, people)
            res = D.DecodeResult(count=torch.from_numpy(count).to(dev), kp_cell=torch.from_numpy(kp_cell).to(dev),
                                 limb_arg=torch.zeros(F, people, len(cfg.EDGES), dtype=torch.int32, device=dev),
                                 bbox=torch.from_numpy(bbox).to(dev), score=torch.zeros(F, people, cfg.K, device=dev),
                                 max_humans=people)
            rend = R.Renderer(F, people)
            rgb = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev)
            variants = {"rgb in place": lambda: rend(rgb, res, out=rgb)}
            moved = {}
            lo, hi = rend(torch.zeros_like(rgb), res), rend(torch.full_like(rgb, 255), res)
            moved["rgb in place"] = int((lo == hi).sum())
            for fmt in ("nv12", "i420", "yuyv"):
                n = rt.yuv_frame_layout(fmt, (H, W))[0]
                raw = torch.randint(0, 256, (F, n), dtype=torch.uint8, device=dev)
                work, out = raw.clone(), torch.empty_like(raw)
                variants[f"{fmt} in place"] = lambda fmt=fmt, work=work: rend.draw_yuv(work, fmt, (H, W), res, out=work)
                variants[f"{fmt} out of place"] = lambda fmt=fmt, raw=raw, out=out: rend.draw_yuv(raw, fmt, (H, W), res, out=out)
                lo = rend.draw_yuv(torch.zeros_like(raw), fmt, (H, W), res)
                hi = rend.draw_yuv(torch.full_like(raw, 255), fmt, (H, W), res)
                moved[f"{fmt} in place"] = int((lo == hi).sum())
                moved[f"{fmt} out of place"] = 2 * F * n
            for fn in variants.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for _ in range(a.windows):
                for name, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.calls):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
            base = statistics.median(times["rgb in place"])
            lines.append(f"  {people} people per frame ({F * people * (cfg.K + len(cfg.EDGES))} primitives):")
            for name, ts in times.items():
                t = statistics.median(ts)
                what = "stored (painted samples)" if "in place" in name else "read + written"
                lines.append(f"    {name:18s}: {t:8.1f} us per call (windows {min(ts):.1f} .. {max(ts):.1f}) = {t / base:5.2f} x rgb "
                             f"in place; {moved[name] / 1e6:8.3f} MB {what}")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
