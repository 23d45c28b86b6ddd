"""Time the monitoring overlay (render.Renderer with overlay=, over ppn_draw_scene / ppn_draw_scene_yuv) at 1080p.

    python tools/bench_overlay.py [--out profiles/overlay_bench.txt] [--parent-lib libppn_of_the_parent_commit.so]

tools/bench_render_yuv.py's method: each figure is the median over `windows` windows of `calls` back-to-back calls between
two device events, after a warm-up of every variant, the variants taking turns window by window; ONE run.  At this size a
call's two launches take a few tens of microseconds, so such a window also measures the enqueue path (ctypes, the argument
checks, two launches), not the kernels alone.

1. 8 frames of 1920 x 1080 with 12 tracked people each, 4 zones and 4 lines per stream, glyph scale 2, in place: the scene
   (ppn_draw_scene) beside the people alone (ppn_draw_humans) on the same frames, RGB and NV12.
2. The people-only calls on this build beside a build of the parent commit (`--parent-lib`, also taken from PPN_PARENT_LIB):
   the rasteriser's paint<V> now walks a second list, so ppn_draw_humans and ppn_draw_humans_yuv are timed through bare
   ctypes calls on both libraries loaded into this one process, each twice ("a" and "b"): the difference between two series
   of the same library is the run-to-run spread a difference between the builds has to be read against.  With PPN_LIB naming
   a library without ppn_draw_scene (a build of the parent commit) only these people-only series are timed, on that library.
3. rt.inference_batch_zones_drawn beside rt.inference_batch_zones (drn_d_22 bf16, synthetic weights, 8 frames of 384 x 384).
4. The host route there was before: TrackResult.to_host(), Zones.totals(), the people and zone results to the host and the
   NumPy restatement (tests/overlay_ref.py) as the host's drawing code, wall clock, on ONE 1080p frame (the restatement is
   test code, not an optimised drawing library; OpenCV would be faster and is not measured).
No threshold: the file is the record.  Without a GPU the file says "not measured"."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from bench_render_yuv import planted  # noqa: E402


def windows(variants, calls, n_windows, warmup):
    """{name: [us per call of each window]}, the variants taking turns window by window."""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(n_windows):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    return times


def report(lines, times, base=None):
    ref = statistics.median(times[base]) if base else None
    for name, ts in times.items():
        t = statistics.median(ts)
        rel = f" = {t / ref:5.2f} x {base}" if base and name != base else ""
        lines.append(f"    {name:34s}: {t:8.1f} us per call (windows {min(ts):.1f} .. {max(ts):.1f}){rel}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_bench.txt"))
    ap.add_argument("--parent-lib", default=os.environ.get("PPN_PARENT_LIB"))
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--people", type=int, default=12)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    F, H, W, P = a.frames, a.height, a.width, a.people
    if os.environ.get("PPN_LIB"):
        os.environ.setdefault("PPN_ALLOW_PARTIAL", "1")                  # a build of the parent commit: people-only series
    if not torch.cuda.is_available():
        text = (f"overlay bench: {F} frames of {H}x{W}: not measured (no GPU in this run; python tools/bench_overlay.py on an "
                "MI355X fills this file)\n")
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    import overlay_ref as O
    import render_cases as RC
    from pytorch_pose_proposal_network_amd import config as cfg, decode as D, lib as L, prng, render as R, rt, synth, track, zones
    dev = torch.device("cuda")
    lines = [f"overlay bench: {F} frames of {H}x{W}, {P} tracked people per frame, 4 zones and 4 lines per stream, scale 2, in "
             f"place; median of {a.windows} windows of {a.calls} back-to-back calls (device events; the windows include the "
             f"enqueue path), {a.warmup} warm-up calls per variant, one run, {torch.cuda.get_device_name(0)}"]

    count, kp_cell, bbox = planted(F, P, H, W, P)
    res = D.DecodeResult(count=torch.from_numpy(count).to(dev), kp_cell=torch.from_numpy(kp_cell).to(dev),
                         limb_arg=torch.zeros(F, P, len(cfg.EDGES), dtype=torch.int32, device=dev),
                         bbox=torch.from_numpy(bbox).to(dev), score=torch.zeros(F, P, cfg.K, device=dev), max_humans=P)
    ids = torch.arange(1, F * P + 1, dtype=torch.int32, device=dev).view(F, P)
    tracks = track.TrackResult(ids=ids, hits=torch.ones_like(ids), xy=None, live=torch.full((F,), P, dtype=torch.int32, device=dev),
                               count=res.count)
    rgb = torch.randint(0, 256, (F, H, W, 3), dtype=torch.uint8, device=dev)
    nv12 = torch.randint(0, 256, (F, rt.yuv_frame_layout("nv12", (H, W))[0]), dtype=torch.uint8, device=dev)

    # the people-only entry points through bare ctypes calls (part 2)
    def bare(lib):
        for name in ("ppn_draw_workspace_bytes", "ppn_draw_humans", "ppn_draw_humans_yuv"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = L._SIGNATURES[name]
        c = R.make_cfg()
        ws = torch.empty(lib.ppn_draw_workspace_bytes(C.byref(c), F, P) // 4, dtype=torch.int32, device=dev)
        _, pitch, pitch_c, u_off, _ = rt.yuv_frame_layout("nv12", (H, W))
        surf = L.YuvSurface(format=L.PPN_PIX_NV12, height=H, width=W, pitch=pitch, pitch_c=pitch_c, frame_stride=nv12.stride(0),
                            y=nv12.data_ptr(), u=nv12.data_ptr() + u_off, v=None, matrix=0, full_range=0)
        people = (res.count.data_ptr(), res.kp_cell.data_ptr(), res.bbox.data_ptr(), P, ws.data_ptr())
        keep = (c, ws, surf)

        def humans():
            assert lib.ppn_draw_humans(C.byref(c), rgb.data_ptr(), rgb.data_ptr(), F, H, W, *people, L.current_stream_ptr()) == 0, keep

        def humans_yuv():
            assert lib.ppn_draw_humans_yuv(C.byref(c), C.byref(surf), C.byref(surf), F, *people, L.current_stream_ptr()) == 0
        return humans, humans_yuv

    if not hasattr(L.load(), "ppn_draw_scene"):                         # PPN_LIB names a build from before the overlay
        fns = bare(L.load())
        times = windows({f"{what}, {os.path.basename(L.LIB_PATH)} {s}": fns[i] for i, what in enumerate(("ppn_draw_humans rgb", "ppn_draw_humans_yuv nv12"))
                         for s in "ab"}, a.calls, a.windows, a.warmup)
        lines.append("  the library has no ppn_draw_scene: people only, bare ctypes calls, two series each (a, b):")
        report(lines, times)
        text = "\n".join(lines) + "\n"
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    z = zones.Zones(F, 1, P)
    polys = [[(200 + 420 * i, 150), (560 + 420 * i, 180), (600 + 420 * i, 900), (180 + 420 * i, 940)] for i in range(4)]
    segs = [(100, 200 + 200 * i, 1800, 260 + 200 * i) for i in range(4)]
    for s in range(F):
        z.set_zones(s, polys)
        z.set_lines(s, segs)
    zr = z.update(res, tracks, smoothed=False)
    rend, ov = R.Renderer(F, P), R.Overlay(frames=1, scale=2)
    scene = dict(overlay=ov, tracks=tracks, zones=z, zone_result=zr)
    times = windows({
        "people, rgb (ppn_draw_humans)": lambda: rend(rgb, res, out=rgb),
        "scene, rgb (ppn_draw_scene)": lambda: rend(rgb, res, out=rgb, **scene),
        "people, nv12 (ppn_draw_humans_yuv)": lambda: rend.draw_yuv(nv12, "nv12", (H, W), res, out=nv12),
        "scene, nv12 (ppn_draw_scene_yuv)": lambda: rend.draw_yuv(nv12, "nv12", (H, W), res, out=nv12, **scene),
    }, a.calls, a.windows, a.warmup)
    lines.append("  1. the scene beside the people alone (render.Renderer):")
    report(lines, {k: times[k] for k in list(times)[:2]}, "people, rgb (ppn_draw_humans)")
    report(lines, {k: times[k] for k in list(times)[2:]}, "people, nv12 (ppn_draw_humans_yuv)")

    lines.append("  2. people only, bare ctypes calls, this build against the parent commit's (two series each: a, b):")
    if a.parent_lib and os.path.exists(a.parent_lib):
        builds = {"this build": bare(L.load()), "parent build": bare(C.CDLL(a.parent_lib))}
        for i, what in enumerate(("ppn_draw_humans rgb", "ppn_draw_humans_yuv nv12")):
            variants = {f"{what}, {b} {s}": fns[i] for s in "ab" for b, fns in builds.items()}
            times = windows(variants, a.calls, a.windows, a.warmup)
            report(lines, times)
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = max(abs(med[f"{what}, {b} a"] - med[f"{what}, {b} b"]) for b in builds)
            this, parent = (0.5 * (med[f"{what}, {b} a"] + med[f"{what}, {b} b"]) for b in builds)
            lines.append(f"      {what}: this build {this:.1f} us, parent build {parent:.1f} us: {this - parent:+.1f} us "
                         f"({(this / parent - 1) * 100:+.1f} %); spread between two series of one library: {spread:.1f} us")
    else:
        lines.append("    not measured: no library of the parent commit was given (--parent-lib)")

    # 3. the pipeline
    B, S = F, 384
    g = S // 16
    frames_u8 = torch.from_numpy(prng.u8_frames(3, B, (S, S))).cuda()
    model, _, _ = rt.network(image_size=S, state_dict=synth.make_state_dict("drn_d_22", 0), compute_dtype="bfloat16")
    dec = D.Decoder(B, (g, g), (S, S), model.local_grid_size)
    M = dec.out.max_humans
    tr, zn, rend2, ov2 = track.Tracker(B, 1, M), zones.Zones(B, 1, M), R.Renderer(B, M), R.Overlay(frames=1, scale=1)
    for s in range(B):
        zn.set_zones(s, [[(40 + 80 * i, 40), (110 + 80 * i, 40), (110 + 80 * i, 340), (40 + 80 * i, 340)] for i in range(4)])
        zn.set_lines(s, [(10, 60 + 80 * i, 370, 70 + 80 * i) for i in range(4)])
    out = torch.empty_like(frames_u8)
    with torch.no_grad():
        times = windows({
            "rt.inference_batch_zones": lambda: rt.inference_batch_zones(frames_u8, model, tr, zn, dec),
            "rt.inference_batch_zones_drawn": lambda: rt.inference_batch_zones_drawn(frames_u8, model, tr, zn, ov2, rend2, out, dec),
        }, max(a.calls // 4, 1), a.windows, a.warmup)
    lines.append(f"  3. pipeline (drn_d_22 bf16, synthetic weights, random frames, {B} x {S}x{S}, {M} people rows per image), per batch:")
    report(lines, times, "rt.inference_batch_zones")

    # 4. the host route, one frame
    _, pal, order, edges, _ = RC.fixture()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = tracks.to_host()
    _, line_total = z.totals()
    host = dict({n: t.cpu().numpy() for n, t in z.geom.items()}, out_zone=zr.zone.cpu().numpy(), out_line=zr.line.cpu().numpy(),
                line_total=line_total)
    c1, k1, b1, i1, frame = (t[:1].cpu().numpy() for t in (res.count, res.kp_cell, res.bbox, ids, rgb))
    t1 = time.perf_counter()
    one = dict(host, out_zone=host["out_zone"][:1], out_line=host["out_line"][:1])
    O.scene_ref(frame, c1, k1, b1, order, edges, pal,
                overlay=dict(frames=1, scale=2, tick=ov.tick, plates=True, colours=ov.colours), ids=i1, zones=one)
    t2 = time.perf_counter()
    lines.append(f"  4. host route, wall clock: results of {F} frames to the host (to_host, totals, people, zone results, one frame) "
                 f"{(t1 - t0) * 1e3:.2f} ms ({len(rows)} track rows); the NumPy restatement drawing ONE {H}x{W} frame "
                 f"{(t2 - t1) * 1e3:.0f} ms (test code, not an optimised drawing library)")
    lines.append("not profiled: no rocprofv3 kernel trace or counter run was taken; the times above are call times (launches "
                 "included), not kernel times")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
