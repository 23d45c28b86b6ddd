"""Time the action model (actions.ActionModel; csrc/stgcn.hip ppn_stgcn_input / gcn / tcn / head, and its float16 mode,
csrc/stgcn16.hip ppn_stgcn16_*).

    python tools/bench_actions.py [--out profiles/actions_bench.txt] [--calls 200] [--warmup 20]

Device events around N back-to-back calls after a warm-up (tools/bench_track.py's `timed`).  Writes:
  * the "paper" network at T = 32 with 64 active clips (one stream, every slot live) and with 2048 (32 streams), beside the
    same function through torch-ROCm's own convolutions and einsum in f32 (tests/stgcn_ref.py on the device) in the same run,
    and the achieved FLOP/s as a fraction of the 157 TFLOP/s f32 MFMA peak;
  * the launches of the 2048-clip call one by one;
  * rt.inference_batch_actions beside rt.inference_batch_clips on the same frames;
  * the float16 model beside the f32 one in the SAME run and process, the two modes alternating (f32, f16, f32, f16, the
    lower time of each kept): 64 and 2048 active clips, the fraction of the 2.5 PFLOP/s f16 MFMA peak, the ratio f32 / f16,
    max |logit difference| between the modes, the launch-by-launch table and the pipeline line with a float16 model.
No threshold: the file is the record.  Without a GPU the file says "not measured"."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))
sys.path.insert(2, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_track import timed  # noqa: E402

PEAK = 157.3e12
PEAK16 = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actions_bench.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--length", type=int, default=32)
    ap.add_argument("--classes", type=int, default=60)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--no-pipeline", action="store_true", help="skip the rt.inference_batch_* comparison")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    T = a.length
    head = f"actions bench: ST-GCN 'paper' (ten blocks, {a.classes} classes), T = {T}, K = 18, exact f32"
    if not torch.cuda.is_available():
        text = (f"{head}: not measured (no GPU in this run; python tools/bench_actions.py on an MI355X fills this file)\n"
                "float16 mode beside the f32 mode: not measured\n")
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    import stgcn_ref as R
    from pytorch_pose_proposal_network_amd import actions as AC, clips, decode as D, prng, rt, synth, track

    spec = AC.stgcn_spec("paper", a.classes)
    sd = AC.random_state_dict(spec, 1)
    A = torch.from_numpy(AC.skeleton_graph()).cuda()
    sd_dev = {k: v.cuda() for k, v in sd.items()}
    flops = spec.flops(T)
    lines = [f"{head}; {flops / 1e9:.3f} GFLOP per clip (aggregation, both convolutions, shortcuts, classifier); {a.calls} "
             f"back-to-back calls after a warm-up of {a.warmup}, device events, one process, {torch.cuda.get_device_name(0)}",
             "ONE run on a shared box.  Call times of back-to-back launches (launch and ctypes overhead included), not kernel "
             "times; no kernel trace or counter run was taken.  Random weights: nothing here says anything about accuracy.",
             f"peak for the fraction: {PEAK / 1e12:.1f} TFLOP/s (f32 MFMA, MI355X)"]
    lines16 = ["float16 mode (compute_dtype=\"float16\", csrc/stgcn16.hip: half storage, v_mfma_f32_16x16x32_f16, f32 accumulation) "
               "beside the f32 mode, SAME run and process, the modes alternating (f32, f16, f32, f16; the lower call time of "
               "each); call times of back-to-back launches, not kernel times",
               f"peak for the float16 fraction: {PEAK16 / 1e12:.0f} TFLOP/s (f16 MFMA dense, MI355X)"]
    gen = torch.Generator(device="cuda").manual_seed(2)
    models, models16 = {}, {}
    for S in (1, 32):
        n = S * 64
        m = models[S] = AC.ActionModel(spec, sd, S, T)
        x = (torch.rand(S, 64, 3, T, 18, device="cuda", generator=gen) - 0.5)
        ids = torch.arange(1, n + 1, dtype=torch.int32, device="cuda").view(S, 64)
        length = torch.full((S, 64), T, dtype=torch.int32, device="cuda")
        batch = clips.ClipBatch(x, ids, length)
        t_mine = timed(lambda: m(batch), a.calls, a.warmup)
        assert int(m.n_active) == n
        h = models16[S] = AC.ActionModel(spec, sd, S, T, compute_dtype="float16")
        t32, t16 = [], []
        for _ in range(2):
            t32.append(timed(lambda: m(batch), a.calls, a.warmup))
            t16.append(timed(lambda: h(batch), a.calls, a.warmup))
        t32, t16 = min(t32), min(t16)
        assert int(h.n_active) == n
        d16 = float((h.logits - m.logits).abs().max())
        same = float((h.label == m.label).float().mean())
        lines16.append(f"{n:5d} active clips ({S} streams): float16 {t16:10.1f} us per call = {t16 / n:8.2f} us per clip, "
                       f"{n * flops / (t16 * 1e-6) / 1e12:6.2f} TFLOP/s = {100 * n * flops / (t16 * 1e-6) / PEAK16:5.1f} % of the f16 "
                       f"peak; f32 in the same alternation {t32:10.1f} us; ratio f32 / f16 {t32 / t16:5.2f}; max |logit difference| "
                       f"between the modes {d16:.2e} at max |logit| {float(m.logits.abs().max()):.2f}, equal labels {100 * same:.1f} %")
        flat = x.view(n, 3, T, 18)
        with torch.no_grad():
            t_torch = timed(lambda: R.forward(spec, sd_dev, A, flat, torch.float32), a.calls, a.warmup)
            diff = float((R.forward(spec, sd_dev, A, flat, torch.float32) - m.logits.view(n, -1)).abs().max())
        lines.append(f"{n:5d} active clips ({S} streams): ActionModel {t_mine:10.1f} us per call = {t_mine / n:8.2f} us per clip, "
                     f"{n * flops / (t_mine * 1e-6) / 1e12:6.2f} TFLOP/s = {100 * n * flops / (t_mine * 1e-6) / PEAK:5.1f} % of peak; "
                     f"torch-ROCm f32 (conv2d, batch_norm, einsum) {t_torch:10.1f} us per call = "
                     f"{n * flops / (t_torch * 1e-6) / 1e12:6.2f} TFLOP/s; ratio torch / ActionModel {t_torch / t_mine:5.2f}; "
                     f"max |logit difference| {diff:.2e}")
    # the launches of the 2048-clip call one by one (the buffers hold the last call's values)
    m = models[32]
    calls = max(a.calls // 4, 10)
    lines.append(f"launch by launch at 2048 active clips ({calls} calls each, {a.warmup} warm-up): us per launch, TFLOP/s of the "
                 "launch's own multiply-adds")
    cur = m.x0
    for i, (d, w) in enumerate(zip(m.descs, m.blocks)):
        out = m.y[i % len(m.y)]
        cin, cout, s, res = spec.blocks[i]
        t, to = m.lengths[i], m.lengths[i + 1]
        tg = timed(lambda: AC.launch_gcn(d, w, cur, m.n_active, m.capacity, m.u), calls, a.warmup)
        tt = timed(lambda: AC.launch_tcn(d, w, m.u, cur, m.n_active, m.capacity, out), calls, a.warmup)
        fg = 2048 * 2 * t * 18 * (3 * cin * 18 + 3 * cin * cout)
        ft = 2048 * 2 * to * 18 * (9 * cout * cout + (cin * cout if res == "proj" else 0))
        lines.append(f"  block {i} ({cin:3d} -> {cout:3d}, stride {s}, {res:8s}, T {t:2d} -> {to:2d}): gcn {tg:9.1f} us "
                     f"{fg / (tg * 1e-6) / 1e12:6.2f} TFLOP/s; tcn {tt:9.1f} us {ft / (tt * 1e-6) / 1e12:6.2f} TFLOP/s")
        cur = out
    h = models16[32]
    lines16.append(f"float16 launch by launch at 2048 active clips ({calls} calls each, {a.warmup} warm-up): us per launch, TFLOP/s "
                   "of the launch's own multiply-adds")
    cur = h.x0
    for i, (d, w) in enumerate(zip(h.descs, h.blocks)):
        out = h.y[i % len(h.y)]
        cin, cout, s, res = spec.blocks[i]
        t, to = h.lengths[i], h.lengths[i + 1]
        tg = timed(lambda: AC.launch_gcn(d, w, cur, h.n_active, h.capacity, h.u), calls, a.warmup)
        tt = timed(lambda: AC.launch_tcn(d, w, h.u, cur, h.n_active, h.capacity, out), calls, a.warmup)
        fg = 2048 * 2 * t * 18 * (3 * cin * 18 + 3 * cin * cout)
        ft = 2048 * 2 * to * 18 * (9 * cout * cout + (cin * cout if res == "proj" else 0))
        lines16.append(f"  block {i} ({cin:3d} -> {cout:3d}, stride {s}, {res:8s}, T {t:2d} -> {to:2d}): gcn {tg:9.1f} us "
                       f"{fg / (tg * 1e-6) / 1e12:6.2f} TFLOP/s; tcn {tt:9.1f} us {ft / (tt * 1e-6) / 1e12:6.2f} TFLOP/s")
        cur = out
    if not a.no_pipeline:
        B, S = a.batch, a.size
        g = S // 16
        frames_u8 = torch.from_numpy(prng.u8_frames(3, B, (S, S))).cuda()
        model, _, _ = rt.network(image_size=S, state_dict=synth.make_state_dict("drn_d_22", 0), compute_dtype="bfloat16")
        dec = D.Decoder(B, (g, g), (S, S), model.local_grid_size)
        with torch.no_grad():
            tr = track.Tracker(B, 1, dec.out.max_humans)
            pc = clips.PoseClips(B, 1, dec.out.max_humans, length=T)
            am = AC.ActionModel(spec, sd, B, T, min_len=1)
            t0 = timed(lambda: rt.inference_batch_clips(frames_u8, model, tr, pc, dec), a.calls, a.warmup)
            t1 = timed(lambda: rt.inference_batch_actions(frames_u8, model, tr, pc, am, dec), a.calls, a.warmup)
            lines.append(f"pipeline (drn_d_22 bf16, synthetic weights, random frames, {B} streams of one {S}x{S} frame, min_len 1): "
                         f"rt.inference_batch_clips {t0:9.1f} us per batch = {B / (t0 * 1e-6):8.0f} images/s; "
                         f"rt.inference_batch_actions {t1:9.1f} us = {B / (t1 * 1e-6):8.0f} images/s with {int(am.n_active)} "
                         f"active clips at the last call")
            am16 = AC.ActionModel(spec, sd, B, T, min_len=1, compute_dtype="float16")
            t2 = timed(lambda: rt.inference_batch_actions(frames_u8, model, tr, pc, am16, dec), a.calls, a.warmup)
            lines16.append(f"pipeline with a float16 model (the same frames, tracker and clips): rt.inference_batch_actions {t2:9.1f} "
                           f"us = {B / (t2 * 1e-6):8.0f} images/s with {int(am16.n_active)} active clips at the last call")
    text = "\n".join(lines + lines16) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
