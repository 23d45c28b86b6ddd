"""Time the redaction (redact.py; csrc/redact.hip ppn_redact_cells, ppn_redact_yuv): 8 frames of 1080p NV12 with 12 and with
60 planted people per frame, cell 16.

    python tools/bench_redact.py [--out profiles/redact_bench.txt] [--calls 200] [--rounds 6]

Device events around N back-to-back calls after a warm-up; the variants that are compared take turns, `rounds` windows each,
and the file gives the median (min .. max) over the windows.  Writes, per crowd:
  * ppn_redact_cells on its own (heads, and whole people);
  * ppn_redact_yuv in place beside ppn_draw_humans_yuv in place on the same frames and people;
  * ppn_redact_yuv out of place beside out.copy_(raw) of the same tensor (the kernel is a copy plus the masked cells);
and once rt.inference_redacted beside rt.inference_windows on the same batch.  No threshold: the file is the record.  These
are call times (launch and ctypes overhead included), not kernel times.  Without a GPU the file says "not measured"."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_render_yuv import planted  # noqa: E402
from bench_windows import fmt, in_turns  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redact_bench.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=384)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    Fr, S, (H, W), cell = a.frames, a.size, (1080, 1920), 16
    head = f"redact bench: {Fr} frames of {W}x{H} NV12, cell {cell}"
    if not torch.cuda.is_available():
        text = f"{head}: not measured (no GPU in this run; python tools/bench_redact.py on an MI355X fills this file)\n"
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    from pytorch_pose_proposal_network_amd import config as cfg, decode as D, redact, render, rt, synth, windows as Wn

    med = statistics.median
    nbytes = rt.yuv_frame_layout("nv12", (H, W))[0]
    gen = torch.Generator(device="cuda").manual_seed(1)
    raw = torch.randint(0, 256, (Fr, nbytes), dtype=torch.uint8, device="cuda", generator=gen)
    out, work = torch.empty_like(raw), raw.clone()
    lines = [f"{head}, {a.calls} back-to-back calls per window after a warm-up of {a.warmup}, {a.rounds} windows per variant "
             f"taking turns, device events, one process, {torch.cuda.get_device_name(0)}",
             "ONE run on a shared box; us per call: median (min .. max) over the windows.  Random bytes.  These are call times of "
             "back-to-back launches (launch and ctypes overhead included), not kernel times: launches this small measure the "
             "enqueue path as much as the kernel."]
    worst, floor = 0.0, [float("nan")] * 2
    for people in (12, 60):
        count, kp_cell, bbox = planted(Fr, people, H, W, people)
        res = D.DecodeResult(torch.from_numpy(count).cuda(), torch.from_numpy(kp_cell).cuda(),
                             torch.zeros(Fr, people, 1, dtype=torch.int32, device="cuda"), torch.from_numpy(bbox).cuda(),
                             torch.ones(Fr, people, cfg.K, device="cuda"), people)
        heads = redact.Redactor(1, Fr, people, (H, W), "nv12", cell=cell, hold=8)
        whole = redact.Redactor(1, Fr, people, (H, W), "nv12", cell=cell, hold=8, parts="person")
        rend = render.Renderer(Fr, people)
        t_h, t_w = in_turns([lambda: heads.cells(res), lambda: whole.cells(res)], a.calls, a.warmup, a.rounds)
        lines += [f"{people} people per frame ({cfg.K} keypoints each), hold 8, one stream of {Fr} frames:",
                  f"  ppn_redact_cells parts head  : {fmt(t_h)}",
                  f"  ppn_redact_cells parts person: {fmt(t_w)}"]
        for name, red in (("head", heads), ("person", whole)):
            bits = red.mask.cpu().numpy().view(np.uint32)
            share = sum(bin(int(v)).count("1") for v in bits.reshape(-1)) / (Fr * red.CH * red.CW)
            t_r, t_d = in_turns([lambda: red.apply(work, out=work), lambda: rend.draw_yuv(work, "nv12", (H, W), res, out=work)],
                                a.calls, a.warmup, a.rounds)
            t_o, t_c = in_turns([lambda: red.apply(raw, out=out), lambda: out.copy_(raw)], a.calls, a.warmup, a.rounds)
            ratio = med(t_o) / med(t_c)
            lines += [f"  parts {name}: {100 * share:.1f} % of the {red.CH} x {red.CW} cells masked",
                      f"    ppn_redact_yuv in place      : {fmt(t_r)}",
                      f"    ppn_draw_humans_yuv in place : {fmt(t_d)}   (same frames and people; ratio redact / draw {med(t_r) / med(t_d):.2f})",
                      f"    ppn_redact_yuv out of place  : {fmt(t_o)}",
                      f"    out.copy_(raw), {raw.numel() / 1e6:.1f} MB       : {fmt(t_c)}   (ratio redact / copy {ratio:.2f})"]
            if people == 12 and name == "head":                              # what the launch costs without and with every cell
                kept = red.mask.clone()
                extra = []
                for what, value in (("all zero", 0), ("all ones", -1)):
                    red.mask.fill_(value)
                    t_zi, t_zo = in_turns([lambda: red.apply(work, out=work), lambda: red.apply(raw, out=out)], a.calls, a.warmup, a.rounds)
                    extra.append(f"    mask {what}: in place {fmt(t_zi)}, out of place {fmt(t_zo)}")
                    if value == 0:
                        floor = [med(t_zi), med(t_zo)]
                red.mask.copy_(kept)
                lines += extra + ["    (all zero in place: every wave reads its mask bit and ends; all zero out of place: the copy path alone)"]
            worst = max(worst, ratio)
    if worst > 2:
        lines += [f"the out-of-place call takes up to {worst:.1f} times the copy of the same bytes.  What this run shows: with an all-zero "
                  f"mask the in-place call, whose waves read their mask bit and end, takes {floor[0]:.1f} us (the enqueue path and "
                  f"{Fr * heads.CH * heads.CW} one-cell waves), the out-of-place call on its copy path alone {floor[1]:.1f} us.  "
                  "Supposed, not traced: one wave moves one cell, a dword per lane (the 256 + 128 bytes of an NV12 cell in two "
                  "accesses, against 16 bytes per lane in a copy kernel), so the launch is bound by instructions and wave "
                  "launches, not by memory.  During development, replacing the integer division of every access by an f32 "
                  "multiply took a third off the call time; letting one wave take four cells of a row changed nothing."]

    # ---- beside the pipeline step (synthetic weights; one stream)
    model, _, _ = rt.network(image_size=S, state_dict=synth.make_state_dict("drn_d_22", 0), compute_dtype="bfloat16")
    tiles = Wn.WindowLayout.tiles((H, W), 2, 2)
    B, g = Fr * tiles.n, S // 16
    dec = D.Decoder(B, (g, g), (S, S), model.local_grid_size)
    merger = Wn.WindowMerger(tiles, Fr, (S, S), dec.out.max_humans)
    pipe = redact.Redactor(1, Fr, merger.max_out, (H, W), "nv12", cell=cell, hold=8)
    with torch.no_grad():
        def windowed():
            return rt.inference_windows(raw, "nv12", (H, W), model, tiles, dec, merger, size=S)

        def redacted():
            return rt.inference_redacted(raw, "nv12", (H, W), model, pipe, tiles, decoder=dec, merger=merger, size=S, out=out)

        t_i, t_x = in_turns([windowed, redacted], a.calls, a.warmup, a.rounds)
    bits = pipe.mask.cpu().numpy().view(np.uint32)
    share = sum(bin(int(v)).count("1") for v in bits.reshape(-1)) / (Fr * pipe.CH * pipe.CW)
    lines += [f"pipeline (drn_d_22 bf16, synthetic weights, random frames, 2 x 2 layout, fused decode, one stream), batch {B}, "
              f"redaction out of place:",
              f"  rt.inference_windows  of {Fr} frames: {fmt(t_i)} = {Fr / (med(t_i) * 1e-6):7.0f} frames/s",
              f"  rt.inference_redacted of {Fr} frames: {fmt(t_x)} = {Fr / (med(t_x) * 1e-6):7.0f} frames/s "
              f"({100 * share:.1f} % of the cells masked)",
              f"  ratio of the medians redacted / windows: {med(t_x) / med(t_i):.3f}",
              "not profiled: no rocprofv3 kernel trace or counter run of redact_cells_kernel or redact_kernel was taken, so no "
              "bandwidth fraction is claimed"]
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
