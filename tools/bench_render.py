"""Time the device drawing stage (render.draw_people / render.Renderer) at the serving configuration: batch 32, 384 x 384,
on the decode of planted crowds.

    python tools/bench_render.py [--out profiles/render_bench.txt] [--calls 50] [--batch 32]

Device events around N calls after a warm-up.  Writes: us per batch of the rasteriser in place and out of place (and of
its two launches' share of the primitives), the only route there was before it -- DecodeResult.to_humans() (a D2H of the
people lists) plus a PIL loop on the host, wall clock, frames read back included -- and the images/s of
rt.inference_batch with and without drawing.  No threshold: the file is the record.  Without a GPU the file says
"not measured"."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def host_route(frames_dev, result):
    """What a caller had to do before: people lists to the host, frames to the host, PIL per frame.  Returns seconds."""
    from PIL import Image, ImageDraw
    from pytorch_pose_proposal_network_amd import config as cfg
    colour = [cfg.COLOR_MAP[n] for n in cfg.KEYPOINT_NAMES]
    t0 = time.perf_counter()
    people = result.to_humans()
    frames = frames_dev.cpu().numpy()
    for img, (humans, _) in zip(frames, people):
        pil = Image.fromarray(img)
        pen = ImageDraw.Draw(pil)
        for hm in humans:
            mid = {k: ((b[1] + b[3]) / 2, (b[0] + b[2]) / 2) for k, b in hm.items()}
            for k, b in hm.items():
                if k == 0:
                    x0, y0, x1, y1 = int(b[1]), int(b[0]), int(b[3]), int(b[2])
                    if x1 - x0 >= 2 and y1 - y0 >= 2:
                        pen.rectangle([x0, y0, x1, y1], outline=colour[0])
                        pen.rectangle([x0 + 1, y0 + 1, x1 - 1, y1 - 1], outline=colour[0])
                else:
                    cx, cy = mid[k]
                    pen.ellipse((cx - 2, cy - 2, cx + 2, cy + 2), fill=colour[k])
            for s, t in cfg.EDGES:
                if s in mid and t in mid:
                    pen.line([*mid[s], *mid[t]], fill=colour[s], width=2)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.txt"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=384)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not torch.cuda.is_available():
        text = (f"render bench: batch {a.batch}, {a.size}x{a.size}: not measured (no GPU in this run; "
                f"python tools/bench_render.py on an MI355X fills this file)\n")
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    from pytorch_pose_proposal_network_amd import decode as D, prng, render as R, rt, synth

    B, S = a.batch, a.size
    g = S // 16
    heads = np.stack([synth.planted_crowd_head(7 + i, out_hw=(g, g)) for i in range(min(B, 4))])
    head = torch.from_numpy(heads).cuda().repeat((B + 3) // 4, 1, 1, 1)[:B].contiguous()
    res = D.decode_heads(head, insize_hw=(S, S))
    del head
    counts = res.count.cpu().numpy()
    kp = int((res.kp_cell.cpu().numpy()[:, :int(counts.max())] >= 0).sum())
    frames = torch.from_numpy(prng.u8_frames(3, B, (S, S))).cuda()
    rend = R.Renderer(B, res.max_humans)
    out = torch.empty_like(frames)
    scratch = frames.clone()
    t_out = timed(lambda: rend(frames, res, out=out), a.calls, a.warmup)
    t_in = timed(lambda: rend(scratch, res, out=scratch), a.calls, a.warmup)
    t_grid = timed(lambda: rend(frames, res, gridOn=True, out=out, outsize=(g, g)), a.calls, a.warmup)
    lines = [
        f"render bench: batch {B}, {S}x{S} u8 RGB, decode of planted crowds ({int(counts.sum())} people, {kp} keypoints in "
        f"the batch, max_humans {res.max_humans}), {a.calls} calls after {a.warmup} warm-up, device events, "
        f"{torch.cuda.get_device_name(0)}",
        f"  Renderer out of place (every pixel written)   : {t_out:9.1f} us per batch = {t_out / B:7.2f} us per image",
        f"  Renderer in place (drawn pixels only)         : {t_in:9.1f} us per batch = {t_in / B:7.2f} us per image",
        f"  Renderer out of place with the cell grid      : {t_grid:9.1f} us per batch",
        f"  frame bytes out of place: {2 * frames.numel() / 1e6:.1f} MB read + written = "
        f"{2 * frames.numel() / (t_out * 1e-6) / 1e12:.2f} TB/s",
    ]
    try:
        import PIL
        host = min(host_route(frames, res) for _ in range(3))
        lines.append(f"  before: to_humans() + frames D2H + Pillow {PIL.__version__} on the host (wall clock, best of 3): "
                     f"{host * 1e6:9.1f} us per batch = {host * 1e6 / B:7.2f} us per image")
    except ImportError:
        lines.append("  before: to_humans() + Pillow on the host: not measured (Pillow is not installed)")

    # the whole pipeline: forward + fused decode, with and without drawing (synthetic weights; one stream)
    model, _, _ = rt.network(image_size=S, state_dict=synth.make_state_dict("drn_d_22", 0), compute_dtype="bfloat16")
    dec = D.Decoder(B, (g, g), (S, S), model.local_grid_size)
    prend = R.Renderer(B, dec.out.max_humans)
    with torch.no_grad():
        t_plain = timed(lambda: rt.inference_batch(frames, model, dec), a.calls, a.warmup)
        t_drawn = timed(lambda: rt.inference_batch_drawn(frames, model, dec, prend, out=out), a.calls, a.warmup)
    lines += [
        f"pipeline (rt.inference_batch, drn_d_22 bf16, synthetic weights, one stream): {t_plain:9.1f} us per batch = "
        f"{B / (t_plain * 1e-6):8.0f} images/s",
        f"pipeline with drawing (rt.inference_batch_drawn, out of place)             : {t_drawn:9.1f} us per batch = "
        f"{B / (t_drawn * 1e-6):8.0f} images/s",
    ]
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
