"""Time the person crops (crops.py; csrc/crops.hip ppn_people_rois, csrc/ingest.hip ppn_ingest_rois): 8 frames of 1080p NV12
with 16 people each = 128 crops of 256 x 128.

    python tools/bench_crops.py [--out profiles/crops_bench.txt] [--calls 200] [--rounds 6]

Device events around N back-to-back calls after a warm-up; two variants that are compared take turns, `rounds` windows each,
and the file gives the median (min .. max) over the windows.  Writes:
  * the ROI ingest launch beside ppn_ingest_windows with the same 16 rectangles as a static layout (every frame holds the
    same 16 people, so both write the same output pixels through the same body; the table in device memory, its
    validation and the two double divides per work item are the difference), the ratio of the medians and, beside it, the
    run-to-run spread of the windows launch itself;
  * ppn_people_rois on its own;
  * rt.inference_crops beside rt.inference_windows on the same frames.
No threshold: the file is the record.  Without a GPU the file says "not measured"."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_windows import fmt, in_turns  # noqa: E402


def planted_people(frames, src_hw, M, K, people, seed):
    """A DecodeResult's arrays in frame pixels: the same `people` people in every frame, well inside the picture."""
    rng = np.random.default_rng(seed)
    H, W = src_hw
    count = np.full(frames, people, np.int32)
    kp = np.full((frames, M, K), -1, np.int32)
    bb = np.zeros((frames, M, K, 4), np.float32)
    sc = np.zeros((frames, M, K), np.float32)
    for p in range(people):
        h, w = rng.uniform(250, 520), rng.uniform(90, 220)
        y, x = rng.uniform(60, H - 60 - h), rng.uniform(140, W - 140 - w)
        for k in range(K):
            ky, kx = (y + h / 2, x + w / 2) if k == 0 else (rng.uniform(y, y + h), rng.uniform(x, x + w))
            kp[:, p, k], sc[:, p, k] = 1, rng.random()
            bb[:, p, k] = (ky - 20, kx - 20, ky + 20, kx + 20) if k else (y + h * 0.3, x + w * 0.2, y + h * 0.7, x + w * 0.8)
    return count, kp, bb, sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crops_bench.txt"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--people", type=int, default=16)
    ap.add_argument("--size", type=int, default=384)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    Fr, P, S, (H, W), out_hw = a.frames, a.people, a.size, (1080, 1920), (256, 128)
    head = f"crops bench: {Fr} frames of {W}x{H} NV12, {P} people each, {Fr * P} crops of {out_hw[1]}x{out_hw[0]}"
    if not torch.cuda.is_available():
        text = f"{head}: not measured (no GPU in this run; python tools/bench_crops.py on an MI355X fills this file)\n"
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    from pytorch_pose_proposal_network_amd import crops as Cr, decode as D, rt, synth, windows as Wn

    nbytes = rt.yuv_frame_layout("nv12", (H, W))[0]
    gen = torch.Generator(device="cuda").manual_seed(1)
    raw = torch.randint(0, 256, (Fr, nbytes), dtype=torch.uint8, device="cuda", generator=gen)
    lines = [f"{head}, {a.calls} back-to-back calls per window after a warm-up of {a.warmup}, {a.rounds} windows per variant "
             f"taking turns, device events, one process, {torch.cuda.get_device_name(0)}",
             "ONE run on a shared box; us per call: median (min .. max) over the windows.  Random bytes.  These are call times of "
             "back-to-back launches (launch and ctypes overhead included), not kernel times."]

    # ---- the rectangles: ppn_people_rois on its own
    M, K = 576, 18
    count, kp, bb, sc = planted_people(Fr, (H, W), M, K, P, 7)
    res = D.DecodeResult(torch.from_numpy(count).cuda(), torch.from_numpy(kp).cuda(),
                         torch.zeros(Fr, M, 1, dtype=torch.int32, device="cuda"), torch.from_numpy(bb).cuda(),
                         torch.from_numpy(sc).cuda(), M)
    cropper = Cr.PersonCropper(Fr, M, (H, W), "nv12", out_hw, max_crops=P)
    root = Cr.PersonCropper(Fr, M, (H, W), "nv12", out_hw, max_crops=P, mode="root")
    t_p, t_r = in_turns([lambda: cropper.rois(res), lambda: root.rois(res)], a.calls, a.warmup, a.rounds)
    roi, status = cropper.roi.cpu().numpy(), cropper.status.cpu().numpy()
    assert (status == 0).all() and (roi == roi[0]).all(), "the planted people must all give a crop, the same in every frame"
    lines += [f"rectangles of {Fr} x {P} slots, max_humans {M}, K {K} (rectangles {int(roi[..., 2].min())}..{int(roi[..., 2].max())} rows "
              f"x {int(roi[..., 3].min())}..{int(roi[..., 3].max())} columns):",
              f"  ppn_people_rois mode people (union of {K} keypoint boxes): {fmt(t_p)}",
              f"  ppn_people_rois mode root                              : {fmt(t_r)}"]

    # ---- the ingest launch: the table in device memory beside the same rectangles as a static layout
    lay = Wn.WindowLayout((H, W), [tuple(int(v) for v in r) for r in roi[0]])
    out_w = torch.empty(Fr * P, out_hw[0], out_hw[1], 3, dtype=torch.uint8, device="cuda")
    t_roi, t_win = in_turns([lambda: cropper.crop(raw), lambda: Wn.ingest_windows(raw, "nv12", lay, out_hw, out_w)],
                            a.calls, a.warmup, a.rounds)
    assert torch.equal(cropper.crops.view(-1), out_w.view(-1)), "both launches must write the same bytes"
    ratio = statistics.median(t_roi) / statistics.median(t_win)
    spread = (max(t_win) - min(t_win)) / statistics.median(t_win)
    lines += [f"ingest, {Fr * P} images of {out_hw[1]}x{out_hw[0]} out ({out_w.numel() / 1e6:.1f} MB written, the same bytes from both):",
              f"  ppn_ingest_rois     {Fr} frames x {P} ROIs from the device table: {fmt(t_roi)}",
              f"  ppn_ingest_windows  {Fr} frames x {P} windows, the same rectangles : {fmt(t_win)}",
              f"  ratio of the medians ROI / windows: {ratio:.3f}; run-to-run spread of the windows launch (max - min) / median: "
              f"{spread:.3f}; spread of the ROI launch: {(max(t_roi) - min(t_roi)) / statistics.median(t_roi):.3f}",
              "  " + ("the ratio lies inside that spread: this run does not resolve a cost of the device-side table"
                      if abs(ratio - 1) <= spread else
                      f"the ratio lies outside that spread: the device-side table (a 16-byte table load and the rectangle's checks per "
                      f"workgroup, two f64 divides per work item where the host passed the scales) costs "
                      f"{statistics.median(t_roi) - statistics.median(t_win):+.1f} us per call in this run")]

    # ---- beside the pipeline step (synthetic weights; one stream)
    model, _, _ = rt.network(image_size=S, state_dict=synth.make_state_dict("drn_d_22", 0), compute_dtype="bfloat16")
    tiles = Wn.WindowLayout.tiles((H, W), 2, 2)
    B, g = Fr * tiles.n, S // 16
    dec = D.Decoder(B, (g, g), (S, S), model.local_grid_size)
    merger = Wn.WindowMerger(tiles, Fr, (S, S), dec.out.max_humans)
    pipe = Cr.PersonCropper(Fr, merger.max_out, (H, W), "nv12", out_hw, max_crops=P)
    with torch.no_grad():
        def windowed():
            return rt.inference_windows(raw, "nv12", (H, W), model, tiles, dec, merger, size=S)

        def cropped():
            return rt.inference_crops(raw, "nv12", (H, W), model, pipe, tiles, decoder=dec, merger=merger, size=S)

        t_i, t_c = in_turns([windowed, cropped], a.calls, a.warmup, a.rounds)
        st = cropped()[1].status.cpu().numpy()
    lines += [f"pipeline (drn_d_22 bf16, synthetic weights, random frames, 2 x 2 layout, fused decode, one stream), batch {B}:",
              f"  rt.inference_windows of {Fr} frames: {fmt(t_i)} = {Fr / (statistics.median(t_i) * 1e-6):7.0f} frames/s",
              f"  rt.inference_crops   of {Fr} frames: {fmt(t_c)} = {Fr / (statistics.median(t_c) * 1e-6):7.0f} frames/s "
              f"({int((st == 0).sum())} of {st.size} slots give a crop)",
              f"  ratio of the medians crops / windows: {statistics.median(t_c) / statistics.median(t_i):.3f}",
              "not profiled: no rocprofv3 kernel trace or counter run of ingest_rois_kernel or people_rois_kernel was taken"]
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
