"""Time one validation epoch (main.py:1017-1172) both ways at the serving configuration: D-22, 384 x 384, batch 32, a
synthetic validation set of a few hundred `prng.u8_frames` images whose ground truth is planted from the network's own
decode (every second person, box centres slightly shifted, at most 64 per image).

    python tools/bench_validate.py [--out profiles/validate_bench.txt] [--images 256] [--batch 32] [--epochs 5]

  host route   what there was before validate.Validator: per batch an eval-mode forward, the decode (a persistent
               decode.Decoder, so that no allocation is charged to it), DecodeResult.to_humans() -- a blocking D2H plus one
               dict per person -- and evaluate.evaluation(pck_object) at the end of the epoch
  Validator    validate.Validator.step per batch (forward, decode, ppn_pckh_match; nothing read back) and finish() (one D2H,
               evaluate.metrics_from_records)
Both in one process on one GPU, warm, wall clock around whole epochs with a device synchronisation at either end, the
median of --epochs epochs; in bfloat16 and float32.  No loss in either route.  The file also says whether both routes
returned the same 8 AP values.  No threshold: the file is the record.  Without a GPU the file says "not measured"."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def planted_ground_truth(people, cap):
    """Per-image (gt_kps f32[G,17,2], gt_bboxes) from DecodeResult.to_host() dicts: every second person, at most `cap`."""
    gt_kps, gt_boxes = [], []
    for r in people:
        kps, boxes = [], []
        for p in range(0, min(int(r["n"]), 2 * cap), 2):
            bb = r["bbox"][p]
            kps.append(np.stack([(bb[1:, 1] + bb[1:, 3]) / 2 + 1.5, (bb[1:, 0] + bb[1:, 2]) / 2 - 1.0], 1).astype(np.float32))
            cy, cx = (bb[0, 0] + bb[0, 2]) / 2, (bb[0, 1] + bb[0, 3]) / 2
            boxes.append((np.float32(cx), np.float32(cy), np.float32(bb[0, 3] - bb[0, 1]), np.float32(bb[0, 2] - bb[0, 0])))
        gt_kps.append(np.stack(kps) if kps else np.zeros((0, 17, 2), np.float32))
        gt_boxes.append(boxes)
    return gt_kps, gt_boxes


def epochs(fn, n):
    fn()                                                  # warm: plans, workspaces, the caching allocator
    times, last = [], None
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_bench.txt"))
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--epochs", type=int, default=5)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not torch.cuda.is_available():
        text = (f"validate bench: {a.images} images, batch {a.batch}, {a.size}x{a.size}: not measured (no GPU in this run; "
                f"python tools/bench_validate.py on an MI355X fills this file)\n")
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    from pytorch_pose_proposal_network_amd import config as cfg, decode as D, drn, evaluate, model, prng, synth, validate as V

    B, S, g = a.batch, a.size, a.size // 16
    nb = max(1, a.images // B)
    N = nb * B
    sd = synth.make_state_dict("drn_d_22", 0)
    mean, std = (torch.tensor(v, device="cuda").view(1, 3, 1, 1) for v in (cfg.MEAN, cfg.STD))
    xs = [(torch.from_numpy(prng.u8_frames(100 + i, B, (S, S))).cuda().permute(0, 3, 1, 2).float() - mean).div_(std).contiguous()
          for i in range(nb)]                                      # rt_test.py:97-101
    index = [torch.arange(i * B, (i + 1) * B, dtype=torch.int32, device="cuda") for i in range(nb)]
    lines = [f"validate bench: drn_d_22, synthetic weights, {N} images of {S}x{S} in {nb} batches of {B}, wall clock per "
             f"epoch, median of {a.epochs} epochs after one warm epoch, {torch.cuda.get_device_name(0)}"]
    for dt in ("bfloat16", "float32"):
        net = model.PoseProposalNet(drn.drn_d_22(), insize=(S, S), outsize=(g, g), compute_dtype=dt).cuda()
        net.load_state_dict(sd)
        net.eval()
        dec = D.Decoder(B, (g, g), (S, S), net.local_grid_size)
        m = dec.out.max_humans
        people = [r for x in xs for r in dec(net(x)).to_host()]
        gt_kps, gt_boxes = planted_ground_truth(people, V.MAX_GT)
        gt = V.GroundTruth(gt_kps, gt_boxes)
        n_pred, n_gt = sum(int(r["n"]) for r in people), int(gt.counts.sum())

        def host_route():
            obj = [[] for _ in range(7)]
            for x in xs:
                for hm, sc in dec(net(x)).to_humans():
                    i = len(obj[0])
                    obj[0].append(i); obj[1].append(gt_kps[i]); obj[2].append(hm); obj[3].append(sc)
                    obj[4].append(gt_boxes[i]); obj[5].append(None); obj[6].append(None)
            return evaluate.evaluation(obj)

        val = V.Validator(net, gt, B, max_humans=m)

        t_finish = []

        def device_route():
            val.reset()
            for x, idx in zip(xs, index):
                val.step(x, idx)
            torch.cuda.synchronize()                      # only to time finish() on its own
            t0 = time.perf_counter()
            out = val.finish()[1]
            t_finish.append(time.perf_counter() - t0)
            return out

        def forward_only():
            for x in xs:
                net(x)

        print(f"{dt}: {n_pred} predicted people, {n_gt} planted ground-truth people; timing ...", flush=True)
        t_fwd, _ = epochs(forward_only, a.epochs)
        t_host, ap_host = epochs(host_route, a.epochs)
        print(f"{dt}: host route {t_host * 1e3:.1f} ms per epoch", flush=True)
        t_dev, ap_dev = epochs(device_route, a.epochs)
        same = np.array_equal(np.asarray(ap_host), np.asarray(ap_dev), equal_nan=True)
        lines += [
            f"{dt}: {n_pred} predicted people, {n_gt} planted ground-truth people, max_humans {m}",
            f"  forward alone                                                : {t_fwd * 1e3:9.2f} ms per epoch = "
            f"{N / t_fwd:8.0f} images/s",
            f"  host route (forward, decode, to_humans(), evaluation)        : {t_host * 1e3:9.2f} ms per epoch = "
            f"{N / t_host:8.0f} images/s",
            f"  Validator (forward, decode, ppn_pckh_match; finish: one D2H) : {t_dev * 1e3:9.2f} ms per epoch = "
            f"{N / t_dev:8.0f} images/s",
            f"    of which finish() (D2H of {val.records.score.numel() * 5 / 1e6:.1f} MB of records + the AP curve on the host)"
            f"{'':3}: {statistics.median(t_finish[1:]) * 1e3:9.2f} ms",
            f"  the 8 AP values of both routes are {'equal' if same else 'DIFFERENT'}: "
            f"{np.round(np.asarray(ap_dev, np.float64), 3).tolist()}" + ("" if same else
                                                                         f" vs {np.round(np.asarray(ap_host, np.float64), 3).tolist()}"),
        ]
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
