"""Time the device augmentation stage (augment.TrainAugmenter) at the training configuration: batch 32, 384 x 384, pmax 8.

    python tools/bench_augment.py [--out profiles/augment_bench.txt] [--calls 50] [--src-h 480 --src-w 640]

Device events around N calls after a warm-up (every shape warmed; one synchronise at the end of each window).  Writes, per
batch: us of the whole call, of the image launch, of the label launch and of the target encoder behind them, each launch
plain and with its option (the colour / noise image launch beside the plain one on the same matrices, the mirror label launch
beside the plain one) in the same run, alternated window by window, and their ratios; the bytes the image kernel must move (f32 planes written + every valid source byte read once) and their rate as a fraction of the chip's
~6.3 TB/s copy ceiling; the share of the training step (`train_shard.ms_per_step` of the newest
profiles/r*_bench.json).  No threshold: the file is the record.  Needs a GPU; there is no fallback."""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

COPY_CEILING = 6.3e12


def alternated(fns, calls, warmup, rounds=3):
    """us per call of each fn: `rounds` windows each, the fns taking turns, the smallest window of each (the box is shared)."""
    best = [float("inf")] * len(fns)
    for r in range(rounds):
        for i, fn in enumerate(fns):
            best[i] = min(best[i], timed(fn, calls, warmup if r == 0 else 2))
    return best


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


def train_step_ms():
    best = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench.json"))):
        with open(path) as f:
            d = json.load(f)
        if "train_shard" in d:
            best = (os.path.relpath(path, ROOT), float(d["train_shard"]["ms_per_step"]))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.txt"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--src-h", type=int, default=480)
    ap.add_argument("--src-w", type=int, default=640)
    ap.add_argument("--pmax", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_augment.py needs a GPU")
    from pytorch_pose_proposal_network_amd import augment as A, prng, synth, targets as T

    B, Hs, Ws, size = a.batch, a.src_h, a.src_w, 384
    src = torch.from_numpy(prng.u8_frames(99, B, (Hs, Ws))).cuda()
    # pictures of different valid sizes inside the common padding (3/4 .. 1 of it), as a real batch has
    frac = 0.75 + 0.25 * prng.uniform01(prng.stream_seed(99, 1), 2 * B).astype(np.float64).reshape(B, 2)
    hw = np.maximum((frac * [Hs, Ws]).astype(np.int32), 16)
    lists = [synth.synthetic_people(500 + b, insize=(int(w), int(h)), max_people=a.pmax) for b, (h, w) in enumerate(hw)]
    packed = tuple(torch.from_numpy(v).cuda() for v in T.pack_people(lists, pmax=a.pmax))
    hwd = torch.from_numpy(hw).cuda()
    aug = A.TrainAugmenter(insize=(size, size), seed=1, mode="train")
    step = [0]

    def whole():
        step[0] += 1
        aug(src, hw, packed, step[0])

    cj = A.ColorJitter()
    aug_opt = A.TrainAugmenter(insize=(size, size), seed=1, mode="train", mirror_p=0.5, color=cj)

    def whole_opt():
        step[0] += 1
        aug_opt(src, hw, packed, step[0])

    t_call, t_call_opt = alternated([whole, whole_opt], a.calls, a.warmup)
    # the launches alone, plain and with their option on the SAME matrices (those of the options' last step: about half the
    # images mirrored); colour rows: the sampler's (noise on in nearly every image), and the same rows with noise_q = 0
    p = aug_opt.params
    inv, fwd = torch.from_numpy(p["inv"]).cuda(), torch.from_numpy(p["fwd"]).cuda()
    rows = torch.from_numpy(p["color"]).cuda()
    quiet = p["color"].copy()
    quiet[:, 7] = 0
    rows_quiet = torch.from_numpy(quiet).cuda()
    flags = torch.from_numpy(p["mirror"].astype(np.int32)).cuda()
    x = torch.empty((B, 3, size, size), device="cuda")
    pout = tuple(torch.empty_like(v) for v in packed)
    t_img, t_img_col, t_img_quiet = alternated(
        [lambda: A.augment_images(src, hwd, inv, (size, size), out_f32=x),
         lambda: A.augment_images(src, hwd, inv, (size, size), out_f32=x, color=rows),
         lambda: A.augment_images(src, hwd, inv, (size, size), out_f32=x, color=rows_quiet)], a.calls, a.warmup)
    t_ppl, t_ppl_mir = alternated([lambda: A.augment_people(packed, fwd, (size, size), out=pout),
                                   lambda: A.augment_people(packed, fwd, (size, size), out=pout, mirror=flags)],
                                  a.calls, a.warmup)
    tg = T.encode_targets(pout, (size, size), (size // 16, size // 16))
    t_enc = timed(lambda: T.encode_targets(pout, (size, size), (size // 16, size // 16), out=tg), a.calls, a.warmup)
    # val mode reads every valid source pixel (train mode at s > 1 reads a part, at s < 1 writes mostly border)
    pv = A.sample_params(0, 0, hw, (size, size), "val")
    inv_v = torch.from_numpy(pv["inv"]).cuda()
    t_img_val, t_img_val_col = alternated(
        [lambda: A.augment_images(src, hwd, inv_v, (size, size), out_f32=x),
         lambda: A.augment_images(src, hwd, inv_v, (size, size), out_f32=x, color=rows)], a.calls, a.warmup)

    wr = B * 3 * size * size * 4
    rd = int((hw[:, 0].astype(np.int64) * hw[:, 1] * 3).sum())
    ref = train_step_ms()
    lines = [
        f"augment bench: batch {B}, sources u8 padded to {Hs}x{Ws} (valid {hw[:, 0].min()}..{hw[:, 0].max()} x "
        f"{hw[:, 1].min()}..{hw[:, 1].max()}), output {size}x{size} f32 NCHW, pmax {a.pmax}, "
        f"windows of {a.calls} calls after a warm-up of {a.warmup}, device events, {torch.cuda.get_device_name(0)}",
        "ONE run on a shared box.  Plain and optioned launches take turns window by window, three windows each, the smallest "
        "is reported.  Not profiled: no kernel trace, no counters, no run-to-run spread.",
        f"TrainAugmenter.__call__ (sampler on the host + 2 small uploads + image + label + target-encoder launches): "
        f"{t_call:9.1f} us per batch",
        f"TrainAugmenter.__call__ with mirror_p=0.5, color=ColorJitter() (same launches, one larger upload)          : "
        f"{t_call_opt:9.1f} us per batch  ({t_call_opt / t_call:.2f} x)",
        f"  ppn_augment_images        (train matrices, {int(p['mirror'].sum())} of {B} mirrored) : {t_img:9.1f} us per batch",
        f"  ppn_augment_images_color  (same matrices, sampled rows)      : {t_img_col:9.1f} us per batch  "
        f"(colour / plain = {t_img_col / t_img:.2f})",
        f"  ppn_augment_images_color  (same, noise_q = 0 in every row)   : {t_img_quiet:9.1f} us per batch  "
        f"(colour / plain = {t_img_quiet / t_img:.2f})",
        f"  ppn_augment_images        (val: plain resize)                : {t_img_val:9.1f} us per batch",
        f"  ppn_augment_images_color  (val matrices, sampled rows)       : {t_img_val_col:9.1f} us per batch  "
        f"(colour / plain = {t_img_val_col / t_img_val:.2f})",
        f"  ppn_augment_people                                            : {t_ppl:9.1f} us per batch",
        f"  ppn_augment_people_mirror (same matrices and flags)          : {t_ppl_mir:9.1f} us per batch  "
        f"(mirror / plain = {t_ppl_mir / t_ppl:.2f})",
        f"  ppn_encode_targets_c (existing, behind them)        : {t_enc:9.1f} us per batch",
        f"image kernel bytes: {wr / 1e6:.1f} MB written (f32 planes) + <= {rd / 1e6:.1f} MB read (every valid source byte "
        f"once) = {(wr + rd) / 1e6:.1f} MB",
        f"  train: {(wr + rd) / (t_img * 1e-6) / 1e12:.2f} TB/s = {(wr + rd) / (t_img * 1e-6) / COPY_CEILING:.2f} of the "
        f"~6.3 TB/s copy ceiling (upper bound on the bytes: a zoomed-in image reads part of its source); "
        f"written bytes alone {wr / (t_img * 1e-6) / 1e12:.2f} TB/s",
        f"  val  : {(wr + rd) / (t_img_val * 1e-6) / 1e12:.2f} TB/s = {(wr + rd) / (t_img_val * 1e-6) / COPY_CEILING:.2f} of "
        f"the copy ceiling",
        f"label kernel bytes: {sum(v.numel() * v.element_size() for v in packed) * 2 / 1e3:.1f} KB (latency-bound: one "
        f"workgroup per image)",
    ]
    if ref:
        lines.append(f"share of the training step ({ref[0]} train_shard.ms_per_step = {ref[1]:.3f} ms): whole call "
                     f"{t_call / (ref[1] * 1e3) * 100:.2f} %, image + label launches {(t_img + t_ppl) / (ref[1] * 1e3) * 100:.2f} %; "
                     f"with both options: whole call {t_call_opt / (ref[1] * 1e3) * 100:.2f} %, image + label launches "
                     f"{(t_img_col + t_ppl_mir) / (ref[1] * 1e3) * 100:.2f} %")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
