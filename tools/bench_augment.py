"""Time the device augmentation stage (augment.TrainAugmenter) at the training configuration: batch 32, 384 x 384, pmax 8.

    python tools/bench_augment.py [--out profiles/augment_bench.txt] [--calls 50] [--src-h 480 --src-w 640]

Device events around N calls after a warm-up (every shape warmed; one synchronise at the end of each window).  Writes, per
batch: us of the whole call, of the image launch, of the label launch and of the target encoder behind them; the bytes the
image kernel must move (f32 planes written + every valid source byte read once) and their rate as a fraction of the chip's
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

    t_call = timed(whole, a.calls, a.warmup)
    p = aug.params
    inv, fwd = torch.from_numpy(p["inv"]).cuda(), torch.from_numpy(p["fwd"]).cuda()
    x = torch.empty((B, 3, size, size), device="cuda")
    pout = tuple(torch.empty_like(v) for v in packed)
    t_img = timed(lambda: A.augment_images(src, hwd, inv, (size, size), out_f32=x), a.calls, a.warmup)
    t_ppl = timed(lambda: A.augment_people(packed, fwd, (size, size), out=pout), a.calls, a.warmup)
    tg = T.encode_targets(pout, (size, size), (size // 16, size // 16))
    t_enc = timed(lambda: T.encode_targets(pout, (size, size), (size // 16, size // 16), out=tg), a.calls, a.warmup)
    # val mode reads every valid source pixel (train mode at s > 1 reads a part, at s < 1 writes mostly border)
    pv = A.sample_params(0, 0, hw, (size, size), "val")
    inv_v = torch.from_numpy(pv["inv"]).cuda()
    t_img_val = timed(lambda: A.augment_images(src, hwd, inv_v, (size, size), out_f32=x), a.calls, a.warmup)

    wr = B * 3 * size * size * 4
    rd = int((hw[:, 0].astype(np.int64) * hw[:, 1] * 3).sum())
    ref = train_step_ms()
    lines = [
        f"augment bench: batch {B}, sources u8 padded to {Hs}x{Ws} (valid {hw[:, 0].min()}..{hw[:, 0].max()} x "
        f"{hw[:, 1].min()}..{hw[:, 1].max()}), output {size}x{size} f32 NCHW, pmax {a.pmax}, "
        f"{a.calls} calls after {a.warmup} warm-up, device events, {torch.cuda.get_device_name(0)}",
        f"TrainAugmenter.__call__ (sampler on the host + 2 small uploads + image + label + target-encoder launches): "
        f"{t_call:9.1f} us per batch",
        f"  ppn_augment_images  (train params of the last step): {t_img:9.1f} us per batch",
        f"  ppn_augment_images  (val: plain resize)            : {t_img_val:9.1f} us per batch",
        f"  ppn_augment_people                                  : {t_ppl:9.1f} us per batch",
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
                     f"{t_call / (ref[1] * 1e3) * 100:.2f} %, the two new launches {(t_img + t_ppl) / (ref[1] * 1e3) * 100:.2f} %")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
