"""Time flip-averaged inference (tta.FlipMerger, rt.inference_batch(flip_tta=True)) at the serving geometry: 24 x 24 cells,
21 x 21 limb windows.

    python tools/bench_tta.py [--out profiles/tta_merge.txt] [--calls 50]

Device events around N calls after a warm-up, everything in one process.  Writes: us per call and achieved bytes/s of
ppn_tta_merge at batch 32 and batch 1, with and without the merged head, for the host's own launch geometry and for
forced window splits (PPN_TTA_SPLIT); ppn_limb_argmax -- the existing kernel with the same access pattern -- on one of the
same heads; images/s of rt.inference_batch with and without flip_tta (bf16, synthetic weights); and, for information, how
many of the reference's people on tests/golden/e2e_tuned_d22_384.npz each route reproduces.  No threshold: the file is the
record.  Without a GPU the file says "not measured"."""
import argparse
import os
import sys

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


def merge_rows(B, calls, warmup, splits):
    from pytorch_pose_proposal_network_amd import decode as D, tta
    mg = tta.FlipMerger(B)
    c = mg.cfg
    ncell, C = c.H * c.W, mg.channels
    pair = torch.rand(2 * B, C, c.H, c.W, device="cuda")
    read = 2 * B * C * ncell * 4
    small = B * 6 * c.K * ncell * 4 + B * c.E * ncell * 8
    rows, rate = [], {}
    for split in splits:
        if split is None:
            os.environ.pop("PPN_TTA_SPLIT", None)
        else:
            os.environ["PPN_TTA_SPLIT"] = str(split)
        for want_head in (False, True):
            t = timed(lambda: mg.merge(pair, want_head=want_head), calls, warmup)
            nbytes = read + small + (B * C * ncell * 4 if want_head else 0)
            rate[(split, want_head)] = nbytes / (t * 1e-6)
            rows.append(f"  batch {B:2d}, {'host choice' if split is None else f'split {split:3d}  '}, "
                        f"{'unary + keys + head' if want_head else 'unary + keys       '}: {t:9.1f} us per call, "
                        f"{nbytes / 1e6:8.1f} MB moved = {nbytes / (t * 1e-6) / 1e12:5.2f} TB/s")
    os.environ.pop("PPN_TTA_SPLIT", None)
    dec = D.Decoder(B)
    head = pair[:B]
    t = timed(lambda: dec.limb_argmax(head), calls, warmup)
    nbytes = B * c.E * c.sH * c.sW * ncell * 4 + B * c.E * ncell * 4
    rows.append(f"  batch {B:2d}, ppn_limb_argmax on the first of the two heads (limb block read once): {t:9.1f} us per call, "
                f"{nbytes / 1e6:8.1f} MB moved = {nbytes / (t * 1e-6) / 1e12:5.2f} TB/s")
    rows.append(f"  batch {B:2d}, achieved bytes/s of the merge (host choice, unary + keys) over ppn_limb_argmax's in this run: "
                f"{rate[(None, False)] / (nbytes / (t * 1e-6)):5.2f}")
    return rows


def agreement_rows():
    """The reference's own people on the tuned checkpoint against this pipeline's, with and without the flag."""
    from pytorch_pose_proposal_network_amd import decode as D, drn, model, prng, rt, synth
    g = np.load(os.path.join(ROOT, "tests", "golden", "e2e_tuned_d22_384.npz"))
    arch, size, batch = str(g["arch"]), int(g["size"]), int(g["batch"])
    st = np.load(os.path.join(ROOT, "pytorch_pose_proposal_network_amd", "data", f"bn_calib_{arch}_seed0.npz"))
    sd = synth.make_state_dict(arch, int(g["seed_w"]), bn_stats={k: st[k] for k in st.files})
    for k in g.files:
        if k.startswith("override/"):
            sd[k[len("override/"):]] = g[k]
    net = model.PoseProposalNet(getattr(drn, arch)(), insize=(size, size), outsize=(size // 16, size // 16),
                                compute_dtype="float32").cuda()
    net.load_state_dict(sd)
    net.eval()
    frames = torch.from_numpy(prng.u8_frames(int(g["seed_in"]), batch, (size, size))).cuda()
    exp = [{k: g[f"{i}/{k}"] for k in ("n", "root_cell", "kp_cell", "limb_arg", "bbox", "score")} for i in range(batch)]
    rows = []
    for flag in (False, True):
        got = rt.inference_batch(frames, net, flip_tta=flag).to_host()
        tot = np.sum([D.people_agreement(e, r) for e, r in zip(exp, got)], 0)
        found = sum(int(r["n"]) for r in got)
        rows.append(f"  flip_tta={flag!s:5}: {found} people found; of the reference's {tot[0]}: {tot[1]} reproduced exactly, "
                    f"{tot[2]} same root, {tot[3]} of {tot[4]} keypoint cells equal among those")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_merge.txt"))
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if not torch.cuda.is_available():
        text = ("tta merge bench: not measured (no GPU in this run; python tools/bench_tta.py on an MI355X fills this "
                "file)\n")
        with open(a.out, "w") as f:
            f.write(text)
        print(text, end="")
        return
    from pytorch_pose_proposal_network_amd import decode as D, prng, rt, synth, tta

    B, S = a.batch, 384
    lines = [f"tta merge bench: 24 x 24 cells, 21 x 21 windows, K 18, E 17 (7605 channels, 17.5 MB per head), uniform random "
             f"heads, {a.calls} calls after {a.warmup} warm-up, device events, {torch.cuda.get_device_name(0)}",
             "ppn_tta_merge (bytes moved = the two heads read once + the outputs written; with a split > 1 the unary launch also clears the keys):"]
    lines += merge_rows(B, a.calls, a.warmup, (None, 1, 2, 4, 8))
    lines += merge_rows(1, a.calls, a.warmup, (None, 1, 4, 15, 63))

    model, _, _ = rt.network(image_size=S, state_dict=synth.make_state_dict("drn_d_22", 0), compute_dtype="bfloat16")
    frames = torch.from_numpy(prng.u8_frames(3, B, (S, S))).cuda()
    dec = D.Decoder(B, (24, 24), (S, S), model.local_grid_size)
    mg = tta.FlipMerger(B)
    with torch.no_grad():
        t_plain = timed(lambda: rt.inference_batch(frames, model, dec), a.calls, a.warmup)
        t_flip = timed(lambda: rt.inference_batch(frames, model, dec, flip_tta=True, merger=mg), a.calls, a.warmup)
        pair = mg.stage(frames, out=model.input_buffer(2 * B, S, S))
        t_fwd2 = timed(lambda: model.forward_u8(pair), a.calls, a.warmup)
    lines += [
        f"pipeline, batch {B}, drn_d_22 bf16, synthetic weights, one stream:",
        f"  rt.inference_batch                  : {t_plain:9.1f} us per batch = {B / (t_plain * 1e-6):8.0f} images/s",
        f"  rt.inference_batch(flip_tta=True)   : {t_flip:9.1f} us per batch = {B / (t_flip * 1e-6):8.0f} images/s "
        f"= {t_plain / t_flip:5.3f} of the plain rate (two forwards per image: 0.5 at best)",
        f"  of which forward_u8 of the doubled batch with a materialised head pair: {t_fwd2:9.1f} us",
        "people on tests/golden/e2e_tuned_d22_384.npz (float32; information only -- the checkpoint was not trained with "
        "mirror augmentation, no accuracy claim):",
    ]
    lines += agreement_rows()
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
