"""GPU: record every libppn call of PPNTrainer.train_step at the C ABI, and digest the state three steps leave behind.

A proxy in front of `lib.load()` (as tools/plan_dump.py's RecordingLib does for plans) notes, for train_step numbers 1 and 2
(step 2 carries the prefetch chain and the batched repack): the function name in call order, every scalar argument and
descriptor field, for every pointer NULL or not -- pointers into the flat parameter / gradient / running-statistics stores as
owning name + offset -- and the stream as the index of its first appearance.  The recording happens at the C ABI, so the same
recorder runs on any two trees: two commits enqueue the same training step when `calls_sha256` matches, and compute the same
when `state_sha256` (flat parameters, last gradients, running statistics, task weights, the losses of the three steps) does.

    python tools/train_calls.py CONFIG [--root OTHER_CHECKOUT] [--out calls.json]     # one configuration per process
    python tools/train_calls.py --list

(--root: import the package from another checkout, e.g. the parent commit with csrc/libppn.so built.  The PPN_TRAIN_* knobs
of a configuration are set before the package is imported: they are read at import / construction time.)
Prints one JSON line; `enqueue_ms`: host time of the train_step calls 2 and 3 (the step is partly bound by it).
"""
import bisect
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, BATCH = 96, 2
CONFIGS = {   # name: (arch, compute dtype, second_order, environment)
    "d22_bf16_so": ("drn_d_22", "bf16", True, {}),
    "d22_bf16_fo": ("drn_d_22", "bf16", False, {}),
    "d22_f32_so": ("drn_d_22", "f32", True, {}),
    "d22_f32_fo": ("drn_d_22", "f32", False, {}),
    "d54_bf16_so": ("drn_d_54", "bf16", True, {}),
    "d22_bf16_so_fuse0": ("drn_d_22", "bf16", True, {"PPN_TRAIN_FUSE_STATS": "0"}),
    "d22_bf16_so_fuse2": ("drn_d_22", "bf16", True, {"PPN_TRAIN_FUSE_STATS": "2"}),
    "d22_bf16_so_side0": ("drn_d_22", "bf16", True, {"PPN_TRAIN_SIDE_STREAM": "0"}),
    "d22_bf16_so_stacked0": ("drn_d_22", "bf16", True, {"PPN_TRAIN_STACKED_PROBES": "0"}),
    "d22_bf16_so_spec0": ("drn_d_22", "bf16", True, {"PPN_TRAIN_SPECULATE_TAIL": "0"}),
}


class RecordingLib:
    """libppn.so with every call noted as (name, [symbolised arguments]) while `on`."""

    def __init__(self, real, sym):
        self._real, self._sym, self.calls, self.on = real, sym, [], False

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("ppn_") or name == "ppn_last_error":
            return fn
        types = fn.argtypes or []

        def rec(*args):
            if self.on:
                self.calls.append((name, [self._sym.arg(v, types[i] if i < len(types) else None, i == len(args) - 1)
                                          for i, v in enumerate(args)]))
            return fn(*args)
        return rec


class Symbols:
    """pointer -> owning name + offset for the trainer's flat stores; stream -> index of first appearance"""

    def __init__(self):
        self.ranges, self.streams = [], {}

    def add_store(self, tag, tensor, names_offsets):
        offs = sorted((o * tensor.element_size(), n) for n, o in names_offsets)
        self.ranges.append((tensor.data_ptr(), tensor.numel() * tensor.element_size(), tag, [o for o, _ in offs], [n for _, n in offs]))

    def pointer(self, v):
        if not v:
            return "NULL"
        for base, size, tag, offs, names in self.ranges:
            if base <= v < base + size:
                i = bisect.bisect_right(offs, v - base) - 1
                return f"{tag}:{names[i]}+{v - base - offs[i]}"
        return "ptr"

    def field(self, v, t):
        if t is C.c_void_p:
            return self.pointer(v)
        if isinstance(t, type) and issubclass(t, C._Pointer):
            return bool(v)                                                   # a typed pointer (stats_tiles): NULL or not
        if isinstance(v, C.Array):
            return [x for x in v]
        return repr(v) if isinstance(v, float) else v

    def struct(self, s):
        return {f: self.field(getattr(s, f), t) for f, t in s._fields_}

    def arg(self, v, t, last):
        if last and t is C.c_void_p:                                         # every launch takes its stream last
            return "stream#%d" % self.streams.setdefault(v or 0, len(self.streams))
        if hasattr(v, "_obj"):                                               # byref(...)
            return self.struct(v._obj) if hasattr(v._obj, "_fields_") else "out"
        if isinstance(v, C.Array):
            return [self.struct(x) if hasattr(x, "_fields_") else repr(float(x)) for x in v]
        if t is C.c_void_p:
            return self.pointer(v)
        return repr(v) if isinstance(v, float) else v


def main(argv):
    if "--list" in argv:
        print(" ".join(CONFIGS))
        return
    name = argv[1]
    arch, dt, second, env = CONFIGS[name]
    root = argv[argv.index("--root") + 1] if "--root" in argv else ROOT
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    for k in [k for k in os.environ if k.startswith("PPN_TRAIN_")]:
        os.environ.pop(k)
    os.environ.update(env)
    sys.path.insert(0, os.path.abspath(root))
    import numpy as np
    import torch
    from oracle import forward_ref as Fr, targets_ref as Tg
    from pytorch_pose_proposal_network_amd import lib as L, prng, synth
    from pytorch_pose_proposal_network_amd.trainer import PPNTrainer

    sym = Symbols()
    px = RecordingLib(L.load(), sym)
    L.load = lambda: px
    torch.manual_seed(0)
    tr = PPNTrainer(arch, synth.make_state_dict(arch, 0), compute_dtype=L.PPN_F32 if dt == "f32" else L.PPN_BF16,
                    insize=(SIZE, SIZE), second_order=second)
    tr.base = torch.full((5,), 0.5, device="cuda")
    sym.add_store("P", tr.flat, tr.offset.items())
    sym.add_store("G", tr._grad_store, [("(prefix)", 0)] + [(n, o + 16) for n, o in tr.offset.items()])
    for n, b in tr.buffers.items():
        sym.add_store("B", b, [(n, 0)])
    h = hashlib.sha256()
    enqueue, losses_all = [], []
    for step in range(3):
        x = torch.as_tensor(Fr.normalize_u8(prng.u8_frames(100 + step, BATCH, (SIZE, SIZE)))).cuda()
        tg = {k: torch.from_numpy(v).cuda() for k, v in
              Tg.synthetic_batch(200 + step, BATCH, insize=(SIZE, SIZE), outsize=(SIZE // 16, SIZE // 16)).items()}
        torch.cuda.synchronize()
        px.on = step < 2
        t0 = time.perf_counter()
        losses, w = tr.train_step(x, tg)
        enqueue.append((time.perf_counter() - t0) * 1e3)
        px.on = False
        torch.cuda.synchronize()
        losses_all.append(losses.cpu().numpy())
        h.update(losses_all[-1].tobytes())
    for t in [tr.flat, tr.grad, tr.task.w] + [tr.buffers[n] for n in sorted(tr.buffers)]:
        h.update(t.detach().cpu().numpy().tobytes())
    text = json.dumps(px.calls, indent=0, default=str)
    if out:
        open(out, "w").write(text)
    print(json.dumps({"config": name, "root": os.path.relpath(root, ROOT), "calls": len(px.calls),
                      "calls_sha256": hashlib.sha256(text.encode()).hexdigest(), "state_sha256": h.hexdigest(),
                      "enqueue_ms": [round(v, 3) for v in enqueue[1:]],
                      "losses": [np.round(v, 6).tolist() for v in losses_all]}))


if __name__ == "__main__":
    main(sys.argv)
