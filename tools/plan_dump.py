"""CPU: record the ppn_plan_add_* calls a PoseProposalNet plan makes, with every pointer turned back into a name.

Building a plan is host work except for the two weight-pack kernels, the stream pointer and the synchronize.  With those
three stubbed (`recording()`), `PoseProposalNet(...).cuda("cpu")` + `load_state_dict` + `_get_plan` run on a machine
without a GPU, and a proxy in front of libppn.so sees every `ppn_plan_add_*` call and its arguments.  The recording happens
at the C ABI, so the same recorder runs on any two trees: two commits lower their plans identically when the digests match.

    python tools/plan_dump.py [--root OTHER_CHECKOUT] [--out dump.json]      # prints sha256 of the dump over CASES

(--root: import the package from another checkout of this repository, e.g. the parent commit with csrc/libppn.so built or
PPN_LIB pointing at one; tests/test_plan_emit.py shares `recording()` and `record_plan()`.)
"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_KNOBS = ("PPN_STEM_RAW_S2", "PPN_PREFETCH", "PPN_HEAD_EDGE", "PPN_BLOCK64")


class RecordingLib:
    """libppn.so with the weight packers answered by 0 and every ppn_plan_add_* call noted as (name, [arguments])."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name in ("ppn_pack_weight", "ppn_pack_weight_x3"):
            return lambda *a: 0
        if not name.startswith("ppn_plan_add_"):
            return fn

        def rec(handle, *args):
            vals = []
            for v in args:
                if hasattr(v, "_obj"):                                       # byref(descriptor)
                    vals.append({f: (getattr(v._obj, f) if not issubclass(t, C._Pointer) else bool(getattr(v._obj, f)))
                                 for f, t in v._obj._fields_})           # a typed pointer (stats_tiles): NULL or not
                elif isinstance(v, C.Array):
                    vals.append([round(float(x), 9) for x in v])
                else:
                    vals.append(v)
            self.calls.append((name, vals))
            return fn(handle, *args)
        return rec


@contextlib.contextmanager
def recording(L):
    """Inside: `L.load()` is a RecordingLib (yielded), the stream pointer is 0 and torch.cuda.synchronize does nothing."""
    import torch
    saved = (L.load, L.current_stream_ptr, torch.cuda.synchronize)
    px = RecordingLib(L.load())
    L.load, L.current_stream_ptr, torch.cuda.synchronize = (lambda: px), (lambda: 0), (lambda *a, **k: None)
    try:
        yield px
    finally:
        L.load, L.current_stream_ptr, torch.cuda.synchronize = saved


def record_plan(pkg, arch, kw, batch, h, w, u8, fused, conv_flags=0):
    """Build one plan of `pkg` (the imported package) on the CPU.  Returns (net, plan, calls, names): the recorded calls
    with raw pointers, and {pointer: name} over the model's parameters, the plan's buffers and its input."""
    import torch
    A, L, M = pkg.arch, pkg.lib, pkg.model
    with recording(L) as px:
        net = M.PoseProposalNet(arch, insize=(w, h), outsize=(w // 16, h // 16), **kw).cuda("cpu")
        g = torch.Generator().manual_seed(0)
        net.load_state_dict({k: torch.rand(s, generator=g) + 0.5 for k, s in A.param_spec(net.arch, net.lastsize)})
        t0 = time.perf_counter()
        plan = net._get_plan(batch, h, w, u8, fused, 0, conv_flags)
        plan.build_seconds = time.perf_counter() - t0
    names = {t.data_ptr(): "dev:" + k for k, t in net._dev.items() if isinstance(t, torch.Tensor)}
    names.update({t.data_ptr(): f"buf:{k}{tuple(t.shape)}{t.dtype}" for k, t in plan.buffers.items()})
    names[plan.input.data_ptr()] = f"input{tuple(plan.input.shape)}{plan.input.dtype}"
    return net, plan, px.calls, names


def symbolise(calls, names):
    def sym(v):
        if isinstance(v, dict):
            return {k: sym(x) for k, x in v.items()}
        if isinstance(v, int) and v > 4096:
            return names.get(v, "?ptr" if v > (1 << 32) else v)
        return v
    return [(n, [sym(v) for v in vals]) for n, vals in calls]


def _cases():
    bf, f16, f32, x3 = (dict(compute_dtype=n) for n in ("bfloat16", "float16", "float32", "float16x3"))
    modes = [("drn_d_22", bf), ("drn_d_22", dict(bf, stem_dtype="bfloat16", half_prefix=-1)), ("drn_d_22", f16),
             ("drn_d_22", dict(f32, fuse_stem=False)), ("drn_d_22", dict(f32, fuse_stem=True)),
             ("drn_d_22", x3), ("drn_d_22", dict(x3, fuse_stem="all")),
             ("drn_d_22", dict(f16, exact_prefix=3)), ("drn_d_22", dict(f16, exact_prefix=3, fuse_stem="all")),
             ("drn_d_22", dict(f16, exact_prefix=3, fuse_stem=True)),
             ("drn_d_54", bf), ("drn_d_54", dict(f16, exact_prefix=4)), ("drn_d_54", dict(f16, exact_prefix=4, fuse_stem="all")),
             ("drn_d_38", f16), ("drn_d_22", dict(bf, fuse_block=False)), ("drn_d_22", dict(bf, fuse_shortcut=False)),
             ("drn_d_22", dict(bf, local_grid_size=(9, 9)))]
    for arch, kw in modes:
        for size in ((2, 384, 384), (2, 104, 72)):
            for u8 in (True, False):
                for fused in (False, True):
                    yield arch, kw, size, u8, fused, 0, {}, 0
    for arch, kw in modes[:3] + modes[5:6]:                      # conv flags and each plan-time knob switched off once
        yield arch, kw, (2, 384, 384), True, True, 1, {}, 0      # lib.PPN_CONV_NO_FILTER_BANK
        for knob in PLAN_KNOBS:
            yield arch, kw, (2, 104, 72), True, True, 0, {knob: "0"}, 0
        yield arch, kw, (32, 384, 384), True, True, 0, {}, 2     # tile policy 2: convs cut into two pixel ranges


def main(argv):
    root = argv[argv.index("--root") + 1] if "--root" in argv else ROOT
    out = argv[argv.index("--out") + 1] if "--out" in argv else None
    sys.path.insert(0, os.path.abspath(root))
    import pytorch_pose_proposal_network_amd as pkg
    from pytorch_pose_proposal_network_amd import arch, lib, model  # noqa: F401
    res, t_plan = [], 0.0
    for arch_, kw, (b, h, w), u8, fused, flags, env, policy in _cases():
        lib.check(lib.load().ppn_set_conv_tile_policy(policy), "ppn_set_conv_tile_policy")
        for k in PLAN_KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        net, plan, calls, names = record_plan(pkg, arch_, kw, b, h, w, u8, fused, flags)
        t_plan += plan.build_seconds
        sym = symbolise(calls, names)
        unresolved = sum(1 for _, vals in sym for v in vals for x in (v.values() if isinstance(v, dict) else [v]) if x == "?ptr")
        assert not unresolved, (arch_, kw, unresolved)
        res.append({"case": [arch_, {k: str(v) for k, v in kw.items()}, b, h, w, u8, fused, flags, env, policy], "calls": sym,
                    "entries": plan.entries, "flops": plan.flops, "n_ops": plan.n_ops,
                    "buffers": [f"{k}{tuple(t.shape)}{t.dtype}" for k, t in plan.buffers.items()]})
    text = json.dumps(res, indent=0, default=str)
    if out:
        open(out, "w").write(text)
    print(f"{len(res)} plans, {sum(len(r['calls']) for r in res)} calls, {t_plan / len(res) * 1e3:.1f} ms per plan build, "
          f"sha256 {hashlib.sha256(text.encode()).hexdigest()}")


if __name__ == "__main__":
    main(sys.argv)
