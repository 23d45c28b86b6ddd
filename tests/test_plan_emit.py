"""CPU: `PoseProposalNet._build_plan` emits exactly what `lowering.lower` decided.  The plan is built on the CPU behind the
recording proxy of tools/plan_dump.py (weight packers answered by 0, stream pointer 0, no synchronize); the recorded
ppn_plan_add_* sequence must have the kinds and names of lower()'s records in order, every pointer argument must be the
buffer or the `_dev` entry the record names, and every scalar field the record's.  Needs libppn.so; no GPU."""
import ctypes as C
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"ppn_plan_add_conv": ("conv",), "ppn_plan_add_block": ("block",), "ppn_plan_add_split": ("split",),
         "ppn_plan_add_memset": ("memset",), "ppn_plan_add_stem": ("stem",), "ppn_plan_add_stem01": ("stem01",),
         "ppn_plan_add_stem012_dt": ("stem012",)}


@pytest.fixture(scope="module")
def PD():
    import pytorch_pose_proposal_network_amd as pkg
    from pytorch_pose_proposal_network_amd import arch, build, lib, lowering, model  # noqa: F401
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(ROOT, "tools", "plan_dump.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return pkg, mod


CASES = [("drn_d_22", dict(compute_dtype="bfloat16"), (2, 104, 72), True, True, 0),
         ("drn_d_22", dict(compute_dtype="bfloat16", local_grid_size=(9, 9)), (2, 96, 96), True, True, 1),
         ("drn_d_22", dict(compute_dtype="float32"), (1, 96, 96), False, False, 0),
         ("drn_d_22", dict(compute_dtype="float32", fuse_stem=True), (2, 96, 96), True, False, 0),
         ("drn_d_22", dict(compute_dtype="float16x3"), (2, 96, 96), True, True, 0),
         ("drn_d_54", dict(compute_dtype="float16", exact_prefix=4, fuse_stem="all"), (2, 96, 96), True, True, 0)]


@pytest.mark.parametrize("arch,kw,shape,u8,fused,flags", CASES)
def test_emitted_calls_are_the_lowered_records(PD, arch, kw, shape, u8, fused, flags):
    pkg, pd = PD
    LW = pkg.lowering
    b, h, w = shape
    net, plan, calls, names = pd.record_plan(pkg, arch, kw, b, h, w, u8, fused, flags)
    sw, sh = net.local_grid_size
    low = LW.lower(net._ops, net.mode, b, h, w, u8, fused, flags, n_unary=6 * len(net.keypoint_names),
                   n_edges=len(net.edges), limb_window=sw * sh)
    assert plan.entries == low.entries and plan.flops == low.flops and plan.n_ops == len(calls) == len(low.launches)
    assert list(plan.buffers) == [n for n in low.tensors if n != "input"]
    for name, (tshape, _) in low.tensors.items():
        assert tuple((plan.input if name == "input" else plan.buffers[name]).shape) == tshape

    def tensor_ptr(name):
        return (plan.input if name == "input" else plan.buffers[name]).data_ptr()

    def param_ptr(key):
        return net._dev[key].data_ptr() if key in net._dev else None
    used = set()
    for (fn, args), l in zip(calls, low.launches):
        assert l.kind in KINDS[fn], (fn, l.kind, l.name)
        if l.kind in ("conv", "block"):
            (d,) = args
            want = {f: 0 for f in d}
            want.update({f: None for f, t in (pkg.lib.ConvDesc if l.kind == "conv" else pkg.lib.BlockDesc)._fields_
                         if t is C.c_void_p})
            want.update({f: False for f in d if d[f] is False})           # typed pointers: recorded as NULL or not
            want.update(l.scalars)
            want.update({f: tensor_ptr(n) for f, n in l.tensors.items()})
            want.update({f: param_ptr(k) for f, k in l.params.items()})
            if want.get("prefetch"):
                t = net._dev[l.params["prefetch"]]
                want["prefetch_bytes"] = t.numel() * t.element_size()
            assert d == want, (l.name, {f: (d[f], want[f]) for f in d if d[f] != want[f]})
        elif l.kind == "split":
            assert args == [tensor_ptr(l.tensors["src"]), l.scalars["rows"], l.scalars["channels"], tensor_ptr(l.tensors["dst"])]
        elif l.kind == "memset":
            assert args == [tensor_ptr(l.tensors["dst"]), l.scalars["bytes"]]
        else:
            s, p = l.scalars, [param_ptr(k) for k in l.params.values()]
            assert len(p) == {"stem": 3, "stem01": 6, "stem012": 11}[l.kind]
            want = [s["dtype"], s["src_is_u8"], tensor_ptr("input"), b, h, w, *p[:3], args[9], args[10], *p[3:]]
            want += [tensor_ptr(l.tensors[f]) if f in l.tensors else None
                     for f in (("out_raw", "out_act") if l.kind == "stem012" else ("out_raw",))]
            assert args == want, l.name
            assert args[9] == [round(float(x), 9) for x in net._mean] and args[10] == [round(float(x), 9) for x in net._std]
        used.update(k for k in l.params.values() if k in net._dev)
    # every pointer is a named one, and every packed weight of the model is an operand of some launch
    assert all(names.get(v) for _, args in calls for a in args for v in (a.values() if isinstance(a, dict) else [a])
               if isinstance(v, int) and not isinstance(v, bool) and v > (1 << 32))
    unused = {k for k in net._dev if k.endswith(".w")} - used
    assert unused <= ({"conv3.w"} if "conv3.w_edge" in used else set()), unused


def test_a_dev_entry_added_before_the_plan_is_picked_up(PD):
    """Diagnostic tools plant operands (tools/clock_conv_seq.py: a `.b2` buffer on a launch without a second output)."""
    import torch
    pkg, pd = PD
    with pd.recording(pkg.lib) as px:
        net = pkg.model.PoseProposalNet("drn_d_22", insize=(96, 96), outsize=(6, 6), compute_dtype="bfloat16").cuda("cpu")
        g = torch.Generator().manual_seed(0)
        net.load_state_dict({k: torch.rand(s, generator=g) + 0.5 for k, s in pkg.arch.param_spec(net.arch, net.lastsize)})
        assert "backbone.7.0.b2" not in net._dev
        probe = net._dev["backbone.7.0.b2"] = torch.zeros(8, dtype=torch.int64)
        net._get_plan(2, 96, 96, True)
    (d,) = [a[0] for fn, a in px.calls if fn == "ppn_plan_add_conv" and a[0]["weight"] == net._dev["backbone.7.0.w"].data_ptr()]
    assert d["shift2"] == probe.data_ptr() and d["scale2"] is None
