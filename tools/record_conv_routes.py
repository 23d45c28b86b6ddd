"""Record which kernel libppn.so runs a ppn_conv_desc on: the fixture tests/golden/conv_routes.json.

One line per unique (descriptor, knobs) entry (compact arrays, see merge(); tests/conv_route_cases.py reads them back): the
descriptor's fields with every pointer reduced to 0 / 1 (splitk_ws: 2 = not 16-byte aligned), the knob state (tile policy, forced tile, conv64 and strip switches), the return code, and either the error text or
ppn_last_conv_kernel(), ppn_last_conv_strip(), *stats_tiles and, under tile policy 2, ppn_conv_split's cut.

    python tools/record_conv_routes.py --gpu OUT.json    # on the GPU: descriptors of real plans and of one training step, launched
    python tools/record_conv_routes.py --layers OUT.json # on the GPU: single layers that no plan of the matrix holds
    python tools/record_conv_routes.py --cpu OUT.json    # no GPU: descriptors the library rejects before its first HIP call
    python tools/record_conv_routes.py --merge GPU.json LAYERS.json CPU.json > tests/golden/conv_routes.json

The expected values are those of the library the recorder runs on, so the fixture is recorded at the commit BEFORE a change of the
dispatch and replayed after it (tests/test_conv_route_cpu.py, tests/test_conv_route_gpu.py).  The `manual` entries at the end are the
only ones written by hand: stride < 1, dilation < 1 and pad < 0 are PPN_E_INVALID ("bad conv geometry"); so are the two `rejected`
entries of the stem3x3 shapes in PPN_F16 / PPN_F16X3, which the library used to run on the bf16 kernel.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEFAULT_KNOBS = {"policy": 0, "ov": [0, 0], "conv64": 1, "strip": 1}
TILE_PAIRS = [(bp, bc) for bc in (64, 128, 256) for bp in (128, 192, 256) if not (bp == 192 and bc == 64)] + [(144, 256)]
MANUAL = [({"stride": 0}, "bad conv geometry"), ({"stride": -1}, "bad conv geometry"), ({"dilation": 0}, "bad conv geometry"),
          ({"pad": -1}, "bad conv geometry"), ({"stride": 0, "flags": 16}, "bad conv geometry")]


def fields(d):
    """ConvDesc -> {field: value}; pointers become 0 / 1."""
    from pytorch_pose_proposal_network_amd import lib as L
    out = {}
    for name, t in L.ConvDesc._fields_:
        v = getattr(d, name)
        if t is C.c_void_p:
            out[name] = 1 if v else 0
        elif issubclass(t, C._Pointer):
            out[name] = 1 if v else 0
        else:
            out[name] = int(v)
    return out


def clone(d):
    from pytorch_pose_proposal_network_amd import lib as L
    c = L.ConvDesc()
    C.memmove(C.byref(c), C.byref(d), C.sizeof(L.ConvDesc))
    return c


def set_knobs(lib, k):
    from pytorch_pose_proposal_network_amd import lib as L
    L.check(lib.ppn_set_conv_tile_policy(k["policy"]), "policy")
    L.check(lib.ppn_set_conv_tile_override(*k["ov"]), "override")
    L.check(lib.ppn_set_conv64_enabled(k["conv64"]), "conv64")
    L.check(lib.ppn_set_conv_strip_enabled(k["strip"]), "strip")


class Recorder:
    def __init__(self, lib):
        self.lib, self.entries, self.seen = lib, [], set()

    def result(self, d, knobs, rc, tiles, source, override_fields=None):
        f = fields(d)
        if override_fields:
            f.update(override_fields)
        e = {"source": source, "d": f, "knobs": knobs, "rc": rc}
        if rc != 0:
            e["error"] = self.lib.ppn_last_error().decode()
        else:
            e["kernel"] = self.lib.ppn_last_conv_kernel().decode()
            e["strip"] = int(self.lib.ppn_last_conv_strip())
            e["stats_tiles"] = int(tiles.value) if tiles is not None else None
            cut = C.c_int64(0)
            if knobs["policy"] == 2 and not (f["flags"] & 16):
                self.lib.ppn_conv_split(f["dtype"], f["cin"], f["cout"], f["batch"] * f["out_h"] * f["out_w"], C.byref(cut))
            e["cut"] = int(cut.value)
        key = json.dumps([e["d"], e["knobs"]], sort_keys=True)
        if key in self.seen:
            return None
        self.seen.add(key)
        self.entries.append(e)
        return e

    def issue(self, d, knobs, source, stream=0, override_fields=None):
        """Launch a copy of `d` under `knobs` (already set) and record what the library reports."""
        key = json.dumps([dict(fields(d), **(override_fields or {})), knobs], sort_keys=True)
        if key in self.seen:
            return None
        c = clone(d)
        tiles = None
        if d.stats_tiles:
            tiles = C.c_int32(-1)
            c.stats_tiles = C.pointer(tiles)
        rc = self.lib.ppn_conv2d_fused(C.byref(c), stream)
        return self.result(c, knobs, rc, tiles, source, override_fields)


# ---- GPU mode -------------------------------------------------------------------------------------------------------------------
class PlanProxy:
    """libppn.so with every ppn_plan_add_conv descriptor copied (its pointers are live plan buffers) and, for the training step,
    every ppn_conv2d_fused call recorded as it is made."""

    def __init__(self, real, rec):
        self._real, self._rec, self.convs, self.train = real, rec, [], False

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name == "ppn_plan_add_conv":
            def add(handle, dref):
                self.convs.append(clone(dref._obj))
                return fn(handle, dref)
            return add
        if name == "ppn_conv2d_fused" and self.train:
            def conv(dref, st):
                rc = fn(dref, st)
                d = dref._obj
                tiles = d.stats_tiles.contents if d.stats_tiles else None
                self._rec.result(d, dict(DEFAULT_KNOBS), rc, tiles, "train")
                return rc
            return conv
        return fn


def gpu_mode(out):
    import numpy as np
    import torch
    import plan_dump
    from pytorch_pose_proposal_network_amd import arch as A, lib as L, model as M, prng, synth
    from pytorch_pose_proposal_network_amd.trainer import PPNTrainer
    from oracle import forward_ref as Fr, targets_ref as T
    lib = L.load()
    rec = Recorder(lib)
    px = PlanProxy(lib, rec)
    real_load = L.load
    L.load = lambda: px
    torch.cuda.set_device(0)

    cases = list(plan_dump._cases())
    bf, f16, f32, x3 = (dict(compute_dtype=n) for n in ("bfloat16", "float16", "float32", "float16x3"))
    # the benchmark's batch-32 shapes under the default policy, and the low-latency (split-K) plans of batch 1-2
    for kw in (bf, f16, f32, x3):
        cases.append(("drn_d_22", kw, (32, 384, 384), True, True, 0, {}, 0))
    for kw in (bf, f16, f32):
        for size in ((1, 384, 384), (2, 104, 72)):
            cases.append(("drn_d_22", dict(kw, latency=True), size, True, True, 0, {}, 0))
    variants = {}                                                     # descriptors re-issued under the other knob states
    for i, (arch_, kw, (b, h, w), u8, fused, flags, env, policy) in enumerate(cases):
        for k in plan_dump.PLAN_KNOBS:
            os.environ.pop(k, None)
        os.environ.update(env)
        knobs = dict(DEFAULT_KNOBS, policy=policy)
        set_knobs(lib, knobs)
        px.convs = []
        net = M.PoseProposalNet(arch_, insize=(w, h), outsize=(w // 16, h // 16), **kw).cuda()
        g = torch.Generator().manual_seed(0)
        net.load_state_dict({k: torch.rand(s, generator=g) + 0.5 for k, s in A.param_spec(net.arch, net.lastsize)})
        plan = net._get_plan(b, h, w, u8, fused, 0, flags)
        st = L.current_stream_ptr()
        n0 = len(rec.entries)
        for d in px.convs:
            e = rec.issue(d, knobs, "plan", st)
            # the plans above run their 64-channel layers through block64 / the fused stem: every descriptor in the scope of the
            # filter bank kernel, from whichever plan, is varied too (conv64 off and PPN_CONV_NO_FILTER_BANK change only those)
            c64 = d.dtype in (L.PPN_BF16, L.PPN_F16) and d.cin == 64 and d.cout == 64 and d.ksize == 3 and d.stride == 1
            vary = (b == 32 and policy == 0) or (b == 2 and h == 104 and arch_ == "drn_d_22" and not env and len(kw) == 1) or c64
            if e is not None and e["rc"] == 0 and vary:
                variants[json.dumps(e["d"], sort_keys=True)] = (e["d"], clone(d))
        if variants:
            # policy 1 and 2, a shared GPU, the strip loader off, conv64 off (switch and flag), and every admissible forced tile on
            # one plain descriptor per (dtype, Cout)
            seen_cout = set()
            for f, d in variants.values():
                for kn in (dict(DEFAULT_KNOBS, policy=1), dict(DEFAULT_KNOBS, policy=2), dict(DEFAULT_KNOBS, strip=0),
                           dict(DEFAULT_KNOBS, conv64=0)):
                    if kn["policy"] and f["batch"] != 32:
                        continue
                    set_knobs(lib, kn)
                    rec.issue(d, kn, "plan", st)
                set_knobs(lib, DEFAULT_KNOBS)
                for flag in (L.PPN_CONV_SHARED_GPU, L.PPN_CONV_NO_FILTER_BANK):
                    c = clone(d)
                    c.flags |= flag
                    rec.issue(c, dict(DEFAULT_KNOBS), "plan", st)
                cls = (f["dtype"], f["cout"])
                bk = 32 if f["dtype"] == L.PPN_F32 else 64
                if (cls not in seen_cout and f["cout"] >= 64 and f["cin"] % bk == 0 and not f["src2"] and not f["limb_edge_pad"]
                        and not f["out_nchw_f32"] and not (f["flags"] & L.PPN_CONV_SPLIT_K) and f["m_count"] == 0):
                    seen_cout.add(cls)
                    for bp, bc in TILE_PAIRS:
                        kn = dict(DEFAULT_KNOBS, ov=[bp, bc])
                        set_knobs(lib, kn)
                        rec.issue(d, kn, "plan", st)
            variants.clear()
        torch.cuda.synchronize()
        del plan, net
        print(f"case {i + 1}/{len(cases)}: {arch_} {kw} {b}x{h}x{w}: {len(px.convs)} convs, +{len(rec.entries) - n0} entries", flush=True)
    set_knobs(lib, DEFAULT_KNOBS)

    # one training step per dtype behind the proxy: forward (stats_mode 1), input gradient (stats_mode 2), stride-2 parity launches
    for dt in (L.PPN_BF16, L.PPN_F32):
        size, batch = 96, 2
        tr = PPNTrainer("drn_d_22", synth.make_state_dict("drn_d_22", 0), compute_dtype=dt, insize=(size, size))
        x = torch.as_tensor(Fr.normalize_u8(prng.u8_frames(11, batch, (size, size)))).cuda()
        tg = {k: torch.from_numpy(v).cuda() for k, v in
              T.synthetic_batch(12, batch, insize=(size, size), outsize=(size // 16, size // 16)).items()}
        n0 = len(rec.entries)
        px.train = True
        tr.train_step(x, tg)
        torch.cuda.synchronize()
        px.train = False
        print(f"train step dtype {dt}: +{len(rec.entries) - n0} entries", flush=True)
    L.load = real_load
    write(out, rec.entries)


def layers_mode(out):
    """Single layers under tile policy 2: 512 -> 512 1x1 at 16 x 48 x 48, by the cost tables the smallest launch that is cut in two."""
    import torch
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    rec = Recorder(lib)
    torch.cuda.set_device(0)
    knobs = dict(DEFAULT_KNOBS, policy=2)
    set_knobs(lib, knobs)
    for dt, tdt in ((L.PPN_BF16, torch.bfloat16), (L.PPN_F16, torch.float16), (L.PPN_F32, torch.float32)):
        d = valid(L, dt, 512, 512, k=1, size=48, batch=16)
        bufs = [torch.zeros(16 * 48 * 48 * 512, dtype=tdt, device="cuda"), torch.zeros(d.cout_pad * d.k_total, dtype=tdt, device="cuda"),
                torch.zeros(16 * 48 * 48 * 512, dtype=tdt, device="cuda"), torch.zeros(1024, device="cuda")]
        d.src, d.weight, d.out_raw, d.zero_page = (b.data_ptr() for b in bufs)
        print(rec.issue(d, knobs, "layer", L.current_stream_ptr()), flush=True)
        torch.cuda.synchronize()
    set_knobs(lib, DEFAULT_KNOBS)
    write(out, rec.entries)


# ---- CPU mode: rejected descriptors ---------------------------------------------------------------------------------------------
def valid(L, dtype, cin, cout, k=3, size=16, stride=1, dil=1, batch=2, **over):
    """A descriptor the library accepts (generic or large-tile kernel), every needed pointer non-NULL."""
    _, _, _, ktot, cpad = L.conv_tiling(dtype, cin, cout, k)
    pad = dil * (k - 1) // 2
    d = L.ConvDesc()
    d.dtype, d.batch, d.in_h, d.in_w, d.cin, d.cout = dtype, batch, size, size, cin, cout
    eff = dil * (k - 1) + 1
    d.out_h = d.out_w = (size + 2 * pad - eff) // stride + 1
    d.ksize, d.stride, d.dilation, d.pad, d.k_total, d.cout_pad = k, stride, dil, pad, ktot, cpad
    d.src = d.weight = d.zero_page = d.out_raw = 0x1000
    for name, v in over.items():
        setattr(d, name, v)
    return d


def negatives(L):
    """(descriptor, field overrides for the record) pairs: each is a valid descriptor with one thing changed."""
    F32, BF, F16, X3 = L.PPN_F32, L.PPN_BF16, L.PPN_F16, L.PPN_F16X3
    P = 0x1000
    tiles = C.pointer(C.c_int32(0))
    out = []

    def neg(d, **over):
        for name, v in over.items():
            setattr(d, name, v)
        out.append(d)

    g = lambda **kw: valid(L, BF, 128, 128, **kw)                      # noqa: E731  large-tile base
    s = lambda **kw: valid(L, F32, 16, 24, **kw)                       # noqa: E731  generic (small Cin) base
    st = dict(stats_partial=P, stats_tiles=tiles)
    st2 = dict(st, stats_mode=2, stats_x=P, stats_gamma=P, stats_beta=P, stats_mean=P, stats_rstd=P)
    # conv_launch, in order
    neg(g(), stats_mode=3, **st)
    neg(g(), stats_mode=1, stats_partial=P)
    neg(g(), stats_mode=1, stats_tiles=tiles)
    neg(g(**st2), stats_x=None)
    neg(g(**st2), stats_act=L.PPN_ACT_SIGMOID)
    neg(g(), dtype=7)
    neg(g(), batch=0)
    neg(g(), cout=0)
    neg(g(), ksize=6)
    neg(g(), ksize=0)
    neg(valid(L, F32, 16, 24), cin=18)
    neg(valid(L, BF, 16, 24), cin=20)
    neg(g(), out_h=15)
    neg(g(), in_w=17)
    neg(valid(L, F32, 16, 16, k_total=144, cout_pad=16, act1=L.PPN_ACT_RELU, scale1=P, shift1=P), src=None)     # stem3x3 route
    neg(valid(L, F32, 16, 32, k_total=144, cout_pad=32), weight=None)
    neg(valid(L, F32, 16, 16, k_total=144, cout_pad=16), out_raw=None)                                           # stem3x3_launch
    # stem3x3.hip has no IEEE-half form (these two entries of the fixture were written by hand when the refusal was added)
    neg(valid(L, F32, 16, 16, k_total=144, cout_pad=16, act1=L.PPN_ACT_RELU, scale1=P, shift1=P), dtype=F16)
    neg(valid(L, F32, 16, 32, stride=2, k_total=144, cout_pad=32), dtype=X3)
    neg(valid(L, F32, 8, 24), cin=24, k_total=224)
    neg(valid(L, X3, 64, 128), cout=32)
    neg(valid(L, X3, 64, 128), limb_edge_pad=448)
    sc = dict(src2=P, cin2=64, stride2=1, in2_h=16, in2_w=16)
    neg(valid(L, X3, 64, 128), **sc)
    neg(g(k_total=9 * 128 + 64, **sc), cin2=32)
    neg(g(k_total=9 * 128 + 64, **sc), scale1=P)
    neg(g(k_total=9 * 128 + 64, **sc), in2_h=15)
    neg(g(k_total=9 * 128 + 64, **sc), stride2=0)
    neg(g(), k_total=9 * 128 + 64)
    neg(valid(L, BF, 64, 64, k=1, size=64), batch=1 << 20)                                                       # m_all > 2^31
    neg(g(), m_begin=500, m_count=100)
    neg(g(), m_begin=-4, m_count=8)
    nchw = dict(out_nchw_f32=1, act1=L.PPN_ACT_SIGMOID)
    neg(g(**nchw), m_begin=2, m_count=64)
    neg(g(**nchw), m_begin=0, m_count=66)
    head = dict(nchw, k=1, out_raw=None, argmax_keys=P, limb_edge_pad=448, limb_window=441, shift1=P)
    hd = lambda **kw: valid(L, BF, 128, 441 * 2, **dict(head, cout_pad=896, **kw))                               # noqa: E731
    neg(hd(), limb_edge_pad=256)
    neg(hd(), out_raw=P)
    neg(hd(), limb_window=449)
    neg(valid(L, BF, 128, 432 * 2, **dict(head, cout_pad=896)), limb_window=432)                                 # pad rows below the last 16
    neg(valid(L, BF, 128, 420 * 2, **dict(head, cout_pad=896)), limb_window=420)
    neg(hd(), act1=L.PPN_ACT_NONE)
    neg(hd(), cout_pad=1024)
    neg(hd(), src=None)
    neg(hd(), scale1=P)                                                                                          # head_limb_launch
    neg(valid(L, BF, 64, 441 * 2, **dict(head, cout_pad=896)))                                                   # odd K steps
    neg(valid(L, F32, 128, 441 * 2, **dict(head, cout_pad=896, size=2048, batch=2)))                              # too large
    neg(g(), cout_pad=192)
    neg(g(), cout_pad=64)
    neg(s(), cout_pad=16)
    neg(g(), src=None)
    neg(g(), zero_page=None)
    neg(s(), weight=None)
    neg(g(), out_raw=None)
    am = dict(nchw, argmax_keys=P, unary_out=P, unary_channels=28, limb_window=25)
    neg(g(**am), out_nchw_f32=0)
    neg(g(**am), unary_out=None)
    neg(g(**am), limb_window=0)
    neg(g(**am), unary_channels=27)
    neg(g(**am), unary_channels=200)
    neg(g(**am), act1=L.PPN_ACT_RELU)
    neg(g(), act1=L.PPN_ACT_SIGMOID)
    neg(g(), act2=L.PPN_ACT_SIGMOID, out_act=P)
    neg(g(**nchw), residual=P)
    neg(g(**nchw), out_act=P)
    neg(valid(L, F32, 32, 16), cout=12)
    neg(valid(L, BF, 128, 128, k=1, size=96), batch=4096)                                                        # in_elems > 2^31
    neg(g(k_total=9 * 128 + 64, **sc), in2_h=4096, in2_w=4096)                                                    # src2 too large
    neg(g(), flags=L.PPN_CONV_X3_PLAIN_OUT)
    neg(valid(L, X3, 64, 128, k_total=3 * 576, **nchw), flags=L.PPN_CONV_X3_PLAIN_OUT)
    neg(g(), flags=L.PPN_CONV_OUT_BF16)
    neg(valid(L, F16, 16, 24), flags=L.PPN_CONV_OUT_BF16)
    neg(valid(L, F16, 128, 128, **nchw), flags=L.PPN_CONV_OUT_BF16)
    neg(valid(L, BF, 64, 32, **dict(am, unary_channels=7)))                                                      # arg-max, not big
    neg(valid(L, BF, 64, 32, **dict(sc, k_total=9 * 64 + 64)))                                                   # shortcut, not big
    neg(valid(L, BF, 64, 64, flags=L.PPN_CONV_NO_FILTER_BANK, **dict(sc, k_total=9 * 64 + 64)))                  # launch_one
    neg(valid(L, F32, 128, 128, k=1, size=1024), batch=4)                                                        # launch_big
    # conv64_launch
    c64 = lambda **kw: valid(L, BF, 64, 64, **kw)                      # noqa: E731
    neg(c64(), src=None)
    neg(c64(), out_raw=None)
    neg(c64(size=4096), batch=2)
    # split-K (flags 16)
    SK = L.PPN_CONV_SPLIT_K
    k = lambda **kw: valid(L, BF, 512, 512, size=8, flags=SK, splitk_ws=P, splitk_ws_bytes=1 << 40, **kw)        # noqa: E731
    neg(k(), dtype=9)
    neg(valid(L, X3, 64, 128, flags=SK))
    neg(k(), src2=P)
    neg(k(), out_nchw_f32=1)
    neg(k(), unary_out=P)
    neg(k(), limb_edge_pad=448)
    neg(k(), stats_mode=1, **st)
    neg(k(), flags=SK | L.PPN_CONV_X3_PLAIN_OUT)
    neg(k(), flags=SK | L.PPN_CONV_OUT_BF16)
    neg(k(), batch=0)
    neg(k(), pad=-1)
    neg(k(), dilation=0)
    neg(valid(L, BF, 512, 512, k=5, size=8, flags=SK, splitk_ws=P, splitk_ws_bytes=1 << 40))
    neg(k(), cin=96)
    neg(k(), m_count=16)
    neg(k(), act1=L.PPN_ACT_SIGMOID)
    neg(k(), act2=-1)
    neg(k(), cout=508)
    neg(k(), cout_pad=544)
    neg(k(), cout_pad=448)
    neg(k(), out_w=7)
    neg(k(), pad=0, in_h=1, out_h=-1, out_w=6)
    neg(k(), k_total=9 * 512 + 64)
    neg(valid(L, BF, 64, 64, k=1, size=64, flags=SK, splitk_ws=P, splitk_ws_bytes=1 << 40), batch=1 << 20)
    neg(valid(L, BF, 128, 128, k=1, size=96, flags=SK, splitk_ws=P, splitk_ws_bytes=1 << 40), batch=4096)
    neg(k(), cout=1 << 21, cout_pad=1 << 21)
    neg(k(), src=None)
    neg(k(), out_raw=None)
    neg(k(), splitk_ws=None)
    neg(k(), splitk_ws_bytes=1024)
    neg(k(), splitk_ws=P + 4)
    big = 3728384                                                       # 9 * cin / 512 slabs > 65535
    neg(valid(L, BF, 512, 64, size=8, batch=1, flags=SK, splitk_ws=P, splitk_ws_bytes=1 << 40), cin=big, k_total=9 * big)
    return out


def cpu_mode(out):
    from pytorch_pose_proposal_network_amd import lib as L
    lib = L.load()
    rec = Recorder(lib)
    set_knobs(lib, DEFAULT_KNOBS)
    dropped = 0
    for d in negatives(L):
        over = {"splitk_ws": 2} if d.splitk_ws and d.splitk_ws & 15 else None
        e = rec.issue(d, dict(DEFAULT_KNOBS), "rejected", 0, over)
        # a descriptor that got as far as a HIP call (which fails without a device) is not a negative case
        if e is not None and e["rc"] in (0, -2):                        # PPN_OK / PPN_E_HIP
            rec.entries.remove(e)
            dropped += 1
            print("dropped (not rejected before the launch):", e, flush=True)
    rc = lib.ppn_conv2d_fused(None, 0)                                  # the NULL descriptor
    rec.entries.append({"source": "rejected", "d": None, "knobs": dict(DEFAULT_KNOBS), "rc": rc,
                        "error": lib.ppn_last_error().decode()})
    base = valid(L, L.PPN_BF16, 128, 128)
    for over, msg in MANUAL:                                            # written by hand, never issued: stride 0 divides by zero
        f = dict(fields(base), **over)
        if over.get("flags") == 16:
            f.update(splitk_ws=1, splitk_ws_bytes=1 << 40)
        rec.entries.append({"source": "manual", "d": f, "knobs": dict(DEFAULT_KNOBS), "rc": -1, "error": msg})
    print(f"{len(rec.entries)} rejected entries, {dropped} dropped", flush=True)
    write(out, rec.entries)


# scalar fields in the order the fixture stores them: the ones that are usually 0 last, so that trailing zeros can be cut
SCALARS = ["dtype", "batch", "in_h", "in_w", "cin", "out_h", "out_w", "cout", "ksize", "stride", "dilation", "pad", "k_total",
           "cout_pad", "act1", "act2", "out_nchw_f32", "prefetch_bytes", "flags", "in2_h", "in2_w", "cin2", "stride2", "unary_channels",
           "limb_window", "limb_edge_pad", "m_begin", "m_count", "stats_mode", "stats_act", "splitk_ws_bytes", "splitk_ws_misaligned"]


def merge(paths):
    """The fixture (read back by tests/conv_route_cases.py): a header line, then one line per entry
        [source, pointer mask, scalars (trailing zeros cut), knob state, rc, error]                       rejected
        [source, pointer mask, scalars, knob state, 0, kernel, strip, stats_tiles (-1: not asked), cut]     accepted
    with knob states and kernel names as indices into the header's tables.  Left out: entries that repeat another's scalar
    fields (prefetch_bytes aside), knobs, outcome and its src2 / residual / out_act / argmax_keys pointers; a strip-off /
    conv64-off / PPN_CONV_SHARED_GPU / PPN_CONV_NO_FILTER_BANK variant that records what the same descriptor records without
    it; and forced tiles on more than one descriptor per Cout."""
    from pytorch_pose_proposal_network_amd import lib as L
    names = [n for n, _ in L.ConvDesc._fields_]
    pointers = [n for n in names if n not in SCALARS]
    entries = [json.loads(line) for p in paths for line in open(p)]
    outcome = lambda e: [e.get(k) for k in ("rc", "error", "kernel", "strip", "stats_tiles", "cut")]          # noqa: E731
    plain = {}
    for e in entries:
        if e["d"] is not None and e["knobs"] == DEFAULT_KNOBS:
            plain[json.dumps(dict(e["d"], prefetch_bytes=0), sort_keys=True)] = outcome(e)
    seen, forced, states, kernels, lines = set(), {}, [], [], []
    for e in entries:
        d, k = e["d"], e["knobs"]
        kv = [k["policy"], k["ov"][0], k["ov"][1], k["conv64"], k["strip"]]
        if d is not None:
            route_ptrs = ("src2", "residual", "out_act", "argmax_keys")
            key = json.dumps([[d[n] for n in SCALARS if n in d and n != "prefetch_bytes"], [d[n] for n in route_ptrs], kv, outcome(e)]
                             if e["rc"] == 0 else [dict(d, prefetch_bytes=0), kv])
            if key in seen:
                continue
            seen.add(key)
            base = None
            if k != DEFAULT_KNOBS and k["policy"] == 0 and k["ov"] == [0, 0]:
                base = dict(d, prefetch_bytes=0)
            elif k == DEFAULT_KNOBS and e["source"] == "plan" and d["flags"] & 3:
                base = dict(d, prefetch_bytes=0, flags=d["flags"] & ~3)
            if base is not None and plain.get(json.dumps(base, sort_keys=True)) == outcome(e):
                continue
            if k["ov"] != [0, 0] and forced.setdefault(d["cout"], json.dumps(dict(d, prefetch_bytes=0))) != json.dumps(dict(d, prefetch_bytes=0)):
                continue
        if kv not in states:
            states.append(kv)
        c = [e["source"][0]]
        if d is None:
            c += [None, []]
        else:
            sc = [(1 if d["splitk_ws"] == 2 else 0) if n == "splitk_ws_misaligned" else d[n] for n in SCALARS]
            while sc and sc[-1] == 0:
                sc.pop()
            c += [sum(1 << i for i, n in enumerate(pointers) if d[n]), sc]
        c += [states.index(kv), e["rc"]]
        if e["rc"] != 0:
            c.append(e["error"])
        else:
            if e["kernel"] not in kernels:
                kernels.append(e["kernel"])
            c += [kernels.index(e["kernel"]), e["strip"], -1 if e["stats_tiles"] is None else e["stats_tiles"], e["cut"]]
        lines.append(json.dumps(c, separators=(",", ":")))
    print(json.dumps({"fields": names, "pointers": pointers, "scalars": SCALARS, "knob_fields": ["policy", "ov_bp", "ov_bc", "conv64", "strip"],
                      "knob_states": states, "kernels": kernels,
                      "sources": {"p": "plan", "t": "train", "l": "layer", "r": "rejected", "m": "manual"}}, separators=(",", ":")))
    print("\n".join(lines))


def write(path, entries):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        for e in entries:
            f.write(json.dumps(e, sort_keys=True, separators=(",", ":")) + "\n")
    print(f"{len(entries)} entries -> {path}", flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "--gpu":
        gpu_mode(sys.argv[2])
    elif sys.argv[1] == "--layers":
        layers_mode(sys.argv[2])
    elif sys.argv[1] == "--cpu":
        cpu_mode(sys.argv[2])
    elif sys.argv[1] == "--merge":
        merge(sys.argv[2:])
