"""GPU: the launchers honour the route.  For every route kind and instantiation flag, the smallest entry of
tests/golden/conv_routes.json that reaches it is launched with real buffers through ppn_conv2d_fused; kernel name, strip flag
and *stats_tiles must be the recorded ones (recorded before the dispatch moved into csrc/conv_route.cpp), and the strip loader,
the statistics epilogue and the two-segment launch must leave the outputs bit-identical to the same launch without them.

The two-segment comparison is made on the single layer recorded for it (512 -> 512 1x1 at 16 x 48 x 48, the smallest launch the
cost tables cut; fixture source "layer").  The other two-segment entries, taken from the batch-32 plans, are checked for their
route only: two of them -- the single-output ReLU 128 -> 256 3x3 launch at 32 x 48 x 48 in bf16 and f16 -- differ from the
single launch in the SIGN OF ZEROS (8 298 328 / 8 298 165 differing bytes of 37.7 M, max |difference| 0.0; the 256 x 256 and the
192 x 128 tile end in different epilogues), measured alike on the library from before the route and on this one: a property of
the kernels, which the dispatch does not touch."""
import ctypes as C

import pytest
import torch

from conv_route_cases import load as load_fixture
from pytorch_pose_proposal_network_amd import lib as L

pytestmark = pytest.mark.gpu

FIELDS, ENTRIES = load_fixture()
F = {n: i for i, n in enumerate(FIELDS)}
POINTERS = [n for n, t in L.ConvDesc._fields_ if t is C.c_void_p]


def _class(e):
    """What instantiation an accepted entry reaches: kernel kind, element type, template flags, epilogue flags, split."""
    d = e["d"]
    name = e["kernel"]
    kind, targs = name.split("<")[0], name[name.index("<") + 1:-1].split(", ")
    flags = tuple(targs[4:]) if kind == "conv_igemm_big_kernel" else (targs[-1],) if kind == "conv_igemm_kernel" else ()
    two = e["k"][0] == 2 and e["cut"] > 0 and d[F["m_count"]] == 0 and d[F["stats_mode"]] == 0 and kind == "conv_igemm_big_kernel"
    return (kind, d[F["dtype"]], flags, e["strip"], d[F["stats_mode"]], bool(e["stats_tiles"]), d[F["flags"]] & (4 | 8),
            bool(d[F["residual"]]), bool(d[F["argmax_keys"]]), two)


def _cost(e):
    d = e["d"]
    m = d[F["batch"]] * d[F["out_h"]] * d[F["out_w"]]
    return d[F["batch"]] * d[F["in_h"]] * d[F["in_w"]] * d[F["cin"]] + m * d[F["cout"]] + d[F["splitk_ws_bytes"]] // 4


def _select():
    best = {}
    for e in ENTRIES:
        if e["rc"] == 0 and e["k"][1] == 0:
            c = _class(e)
            if c not in best or _cost(e) < _cost(best[c]):
                best[c] = e
    # + one forced tile per large tile shape (the smallest layer recorded with it)
    for e in ENTRIES:
        if e["rc"] == 0 and e["k"][1] != 0:
            c = ("forced", e["kernel"])
            if c not in best or _cost(e) < _cost(best[c]):
                best[c] = e
    # + the scope of the filter bank kernel with conv64 switched off and with PPN_CONV_NO_FILTER_BANK, per 16-bit type
    for e in ENTRIES:
        d = e["d"]
        if (e["rc"] == 0 and e["k"][:3] == [0, 0, 0] and d[F["dtype"]] in (L.PPN_BF16, L.PPN_F16) and d[F["cin"]] == 64 and
                d[F["cout"]] == 64 and d[F["ksize"]] == 3 and d[F["stride"]] == 1 and (e["k"][3] == 0 or d[F["flags"]] & 1)):
            c = ("conv64 off", d[F["dtype"]], e["k"][3], d[F["flags"]] & 1)
            if c not in best or _cost(e) < _cost(best[c]):
                best[c] = e
    for i, e in enumerate(ENTRIES):                               # + the single layers recorded for the two-segment launch
        if e["s"] == "layer":
            best[("layer", i)] = e
    return sorted(best.values(), key=lambda e: (e["kernel"], _cost(e)))


SELECTED = _select()


def _id(e):
    d = e["d"]
    return "%s-%dx%dx%d-%d-%d-k%d-st%d-f%d-p%d-c%d" % (e["kernel"].replace(" ", ""), d[F["batch"]], d[F["in_h"]], d[F["in_w"]], d[F["cin"]],
                                                     d[F["cout"]], d[F["ksize"]], d[F["stats_mode"]], d[F["flags"]], e["k"][0], e["k"][3])


@pytest.fixture
def knobs():
    lib = L.load()

    def set_(k):
        L.check(lib.ppn_set_conv_tile_policy(k[0]), "policy")
        L.check(lib.ppn_set_conv_tile_override(k[1], k[2]), "override")
        L.check(lib.ppn_set_conv64_enabled(k[3]), "conv64")
        L.check(lib.ppn_set_conv_strip_enabled(k[4]), "strip")
    yield set_
    set_([0, 0, 0, 1, 1])


class Launch:
    """The entry's descriptor over real buffers sized from its fields (random operands, fixed seed)."""

    def __init__(self, e):
        d = dict(zip(FIELDS, e["d"]))
        dev = torch.device("cuda")
        g = torch.Generator(device="cuda").manual_seed(5)
        es = 4 if d["dtype"] == L.PPN_F32 else 2
        tdt = {L.PPN_F32: torch.float32, L.PPN_BF16: torch.bfloat16}.get(d["dtype"], torch.float16)
        m = d["batch"] * d["out_h"] * d["out_w"]
        rnd = lambda n, dt, s: (torch.randn(n, generator=g, device=dev) * s).to(dt)                      # noqa: E731
        vec = lambda s, o=0.0: torch.randn(d["cout_pad"] + 1024, generator=g, device=dev) * s + o        # noqa: E731
        out_bytes = m * d["cout"] * 8 + 4096                      # covers NHWC 16-bit / f32 / PPN_F16X3 pairs and NCHW f32
        self.bufs = {
            "src": rnd(d["batch"] * d["in_h"] * d["in_w"] * d["cin"] * (2 if d["dtype"] == L.PPN_F16X3 else 1), tdt, 0.5),
            "weight": rnd(d["cout_pad"] * d["k_total"], torch.float32 if d["k_total"] == 144 else tdt, 0.05),
            "scale1": vec(0.1, 1.0), "shift1": vec(0.1), "scale2": vec(0.1, 1.0), "shift2": vec(0.1),
            "residual": rnd(m * d["cout"] * 2, tdt, 0.5),
            "out_raw": torch.zeros(out_bytes, dtype=torch.uint8, device=dev),
            "out_act": torch.zeros(out_bytes, dtype=torch.uint8, device=dev),
            "zero_page": torch.zeros(4096, dtype=torch.uint8, device=dev),
            "src2": rnd(max(1, d["batch"] * d["in2_h"] * d["in2_w"] * d["cin2"]), tdt, 0.5),
            "unary_out": torch.zeros(d["batch"] * max(1, d["unary_channels"]) * d["out_h"] * d["out_w"] + 1024, device=dev),
            "argmax_keys": torch.zeros(m * (d["cout"] // max(1, d["limb_window"]) + 1) + 1024, dtype=torch.int64, device=dev),
            "prefetch": torch.zeros(max(128, d["prefetch_bytes"]), dtype=torch.uint8, device=dev),
            "stats_partial": torch.zeros(2 * L.load().ppn_bn_workspace_bytes(d["cout"]) + 4096, dtype=torch.uint8, device=dev),
            "stats_x": rnd(m * d["cout"], tdt, 0.5),
            "stats_gamma": vec(0.1, 1.0), "stats_beta": vec(0.1), "stats_mean": vec(0.1), "stats_rstd": vec(0.05, 1.0).abs(),
            "splitk_ws": torch.zeros(max(16, d["splitk_ws_bytes"]), dtype=torch.uint8, device=dev),
        }
        self.d, self.es = d, es
        self.tiles = C.c_int32(-1)

    def desc(self, **over):
        c = L.ConvDesc()
        for n, v in dict(self.d, **over).items():
            if n in POINTERS:
                setattr(c, n, self.bufs[n].data_ptr() if v else None)
            elif n == "stats_tiles":
                c.stats_tiles = C.pointer(self.tiles) if v else None
            else:
                setattr(c, n, v)
        return c

    def run(self, **over):
        """Launch; returns (kernel name, strip flag, stats tiles or None, bytes of out_raw and out_act)."""
        lib = L.load()
        for n in ("out_raw", "out_act", "argmax_keys", "unary_out"):
            self.bufs[n].zero_()
        self.tiles.value = -1
        c = self.desc(**over)
        L.check(lib.ppn_conv2d_fused(C.byref(c), L.current_stream_ptr()), "ppn_conv2d_fused")
        torch.cuda.synchronize()
        return (lib.ppn_last_conv_kernel().decode(), int(lib.ppn_last_conv_strip()),
                self.tiles.value if c.stats_tiles else None,
                [self.bufs[n].clone().view(torch.uint8) for n in ("out_raw", "out_act", "argmax_keys", "unary_out")])


def test_selection_reaches_every_kind_and_flag():
    classes = {_class(e) for e in SELECTED if e["k"][1] == 0}
    kinds = {c[0] for c in classes}
    assert kinds == {"stem3x3_kernel", "conv64_kernel", "head_limb_argmax_kernel", "conv_igemm_big_kernel", "conv_igemm_kernel",
                     "conv_splitk_partial_kernel"}
    big = [c for c in classes if c[0] == "conv_igemm_big_kernel"]
    assert any(c[2] == ("false",) for c in big) and any(c[2] == ("true",) for c in big)                  # plain, fused shortcut
    assert any(c[2] == ("false", "true") for c in big)                                                   # X3
    assert any(c[2] == ("false", "false", "true") and c[4] == 1 for c in big)                            # stats mode 1
    assert any(c[2] == ("false", "false", "true") and c[4] == 2 for c in big)                            # stats mode 2
    assert any(c[3] for c in big) and any(c[6] & 4 for c in big) and any(c[6] & 8 for c in big)          # strip, OUT_BF16, PLAIN_OUT
    assert any(c[9] for c in big)                                                                        # two-segment split
    gen = [c for c in classes if c[0] == "conv_igemm_kernel"]
    assert any(c[2] == ("true",) for c in gen) and any(c[2] == ("false",) for c in gen)                  # small Cin and not


@pytest.mark.parametrize("e", SELECTED, ids=[_id(e) for e in SELECTED])
def test_launch_matches_the_recorded_route(knobs, e):
    knobs(e["k"])
    run = Launch(e)
    name, strip, tiles, out = run.run()
    assert (name, strip, tiles) == (e["kernel"], e["strip"], e["stats_tiles"])
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))                                     # noqa: E731
    if e["strip"]:
        knobs(e["k"][:4] + [0])
        n2, s2, _, ref = run.run()
        assert (n2, s2) == (name, 0) and same(out, ref), "strip loader changes the output"
    if e["stats_tiles"]:
        n2, _, t2, ref = run.run(stats_mode=0, stats_partial=0, stats_tiles=0)
        assert t2 is None and "false, false, true" not in n2 and same(out, ref), "statistics epilogue changes the output"
    if e["s"] == "layer":
        assert _class(e)[9], "the recorded layer is not cut in two"
        knobs([0] + e["k"][1:])
        _, _, _, ref = run.run()
        assert same(out, ref), "two-segment launch changes the output"
