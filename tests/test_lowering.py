"""CPU: what `lowering.lower` decides for every inference mode -- launch order, per-launch types, tensor storage, block
fusion, the split head, the pixel-range cut and the prefetch chain.  Needs libppn.so for the host-only ppn_conv_tiling /
ppn_conv_split (built on demand, as tests/test_host_cpu.py does); no GPU."""
import os

import pytest

from pytorch_pose_proposal_network_amd import arch as A, config as cfg

N_UNARY, N_EDGES = 6 * len(cfg.KEYPOINT_NAMES), len(cfg.EDGES)


@pytest.fixture(scope="module")
def LW():
    from pytorch_pose_proposal_network_amd import build, lib, lowering
    if not os.path.exists(lib.LIB_PATH):
        build.build(verbose=False)
    return lowering


@pytest.fixture
def cut_convs(LW):
    """Tile policy 2 (opt-in, host state of the library): the launcher cuts some convolutions into two pixel ranges."""
    from pytorch_pose_proposal_network_amd import lib as L
    L.check(L.load().ppn_set_conv_tile_policy(2))
    yield
    L.check(L.load().ppn_set_conv_tile_policy(0))


BF, F16, F32, X3 = (dict(compute_dtype=n) for n in ("bfloat16", "float16", "float32", "float16x3"))
MODES = {"f32": ("drn_d_22", dict(F32, fuse_stem=False)), "f32_stem01": ("drn_d_22", dict(F32, fuse_stem=True)),
         "bf16": ("drn_d_22", BF), "bf16_pure": ("drn_d_22", dict(BF, stem_dtype="bfloat16", half_prefix=-1)),
         "f16": ("drn_d_22", F16), "x3": ("drn_d_22", X3), "x3_stem": ("drn_d_22", dict(X3, fuse_stem="all")),
         "f16_exact3": ("drn_d_22", dict(F16, exact_prefix=3)),
         "f16_exact3_stem": ("drn_d_22", dict(F16, exact_prefix=3, fuse_stem="all")),
         "d54_bf16": ("drn_d_54", BF), "d54_f16_exact4": ("drn_d_54", dict(F16, exact_prefix=4)),
         "d54_f16_exact4_stem": ("drn_d_54", dict(F16, exact_prefix=4, fuse_stem="all"))}


def _lower(LW, mode_id, fused=False, size=(96, 96), batch=2, u8=True, grid=(21, 21), **kw):
    arch, args = MODES[mode_id] if isinstance(mode_id, str) else mode_id
    mode = LW.resolve_mode(**args)
    win = grid[0] * grid[1]
    ops = A.build_program(arch, N_UNARY + win * N_EDGES, fuse_stem=mode.fuse_stem, fuse_shortcut=mode.fuses_shortcut)
    h, w = size
    low = LW.lower(ops, mode, batch, h, w, u8, fused, n_unary=N_UNARY, n_edges=N_EDGES, limb_window=win, **kw)
    return ops, mode, low


def _run_dtype(launch):
    return launch.scalars["dtype"] & 0xff           # the stem's dtype word carries the output type and RAW_S2 above bit 8


# ---- structural invariants, every mode ---------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("size", [(96, 96), (104, 72)])
@pytest.mark.parametrize("mode_id", sorted(MODES))
def test_structural_invariants(LW, mode_id, size, fused):
    _check_invariants(LW, mode_id, size, fused, 2)


@pytest.mark.parametrize("mode_id", ["bf16", "f32", "x3", "f16_exact3_stem"])
def test_structural_invariants_with_cut_convs(LW, mode_id, cut_convs):
    low = _check_invariants(LW, mode_id, (384, 384), True, 32)
    pieces = [l for l in low.launches if "m_count" in l.scalars]
    assert pieces and len(pieces) % 2 == 0
    for a, b in zip(pieces[::2], pieces[1::2]):
        base, n = a.name[:a.name.index("[")], a.scalars["m_count"] + b.scalars["m_count"]
        assert (a.name, b.name) == (f"{base}[0:{a.scalars['m_count']}]", f"{base}[{b.scalars['m_begin']}:{n}]")
        assert (a.tensors, a.params) == (b.tensors, b.params)
        assert a.scalars["m_begin"] == 0 and b.scalars["m_begin"] == a.scalars["m_count"]


def _check_invariants(LW, mode_id, size, fused, batch):
    ops, mode, low = _lower(LW, mode_id, fused, size, batch)
    F32_, BF16_, F16_, X3_ = LW.F32, LW.BF16, LW.F16, LW.X3
    table, launches = low.tensors, low.launches
    written, cover = {"input": -1}, {}
    for i, l in enumerate(launches):
        for name in l.reads:
            assert name in written, f"{l.name} reads {name} before it is written"
        for name in l.writes:
            assert name in table, (l.name, name)
            if l.kind == "memset":                    # not a producer: the fill the atomicMax head conv accumulates onto
                assert name == "keys" and name not in written
                continue
            if "m_count" in l.scalars:                # a pixel-range piece: the pieces of one conv tile its output once
                lo, n = l.scalars["m_begin"], l.scalars["m_count"]
                assert cover.get(name, 0) == lo, f"{l.name}: pieces of {name} do not abut"
                cover[name] = lo + n
                if lo:
                    continue
            assert name not in written, f"{name} written twice ({l.name})"
            written[name] = i
    # ... except the tensors a one-launch block keeps on chip: they keep their table row (the plan has always allocated
    # every tensor of the program by name), and no launch touches them
    names = [o.name for o in ops]
    on_chip = set()
    for l in launches:
        if l.kind == "block":
            first = names.index(l.name.split("+")[0])
            on_chip.update(o.out_raw for o in ops[first:first + l.name.count("+")])
    assert set(written) == set(table) - on_chip and not on_chip & set(written), set(table) ^ set(written)
    for name, end in cover.items():
        (b, th, tw, _), _ = table[name]
        assert end == b * th * tw, name
    # the "#x3" twin comes from a split record directly behind the launch that wrote the f32 tensor
    for name in table:
        if name.endswith("#x3"):
            l = launches[written[name]]
            base = name[:-3]
            assert l.kind == "split" and l.tensors == {"src": base, "dst": name}
            assert table[base][1] == F32_ and table[name][1] == X3_ and table[name][0][-1] == 2 * table[base][0][-1]
            assert l.scalars["channels"] == table[base][0][-1]
            prod = written[base]
            assert all(launches[j].kind == "split" for j in range(prod + 1, written[name])) and written[name] - prod <= 2
    # one storage type per tensor; every reader's and writer's type fits it (the storage comment of tensor_table)
    for l in launches:
        if l.kind in ("split", "memset"):
            continue
        d = _run_dtype(l)
        for name in l.reads:
            st = table[name][1]
            if name == "input":
                assert st in (LW.U8, F32_)
            else:
                assert st == d, f"{l.name} ({d}) reads {name} stored as {st}"      # X3 launches read the #x3 twin of f32
        for f, name in l.tensors.items():
            if f in ("out_raw", "out_act") and name not in ("head", "unary"):
                st = table[name][1]
                flags = l.scalars.get("flags", 0)
                if l.kind == "stem012" and l.scalars["dtype"] >> 8 & 0xff:
                    assert st == (l.scalars["dtype"] >> 8 & 0xff) - 1              # PPN_STEM_IO(internal, out)
                elif d == F16_ and st == BF16_:
                    assert flags & 4, l.name                                        # PPN_CONV_OUT_BF16
                elif d == X3_ and st == F16_:
                    assert flags & 8, l.name                                        # PPN_CONV_X3_PLAIN_OUT
                else:
                    assert st == d and not flags & 12, (l.name, name, st, d)
    assert table["head" if not fused else "unary"][1] == F32_ and ("keys" in table) == fused
    # entries and flops
    assert len(low.entries) == len(launches) and low.entries == [(l.name, l.flops) for l in launches]
    assert sum(f for _, f in low.entries) == low.flops == A.conv_flops(ops, *size) * batch
    shapes = A.tensor_shapes(ops, *size)
    for l in launches:
        if l.kind == "block":
            first = names.index(l.name.split("+")[0])
            n = l.name.count("+") + 1
            assert l.flops == sum(A.op_flops(o, shapes) for o in ops[first:first + n]) * batch
    return low


# ---- the specific lowerings ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode_id", ["bf16", "f16"])
def test_16bit_default_front(LW, mode_id):
    ops, mode, low = _lower(LW, mode_id, size=(104, 72))
    k = [l.kind for l in low.launches]
    assert k[:3] == ["stem012", "block", "block"] and "block" not in k[3:]
    stem, first, pair = low.launches[:3]
    from pytorch_pose_proposal_network_amd import lib as L
    assert stem.scalars["dtype"] & L.PPN_STEM_RAW_S2 and _run_dtype(stem) == L.PPN_F16
    full = A.tensor_shapes(ops, 104, 72)[stem.tensors["out_raw"]]
    assert full[:2] == (52, 36)
    assert low.tensors[stem.tensors["out_raw"]][0] == (2, 26, 18, 32)             # the raw stem tensor at half size
    assert low.tensors[stem.tensors["out_act"]][0] == (2, 52, 36, 32)
    assert first.scalars["stride"] == 2 and first.tensors["proj_src"] == stem.tensors["out_raw"]
    assert first.tensors["src"] == stem.tensors["out_act"] and (first.scalars["in_h"], first.scalars["in_w"]) == (52, 36)
    assert (first.scalars["h"], first.scalars["w"]) == (26, 18) and first.name == "backbone.3.0.downsample+conv1+conv2"
    dt = _run_dtype(first)
    assert (first.scalars["w1_ld"], first.scalars["proj_ld"]) == (L.conv_tiling(dt, 32, 64, 3)[3], L.conv_tiling(dt, 32, 64, 1)[3])
    assert "stride" not in pair.scalars and pair.name == "backbone.3.1.conv1+conv2"
    assert pair.tensors["src"] == first.tensors["out_act"] and pair.tensors["residual"] == first.tensors["out_raw"]
    assert (pair.scalars["h"], pair.scalars["w"]) == (26, 18)


def _without(launches, fields=()):
    return [(l.kind, l.name, l.flops, l.tensors, {k: v for k, v in l.params.items() if k not in fields}, l.scalars)
            for l in launches]


def test_each_knob_changes_only_its_records(LW):
    from pytorch_pose_proposal_network_amd import lib as L
    ops, mode, ref = _lower(LW, "bf16", fused=True, size=(104, 72))
    # PPN_PREFETCH=0: the same records without the prefetch operand
    _, _, off = _lower(LW, "bf16", fused=True, size=(104, 72), prefetch=False)
    assert not any("prefetch" in l.params for l in off.launches) and off.tensors == ref.tensors
    assert _without(off.launches) == _without(ref.launches, ("prefetch",))
    # PPN_STEM_RAW_S2=0: full-size raw stem tensor, no flag, and the first block back as three launches (its one-launch form
    # reads the subsampled tensor); everything from layer3's second block on unchanged
    _, _, off = _lower(LW, "bf16", fused=True, size=(104, 72), raw_s2=False)
    stem = off.launches[0]
    assert not stem.scalars["dtype"] & L.PPN_STEM_RAW_S2 and off.tensors[stem.tensors["out_raw"]][0] == (2, 52, 36, 32)
    assert [l.kind for l in off.launches[:5]] == ["stem012", "conv", "conv", "conv", "block"]
    assert off.launches[1].scalars["stride"] == 2 and (off.launches[1].scalars["in_h"], off.launches[1].scalars["in_w"]) == (52, 36)
    assert _without(off.launches[4:]) == _without(ref.launches[2:])
    assert {k: v for k, v in off.tensors.items() if k != stem.tensors["out_raw"]}.items() <= off.tensors.items()
    # fuse_block=False: five conv launches where the two blocks were; the projection reads the subsampled tensor at stride 1
    _, _, off = _lower(LW, ("drn_d_22", dict(BF, fuse_block=False)), fused=True, size=(104, 72))
    assert [l.kind for l in off.launches[:6]] == ["stem012"] + ["conv"] * 5 and not any(l.kind == "block" for l in off.launches)
    ds = off.launches[1]
    assert ds.scalars["stride"] == 1 and (ds.scalars["in_h"], ds.scalars["in_w"]) == (26, 18)
    assert _without(off.launches[:1]) == _without(ref.launches[:1]) and _without(off.launches[6:]) == _without(ref.launches[3:])
    # PPN_HEAD_EDGE=0: memset + one head conv instead of .unary / .limbs; the conv before it prefetches conv3.w
    _, _, off = _lower(LW, "bf16", fused=True, size=(104, 72), head_edge=False)
    assert [l.name for l in ref.launches[-2:]] == ["conv3.unary", "conv3.limbs"]
    assert [(l.kind, l.name) for l in off.launches[-2:]] == [("memset", "zero arg-max keys"), ("conv", "conv3")]
    assert off.launches[-3].params["prefetch"] == "conv3.w" and ref.launches[-3].params["prefetch"] == "conv3.w_unary"
    assert _without(off.launches[:-3]) == _without(ref.launches[:-3]) and off.tensors == ref.tensors
    assert _without(off.launches[-3:-2], ("prefetch",)) == _without(ref.launches[-3:-2], ("prefetch",))


def test_prefix_boundaries_carry_their_flags(LW):
    from pytorch_pose_proposal_network_amd import lib as L
    for mode_id, dt, flag, prefix in (("bf16", L.PPN_F16, L.PPN_CONV_OUT_BF16, 4), ("d54_bf16", L.PPN_F16, L.PPN_CONV_OUT_BF16, 4),
                                      ("f16_exact3", L.PPN_F16X3, L.PPN_CONV_X3_PLAIN_OUT, 3),
                                      ("f16_exact3_stem", L.PPN_F16X3, L.PPN_CONV_X3_PLAIN_OUT, 3),
                                      ("d54_f16_exact4", L.PPN_F16X3, L.PPN_CONV_X3_PLAIN_OUT, 4)):
        ops, mode, low = _lower(LW, mode_id)
        inside = tuple(f"backbone.{i}." for i in range(prefix + 1))
        convs = [l for l in low.launches if l.kind == "conv"]
        flagged = [l for l in convs if l.scalars["flags"] & flag]
        last = [l for l in low.launches if l.kind not in ("split", "memset") and l.name.startswith(inside)][-1]
        assert flagged == [last] and last.scalars["dtype"] == dt, (mode_id, [l.name for l in flagged])
        after = low.launches[low.launches.index(last) + 1]
        assert after.scalars["dtype"] == mode.compute_dtype and not after.name.startswith(inside)
    for mode_id in ("bf16_pure", "f16", "f32", "x3"):
        assert not any(l.scalars.get("flags", 0) for l in _lower(LW, mode_id)[2].launches)


@pytest.mark.parametrize("mode_id", ["x3_stem", "f16_exact3_stem", "d54_f16_exact4_stem"])
def test_fused_x3_stem_record(LW, mode_id):
    from pytorch_pose_proposal_network_amd import lib as L
    ops, mode, low = _lower(LW, mode_id)
    stem = low.launches[0]
    assert stem.kind == "stem012" and stem.scalars["dtype"] == L.PPN_STEM_X3_F32      # no RAW_S2 bit either
    assert all(low.tensors[n][1] == L.PPN_F32 and low.tensors[n][0][1:3] == (48, 48) for n in stem.writes) and stem.writes
    assert sum(1 for l in low.launches if l.kind.startswith("stem")) == 1
    _, _, base = _lower(LW, mode_id[:-5])                  # the same mode with the stem as three f32 launches
    assert [l.kind for l in base.launches[:3]] == ["stem", "conv", "conv"]
    assert all(l.scalars["dtype"] == L.PPN_F32 for l in base.launches[:3])
    assert _without(low.launches[1:]) == _without(base.launches[3:])


@pytest.mark.parametrize("mode_id", ["bf16", "f16", "f32", "f16_exact3"])
def test_fused_decode_head_with_the_edge_tile(LW, mode_id):
    ops, mode, low = _lower(LW, mode_id, fused=True)
    assert not any(l.kind == "memset" for l in low.launches) and "head" not in low.tensors
    un, li = low.launches[-2:]
    assert (un.name, li.name) == ("conv3.unary", "conv3.limbs") and un.flops + li.flops == A.op_flops(ops[-1], A.tensor_shapes(ops, 96, 96)) * 2
    assert un.tensors == {"src": li.tensors["src"], "out_raw": "unary"} and li.tensors["argmax_keys"] == "keys"
    assert un.params["weight"] == "conv3.w_unary" and un.params["shift1"] == "conv3.b_unary" and un.params["prefetch"] == "conv3.w_edge"
    assert li.params["weight"] == "conv3.w_edge" and li.params["shift1"] == "conv3.b_edge" and "prefetch" not in li.params
    assert un.scalars["cout"] == N_UNARY and li.scalars["cout"] == 441 * N_EDGES
    assert li.scalars["limb_edge_pad"] == 448 and li.scalars["cout_pad"] == 448 * N_EDGES and li.scalars["limb_window"] == 441
    assert low.tensors["unary"] == ((2, N_UNARY, 6, 6), LW.F32) and low.tensors["keys"] == ((2, N_EDGES, 6, 6), LW.I64)


def test_head_edge_pad_takes_windows_433_to_448_only(LW):
    """The edge-aligned tile masks pad rows in its last 16 rows only (csrc/conv_head.hip) and the dispatch refuses every other
    window: the lowering must send exactly the windows 433 .. 448 to it."""
    _, mode, _ = _lower(LW, "bf16", fused=True)
    got = [LW.head_edge_pad(mode, w) for w in (1, 384, 385, 420, 431, 432, 433, 441, 447, 448, 449)]
    assert got == [0, 0, 0, 0, 0, 0, 448, 448, 448, 448, 0]
    assert LW.head_edge_pad(mode, 441, False) == 0


@pytest.mark.parametrize("mode_id,grid", [("bf16", (9, 9)), ("f16", (9, 9)), ("x3", (21, 21)), ("bf16", (23, 23)),
                                          ("bf16", (21, 20)), ("f16", (27, 16)), ("f32", (24, 18))])
def test_fused_decode_head_with_atomic_keys(LW, mode_id, grid):
    """A window outside 433..448 values (and the float16x3 mode): zero fill, then ONE head conv."""
    ops, mode, low = _lower(LW, mode_id, fused=True, grid=grid)
    win = grid[0] * grid[1]
    ms, head = low.launches[-2:]
    assert (ms.kind, ms.tensors, ms.scalars) == ("memset", {"dst": "keys"}, {"bytes": 2 * N_EDGES * 6 * 6 * 8})
    assert head.kind == "conv" and head.name == "conv3" and sum(1 for l in low.launches if l.kind == "memset") == 1
    assert head.tensors["unary_out"] == "unary" and head.tensors["argmax_keys"] == "keys" and "out_raw" not in head.tensors
    assert head.scalars["unary_channels"] == N_UNARY and head.scalars["limb_window"] == win and "limb_edge_pad" not in head.scalars
    assert head.scalars["cout"] == N_UNARY + win * N_EDGES and head.params["weight"] == "conv3.w"


def _first_weight(l):
    return l.params.get("proj_weight") or l.params.get("weight1") or l.params["weight"]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("mode_id", ["bf16", "f32", "x3_stem", "f16_exact3", "d54_bf16"])
def test_prefetch_chain(LW, mode_id, fused, cut_convs):
    """Every conv prefetches the packed weight the NEXT op's launch reads first (a one-launch first block starts with its
    projection; the pieces of a cut conv both point past their own weight); block and stem launches carry no hint, nor does
    the last launch.  With the edge-aligned head the unary launch prefetches .w_edge and its predecessor .w_unary."""
    _, _, low = _lower(LW, mode_id, fused, size=(384, 384), batch=32)
    heavy = [l for l in low.launches if l.kind in ("conv", "block")]
    assert any("m_count" in l.scalars for l in heavy)
    for i, l in enumerate(heavy):
        nxt = [n for n in heavy[i + 1:] if _first_weight(n) != _first_weight(l)]
        if l.kind == "block" or not nxt:
            assert "prefetch" not in l.params, l.name
        else:
            assert l.params["prefetch"] == _first_weight(nxt[0]), l.name
    assert all("prefetch" not in l.params for l in low.launches if l.kind not in ("conv",))


# ---- launch counts of the parent commit, recorded at the C ABI (drn_d_22 / drn_d_54, batch 2, 384 x 384) ------------------
@pytest.mark.parametrize("mode_id,u8,fused,n", [
    ("bf16", True, True, 29), ("bf16", True, False, 28), ("f32", False, False, 33), ("f32_stem01", True, False, 32),
    ("f16", True, True, 29), ("x3", True, False, 37), ("x3_stem", True, False, 35), ("d54_f16_exact4_stem", True, True, 68)])
def test_launch_counts(LW, mode_id, u8, fused, n):
    _, _, low = _lower(LW, mode_id, fused, size=(384, 384), u8=u8)
    assert len(low.launches) == n
    assert low.tensors["input"] == (((2, 384, 384, 3), LW.U8) if u8 else ((2, 3, 384, 384), LW.F32))


# ---- mode resolution ----------------------------------------------------------------------------------------------
def test_resolve_mode_reads_the_environment_it_is_given(LW):
    from pytorch_pose_proposal_network_amd import lib as L
    m = LW.resolve_mode("bfloat16", env={})
    assert (m.compute_dtype, m.stem_dtype, m.half_prefix, m.exact_prefix, m.fuse_stem, m.fuse_shortcut, m.fuse_block) == \
        (L.PPN_BF16, L.PPN_F16, 4, -1, "all", True, True)
    assert m.half_names == tuple(f"backbone.{i}." for i in range(5)) and m.exact_names == ()
    m = LW.resolve_mode("bfloat16", env={"PPN_BLOCK64": "0", "PPN_STEM_DTYPE": "bfloat16", "PPN_FUSE_SHORTCUT": "0"})
    assert (m.stem_dtype, m.half_prefix, m.fuse_shortcut, m.fuse_block) == (L.PPN_BF16, -1, False, False)
    assert LW.resolve_mode("bfloat16", env={"PPN_BF16_HALF_PREFIX": "-1"}).half_names == ()
    m = LW.resolve_mode("bfloat16", env={"PPN_FUSE_STEM": "0"})
    assert m.fuse_stem is False and m.half_prefix == -1           # the half prefix starts with the fused stem's outputs
    m = LW.resolve_mode("float16", exact_prefix=3, env={})
    assert m.fuse_shortcut is True and m.fuse_stem is False       # data, not a closure: the prefix is excluded by the predicate
    assert not m.fuses_shortcut("backbone.3.0") and m.fuses_shortcut("backbone.4.0")
    assert LW.resolve_mode("float16x3", env={"PPN_FUSE_SHORTCUT": "1"}).fuse_shortcut is False
    for bad in (dict(compute_dtype="float16", stem_dtype="bfloat16"), dict(compute_dtype="bfloat16", exact_prefix=3),
                dict(compute_dtype="float16", exact_prefix=2), dict(compute_dtype="float16", exact_prefix=3, fuse_stem="some"),
                dict(compute_dtype="float16", fuse_stem=False), dict(compute_dtype="float32", fuse_stem="all"),
                dict(compute_dtype="float16x3", fuse_stem=True), dict(compute_dtype="float16x3", fuse_shortcut=True),
                dict(compute_dtype="bfloat16", stem_dtype="bfloat16", half_prefix=4)):
        with pytest.raises(ValueError):
            LW.resolve_mode(env={}, **bad)
