"""CPU: the conv dispatch as data.  csrc/conv_route.cpp is host-only; tools/conv_route_check.cpp drives it as a program of its own,
built with ASan + UBSan, over every entry of tests/golden/conv_routes.json -- the kernel, strip flag, statistics tile count,
two-segment cut and (for rejected descriptors) return code and message that the library recorded BEFORE the dispatch moved into
the route (tools/record_conv_routes.py; the entries with stride < 1, dilation < 1 or pad < 0 are written by hand).  No GPU."""
import os
import shutil
import subprocess

import pytest

from conv_route_cases import load as load_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch_pose_proposal_network_amd", "csrc")
SEG = ("kind", "name", "m_lo", "m_hi", "strip", "stats_tiles", "bp", "bc", "n_ptiles", "n_ctiles")


@pytest.fixture(scope="module")
def routed(tmp_path_factory):
    """(fixture entries, what conv_route says for each): one build, one run."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("route") / "conv_route_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "conv_route_check.cpp"), os.path.join(CSRC, "conv_route.cpp"), "-o", exe],
                   check=True)
    fields, entries = load_fixture()
    assert len(fields) == 53
    text = "".join("NULL\n" if e["d"] is None else " ".join(str(v) for v in e["d"] + e["k"]) + "\n" for e in entries)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PPN_")}
    out = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(entries)
    got = []
    for line in lines:
        p = line.split("\t")
        n = int(p[2])
        assert len(p) == 5 + 10 * n, line
        segs = [dict(zip(SEG, p[4 + 10 * i: 14 + 10 * i])) for i in range(n)]
        for s in segs:
            s.update({k: int(s[k]) for k in SEG[2:]})
        got.append({"rc": int(p[0]), "error": p[1], "n": n, "split": int(p[3]), "segs": segs, "strip": int(p[-1])})
    return fields, entries, got


def test_fixture_covers_every_route_kind():
    _, entries = load_fixture()
    ok = [e for e in entries if e["rc"] == 0]
    names = {e["kernel"].split("<")[0] for e in ok}
    assert names == {"stem3x3_kernel", "conv64_kernel", "head_limb_argmax_kernel", "conv_igemm_big_kernel", "conv_igemm_kernel",
                     "conv_splitk_partial_kernel"}
    assert any(e["strip"] for e in ok) and any(e["stats_tiles"] for e in ok) and any(e["cut"] for e in ok)
    assert sum(e["rc"] != 0 for e in entries) >= 100 and any(e["s"] == "manual" for e in entries)
    # a descriptor in the scope of the filter bank kernel under each of its three switches: on, conv64 off, PPN_CONV_NO_FILTER_BANK
    fields, _ = load_fixture()
    F = {n: i for i, n in enumerate(fields)}
    scope = [e for e in ok if e["d"][F["dtype"]] in (1, 2) and e["d"][F["cin"]] == 64 and e["d"][F["cout"]] == 64 and
             e["d"][F["ksize"]] == 3 and e["d"][F["stride"]] == 1 and e["d"][F["m_count"]] == 0 and e["k"][:3] == [0, 0, 0]]
    for dtype in (1, 2):
        on = [e for e in scope if e["d"][F["dtype"]] == dtype and e["k"][3] == 1 and not e["d"][F["flags"]] & 1]
        off = [e for e in scope if e["d"][F["dtype"]] == dtype and e["k"][3] == 0]
        flag = [e for e in scope if e["d"][F["dtype"]] == dtype and e["k"][3] == 1 and e["d"][F["flags"]] & 1]
        assert any(e["kernel"].startswith("conv64_kernel") for e in on)
        assert off and all(not e["kernel"].startswith("conv64_kernel") for e in off)
        assert flag and all(not e["kernel"].startswith("conv64_kernel") for e in flag)


def test_rejected_descriptors_keep_code_and_message(routed):
    _, entries, got = routed
    n = 0
    for e, g in zip(entries, got):
        if e["rc"] != 0:
            assert (g["rc"], g["error"]) == (e["rc"], e["error"]), (e, g)
            n += 1
        else:
            assert g["rc"] == 0, (e, g)
    assert n >= 100


def test_stride_dilation_pad_are_validated_before_the_division(routed):
    """The one deliberate change: a zeroed stride used to divide by zero in conv_launch."""
    header, entries, got = routed
    manual = [(e, g) for e, g in zip(entries, got) if e["s"] == "manual"]
    assert len(manual) == 5
    for e, g in manual:
        assert g["rc"] == -1 and g["error"] == "bad conv geometry", (e, g)


def test_accepted_descriptors_route_as_recorded(routed):
    fields, entries, got = routed
    F = {n: i for i, n in enumerate(fields)}
    n = 0
    for e, g in zip(entries, got):
        if e["rc"] != 0:
            continue
        n += 1
        d, seg = e["d"], g["segs"]
        assert seg[0]["name"] == e["kernel"], (e, g)                      # ppn_last_conv_kernel: the first segment's
        assert g["strip"] == e["strip"], (e, g)                           # ppn_last_conv_strip
        if d[F["stats_tiles"]]:
            assert g["n"] == 1 and seg[0]["stats_tiles"] == e["stats_tiles"], (e, g)
        else:
            assert e["stats_tiles"] is None and seg[0]["stats_tiles"] == 0
        # the two-segment cut is ppn_conv_split's, and the recorded one under tile policy 2
        m_all = d[F["batch"]] * d[F["out_h"]] * d[F["out_w"]]
        if e["k"][0] == 2 and not d[F["flags"]] & 16:
            assert g["split"] == e["cut"], (e, g)
        else:
            assert e["cut"] == 0 and g["split"] == 0
        if g["n"] == 2:
            assert g["split"] > 0 and (seg[0]["m_lo"], seg[0]["m_hi"], seg[1]["m_lo"], seg[1]["m_hi"]) == (0, g["split"], g["split"], m_all)
        else:
            lo = d[F["m_begin"]] if d[F["m_count"]] else 0
            hi = lo + d[F["m_count"]] if d[F["m_count"]] else m_all
            assert (seg[0]["m_lo"], seg[0]["m_hi"]) == (lo, hi), (e, g)
            # the launcher splits exactly the whole-tensor launches ppn_conv_split cuts (not the statistics or conv64 ones)
            if g["split"] > 0 and seg[0]["kind"] in ("big", "generic"):
                assert d[F["m_count"]] or d[F["stats_mode"]], (e, g)
        for s in seg:
            if s["kind"] in ("big", "generic", "splitk"):
                assert s["n_ptiles"] == -(-(s["m_hi"] - s["m_lo"]) // s["bp"]), (e, g)
                # (PPN_CONV_WAVES=4 aside, bc is the tile the weights' rows are counted in)
                assert s["n_ctiles"] * s["bc"] == d[F["cout_pad"]], (e, g)
    assert n >= 1000
