"""Build libppn.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

    python -m pytorch_pose_proposal_network_amd.build [--force]

The shared library lands next to the sources (csrc/libppn.so) so that it travels with the
repo snapshot to the GPU box; it is git-ignored.
"""
from __future__ import annotations

import os
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB = os.path.join(CSRC, "libppn.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
COMMON = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]
# NOSLP: every kernel that runs MFMAs is compiled WITHOUT SLP vectorisation (round 5).  hipcc packs adjacent f32 adds / FMAs of an
# epilogue into v_pk_add_f32 / v_pk_fma_f32 (... op_sel:[0,1] op_sel_hi:[1,0]) right behind the VALU instructions that write
# their operands; in csrc/block64.hip's bf16 instantiation -- two waves per SIMD, the partner wave issuing MFMAs -- lanes 48-63
# then sporadically added a stale operand: the last channel of a lane's four lost its residual in ~25 % of the first tiles
# (tools/diag_block64.py, profiles/r05/block64_pk_add_hazard.txt; scalar v_add_f32: never).  conv_big.hip alone held 2 880
# v_pk_add_f32 and 276 op_sel forms.  Same arithmetic, same bits; same-box A/B of the whole library: three lanes 10.89 / 10.89 k
# vs 10.90 / 10.92 k images/s, one lane 10.64 / 10.66 vs 10.66 / 10.70 k, training step 18.36 / 18.39 vs 18.42 / 18.39 ms
# (profiles/r05/ab_noslp.txt) -- and MI355X_MICROARCH.md prices packed f32 VALU beside MFMAs at +22-26 cycles per gap anyway.
NOSLP = ["-fno-slp-vectorize"]
# (source, extra flags).  decode.hip must not contract a*b+c: the IoU / threshold tests are knife edges.
SOURCES = [
    ("abi.cpp", ["-x", "hip"]),
    ("decode.hip", ["-ffp-contract=off"]),
    ("conv_route.cpp", []),   # host-only: which kernel a conv descriptor runs on
    ("conv.hip", NOSLP),
    ("conv_big.hip", NOSLP),
    ("conv_splitk.hip", NOSLP),
    ("conv_head.hip", NOSLP),
    ("conv64.hip", NOSLP),
    ("block64.hip", NOSLP),
    ("stem.hip", NOSLP),
    ("stem3x3.hip", NOSLP),
    ("stem01.hip", NOSLP),
    ("stem012.hip", NOSLP),
    ("stem012_x3.hip", NOSLP),
    ("plan.hip", []),
    ("loss.hip", []),
    ("train.hip", []),
    ("encode.hip", ["-ffp-contract=off"]),
    ("wgrad.hip", NOSLP),
    ("stem_wgrad.hip", NOSLP),
    ("ingest.hip", ["-ffp-contract=off"]),
    # augment.hip is bit-exact with a NumPy restatement: no contraction, and the normalisation's f32 divide IEEE-rounded
    ("augment.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),
    # render.hip is bit-exact with PIL's scan-line fill: x = (y - y0) * slope + x0 uncontracted, the slope's divide IEEE-rounded
    ("render.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),
    # validate.hip is bit-exact with NumPy's f32 distance at the PCKh threshold: dx*dx + dy*dy uncontracted, IEEE sqrt and divide
    ("validate.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),
    # tta.hip is bit-exact with NumPy's (a + b) * 0.5 in f32: the add and the multiply stay two IEEE operations
    ("tta.hip", ["-ffp-contract=off"]),
    # track.hip is bit-exact with a NumPy restatement at the IoU and keypoint-gate thresholds: dx*dx + dy*dy and
    # old + alpha * (new - old) uncontracted, the IoU's divide IEEE-rounded
    ("track.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),
    # windows.hip is bit-exact with a NumPy restatement at the merge threshold and in the mapped boxes: y * sy + y0
    # uncontracted, the scales' and the IoU's divides IEEE-rounded
    ("windows.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),
    # crops.hip is bit-exact with a NumPy restatement in the rectangles it writes: hh + hh * margin uncontracted, the
    # aspect's divide IEEE-rounded
    ("crops.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),
    # redact.hip is bit-exact with a NumPy restatement in the cells a person covers: crops.hip's hh + hh * margin, uncontracted
    # (no MFMA code, hence no NOSLP)
    ("redact.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),
    # clips.hip is bit-exact with a NumPy restatement in the normalised clips: (x - cx) / s as one subtraction and one
    # IEEE-rounded divide
    ("clips.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),
    # zones.hip is bit-exact with a NumPy restatement at the zone and line boundaries: the edge interpolation of the polygon
    # test, (xj - xi) * (ay - yi) / (yj - yi) + xi, uncontracted with an IEEE-rounded divide, and the two cross products
    # (the side of a line, the segment test) as two products and one subtraction
    ("zones.hip", ["-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt"]),
    # reid.hip has no float arithmetic at all (integer histograms and their intersection): nothing to contract or to round,
    # and no MFMA code, hence no NOSLP
    ("reid.hip", []),
    # stgcn.hip runs f32 MFMAs: NOSLP like the convolutions; its results are held to derived bounds, not to bytes
    ("stgcn.hip", NOSLP),
    # stgcn16.hip runs f16 MFMAs on half storage: NOSLP; held to derived bounds, and to bytes on exactly representable operands
    ("stgcn16.hip", NOSLP),
]


def torch_lib_dir():
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return None
    d = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    return d if os.path.exists(os.path.join(d, "libamdhip64.so")) else None


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force: bool = False, verbose: bool = True) -> str:
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hpp"))]
    headers.append(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "ppn.h"))
    objs = []
    procs = []
    for src, extra in SOURCES:
        path = os.path.join(CSRC, src)
        if not os.path.exists(path):
            continue
        obj = os.path.join(CSRC, os.path.splitext(src)[0] + ".o")
        objs.append(obj)
        if force or _stale(obj, [path] + headers):
            cmd = [HIPCC] + COMMON + extra + ["-c", path, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
    if force or procs or _stale(LIB, objs):
        # Link against the HIP runtime PyTorch-ROCm bundles (torch/lib/libamdhip64.so) so that the process
        # holds ONE runtime: streams, events and allocations are then shared with torch by construction.
        tl = torch_lib_dir()
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if tl:
            cmd += ["-L" + tl, "-Wl,-rpath," + tl]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
