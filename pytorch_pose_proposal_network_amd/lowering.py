"""From the constructor arguments of ``PoseProposalNet`` to the ordered launches of one inference plan -- as data.

``arch.build_program`` restates the network as fused convolutions; this module decides everything between that list and
the ``ppn_plan_add_*`` calls: the inference mode (``resolve_mode``), the type every launch runs in (``op_dtype``), the type
and shape every tensor is stored in (``tensor_table``), which BasicBlocks run as one launch (``block64_pair`` /
``block64_first``) and the launches themselves (``lower``), operands BY NAME.  ``model.PoseProposalNet._build_plan``
allocates one buffer per table row and turns each ``Launch`` into one call.

No device, no pointers, no descriptors: the only calls into libppn.so are the host-only ``ppn_conv_tiling`` and
``ppn_conv_split``, so every decision here is testable without a GPU (tests/test_lowering.py).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

from . import arch as A
from . import lib as L

F32, BF16, F16, X3 = L.PPN_F32, L.PPN_BF16, L.PPN_F16, L.PPN_F16X3
U8, I64 = "u8", "i64"                  # storage types of the input frames and the arg-max keys (no launch runs in them)
_DTYPES = {"float32": F32, "fp32": F32, "bfloat16": BF16, "bf16": BF16, "float16": F16, "fp16": F16, "f16": F16,
           "float16x3": X3, "f16x3": X3}
OUTPUTS = ("out_raw", "out_act", "unary_out", "argmax_keys", "dst")    # Launch.tensors fields a launch WRITES


# ---- mode resolution ---------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Mode:
    """What the constructor arguments and the environment resolve to (``resolve_mode``)."""
    compute_dtype: int
    stem_dtype: Optional[int]          # type the fused 16-bit stem (csrc/stem012.hip) computes in
    half_prefix: int                   # bf16 mode: backbone.0 .. backbone.{half_prefix} run in IEEE half (>= 3, else off)
    exact_prefix: int                  # float16 mode: backbone.0 .. backbone.{exact_prefix} run as in float16x3 (>= 3, else off)
    fuse_stem: object                  # False | True (csrc/stem01.hip) | "all" (csrc/stem012.hip, csrc/stem012_x3.hip)
    fuse_shortcut: object              # projection shortcuts as GEMM depth of conv2 (never inside an exact prefix)
    fuse_block: bool                   # 64-channel BasicBlocks as one launch (csrc/block64.hip)

    @property
    def half_names(self) -> Tuple[str, ...]:
        return tuple(f"backbone.{i}." for i in range(self.half_prefix + 1)) if self.half_prefix >= 3 else ()

    @property
    def exact_names(self) -> Tuple[str, ...]:
        return tuple(f"backbone.{i}." for i in range(self.exact_prefix + 1)) if self.exact_prefix >= 3 else ()

    def fuses_shortcut(self, prefix: str) -> bool:
        """arch.build_program's predicate of a unit's prefix."""
        if callable(self.fuse_shortcut):
            return self.fuse_shortcut(prefix)
        return bool(self.fuse_shortcut) and not (prefix + ".").startswith(self.exact_names)


def resolve_mode(compute_dtype: str = "float32", fuse_stem=None, fuse_shortcut=None, stem_dtype: Optional[str] = None,
                 half_prefix: Optional[int] = None, exact_prefix: int = -1, fuse_block: Optional[bool] = None,
                 env=os.environ) -> Mode:
    """The inference mode of these ``PoseProposalNet`` arguments; an argument left None takes its environment knob
    (PPN_BLOCK64, PPN_STEM_DTYPE, PPN_BF16_HALF_PREFIX, PPN_FUSE_STEM, PPN_FUSE_SHORTCUT) or the mode's default."""
    cdt = _DTYPES[compute_dtype]
    sixteen = cdt in (BF16, F16)
    # 64-channel stride-1 BasicBlocks (layer3 behind its first block) as one launch each (csrc/block64.hip; PPN_BLOCK64=0 /
    # fuse_block=False keep the two launches; results are bit-identical)
    fuse_block = (env.get("PPN_BLOCK64", "1") != "0") if fuse_block is None else bool(fuse_block)
    # Type the FUSED stem (csrc/stem012.hip, 16-bit modes) computes in: its MFMA operands and on-chip tensors; its two
    # output tensors are always stored in the trunk's type.  The bf16 mode defaults to IEEE half (round 4): the stem
    # is 1.8 % of the FLOPs, but its rounding noise passes through every layer behind it -- half internals take the
    # bf16 pipeline from 95 to ~150 of the reference's 260 people at the same speed (PPN_STEM_DTYPE=bfloat16 / the
    # argument restore the all-bf16 stem).
    sdt = {None: None, "float16": F16, "fp16": F16, "f16": F16, "bfloat16": BF16, "bf16": BF16}[
        stem_dtype or (env.get("PPN_STEM_DTYPE") if cdt == BF16 else None) or ("float16" if sixteen else None)]
    if cdt == F16 and sdt == BF16:
        raise ValueError("the float16 mode has no bfloat16 stem")
    # bf16 mode, round 4: the launches of backbone.0 .. backbone.{half_prefix} (default 4: stem + layer3 + layer4 = 6.9 % of
    # DRN-D-22's FLOPs) run in IEEE half -- the same kernels at the same rate -- and the last of them stores its outputs
    # as bf16 (PPN_CONV_OUT_BF16).  Rounding noise injected in the first layers is amplified by every layer behind
    # them: with this prefix the bf16 pipeline reproduces ~200 instead of 95 of the reference's 260 people
    # (tests/precision_study_mixed.py; measured numbers in DESIGN.md section 2).  half_prefix=-1 / PPN_BF16_HALF_PREFIX=-1:
    # pure bf16 (with stem_dtype="bfloat16": the round-3 behaviour).
    explicit = half_prefix is not None
    if not explicit:
        half_prefix = int(env.get("PPN_BF16_HALF_PREFIX", "4"))
    if cdt != BF16:
        half_prefix = -1
    if half_prefix >= 3 and sdt == BF16:
        if explicit:
            raise ValueError("half_prefix >= 3 needs the IEEE-half stem (stem_dtype='float16')")
        half_prefix = -1                                       # an all-bf16 stem was asked for: pure bf16
    # float16 mode with an EXACT prefix (round 4): the launches of backbone.0 .. backbone.{exact_prefix} run as in the
    # float16x3 mode (f32 where cin < 64, split-f16 elsewhere) and the last of them stores plain half for the f16 trunk
    # (PPN_CONV_X3_PLAIN_OUT).  exact_prefix=3 (stem + layer3, 4.3 % of the FLOPs): 251 of the reference's 260 people
    # where the plain f16 mode reproduces 233 (emulated: tests/precision_study_mixed.py).
    if exact_prefix >= 0 and (cdt != F16 or exact_prefix < 3):
        raise ValueError("exact_prefix is an option of the float16 mode and covers at least backbone.0 .. backbone.3")
    if cdt != F16:
        exact_prefix = -1
    exact = exact_prefix >= 3
    if exact:
        # the stem as f32 launches (fuse_stem False / True), or as ONE split-f16 launch (fuse_stem="all":
        # csrc/stem012_x3.hip, the float16x3 convolutions' error model, f32 outputs)
        if fuse_stem not in (None, False, True, "all"):
            raise ValueError("an exact prefix runs the stem as f32 launches (fuse_stem False / True) or as the "
                             "split-f16 fused stem (fuse_stem='all')")
        fuse_stem = "all" if fuse_stem == "all" else bool(fuse_stem)
    if fuse_stem is None:
        # bf16 mode: the three stem layers share one launch (csrc/stem012.hip; PPN_FUSE_STEM=0 keeps them apart);
        # the exact-f32 parity mode runs them layer by layer
        fuse_stem = "all" if (cdt == F16 or (cdt == BF16 and env.get("PPN_FUSE_STEM", "1") != "0")) else False
    if cdt == X3:
        # split-f16 mode: the layers with cin < 64 (stem, first block's stride-2 convs) run as exact f32, launch by
        # launch -- or, with fuse_stem="all", the stem as one split-f16 launch (csrc/stem012_x3.hip); the split kernel
        # has no fused-shortcut instantiation
        if (fuse_stem and fuse_stem != "all") or fuse_shortcut:
            raise ValueError("the float16x3 mode runs the stem layer by layer (or fused: fuse_stem='all') and without "
                             "fused shortcuts")
        fuse_stem, fuse_shortcut = ("all" if fuse_stem == "all" else False), False
    if fuse_stem == "all" and cdt == F32:
        raise ValueError("fuse_stem='all' (csrc/stem012.hip) is a 16-bit-mode kernel; the float32 mode stays exact f32")
    if cdt == F16 and fuse_stem != "all" and not exact:
        raise ValueError("the float16 mode runs the stem through csrc/stem012.hip only (fuse_stem='all')")
    if fuse_stem != "all":                                     # the half prefix starts with the fused stem's half outputs
        half_prefix = -1
    if fuse_shortcut is None:                                  # tuning knob: PPN_FUSE_SHORTCUT=0 keeps the 1x1 shortcuts apart
        fuse_shortcut = env.get("PPN_FUSE_SHORTCUT", "1") != "0"
    return Mode(cdt, sdt, half_prefix, exact_prefix, fuse_stem, fuse_shortcut, fuse_block)


# ---- per-launch dtype --------------------------------------------------------------------------------------------
def op_dtype(mode: Mode, op: A.ConvOp) -> int:
    """The dtype a launch runs in: the model's, except that the bf16 mode's half prefix runs in IEEE half and the exact
    launches (float16x3 mode, a float16 mode's exact prefix) run as split-f16 where that kernel covers them and as exact
    f32 where it does not (cin not a multiple of 64: the unfused stem and the first block's stride-2 convs)."""
    if mode.compute_dtype == BF16:
        return F16 if (mode.half_names and op.name.startswith(mode.half_names)) else BF16
    if not (mode.compute_dtype == X3 or (mode.exact_names and op.name.startswith(mode.exact_names))):
        return mode.compute_dtype
    if op.k == 7:
        return X3 if op.next_s2 is not None else F32          # fuse_stem="all": csrc/stem012_x3.hip
    return X3 if (op.cin % 64 == 0 and op.cout >= 64) else F32


def is_x3_stem(mode: Mode, op: A.ConvOp) -> bool:
    """The fused stem of an exact mode (fuse_stem="all" with float16x3 or an exact prefix): one split-f16 launch
    (csrc/stem012_x3.hip) that runs as PPN_F16X3 but STORES f32, like the three exact-f32 launches it replaces."""
    return op.k == 7 and op.next_s2 is not None and op_dtype(mode, op) == X3


def out_dtype(mode: Mode, op: A.ConvOp) -> int:
    """The dtype a launch writes as: the one it runs in, but f32 from the split-f16 stem."""
    return F32 if is_x3_stem(mode, op) else op_dtype(mode, op)


# ---- packed-weight geometry --------------------------------------------------------------------------------------
def weight_geometry(dtype: int, op: A.ConvOp):
    """(k_step, k_order, k_main, k_total, cout_pad) of the packed weight ``<op.name>.w`` of a launch of ``dtype``: rows of
    k_total = the convolution's own k_main (three half copies in split-f16) + a fused projection shortcut's channels."""
    kstep, _, korder, kmain, cpad = L.conv_tiling(dtype, op.cin, op.cout, op.k)
    if dtype == X3:
        return kstep, korder, kmain, 3 * kmain, cpad
    return kstep, korder, kmain, kmain + (op.ds_cin if op.ds_src else 0), cpad


def head_edge_pad(mode: Mode, limb_window: int, enabled: bool = True) -> int:
    """Rows per edge of the edge-aligned limb tile (448) when the limb window is one it decides correctly (433..448 values,
    e.g. the reference's 21 x 21: the kernel masks the pad rows of an edge's tile in its last 16 rows only, and the dispatch
    refuses every other window), else 0: the chunked epilogue with atomicMax keys.  enabled=False forces the latter."""
    if not enabled or not (432 < limb_window <= 448) or mode.compute_dtype == X3:
        return 0
    return 448 if L.conv_tiling(mode.compute_dtype, 512, 512, 1)[2] == 1 else 0


# ---- tensor storage ----------------------------------------------------------------------------------------------
def _n_readers(ops, name) -> int:
    return sum(1 for o in ops if name in (o.src, o.residual, o.ds_src))


def tensor_table(ops: List[A.ConvOp], mode: Mode, batch: int, h: int, w: int, src_is_u8: bool = True,
                 raw_s2: bool = True):
    """({tensor name: (shape, storage type)}, tensors that need a half-pair "#x3" twin, the subsampled raw stem tensor).

    f32 launches write f32 (plus a half-PAIR copy made by a split launch where a float16x3 launch reads it); float16x3
    launches write half pairs, or plain half when only float16 launches read the tensor (the last launch of an exact
    prefix); float16 launches write half, or bf16 when only bf16 launches read it (the last launch of the bf16 mode's
    half prefix).  A tensor is read by launches of ONE type (f32 + split excepted)."""
    producer = {n: out_dtype(mode, op) for op in ops for n in (op.out_raw, op.out_act) if n}
    readers: Dict[str, set] = {}
    for op in ops:
        for name in (op.src, op.residual, op.ds_src):
            if name and name != "input":
                readers.setdefault(name, set()).add(op_dtype(mode, op))
    store, need_split = {}, set()
    for name, p_ in producer.items():
        rs = readers.get(name, set())
        if p_ == F32:
            assert rs <= {F32, X3}, f"{name}: an f32 tensor read by {rs}"
            store[name] = F32
            if X3 in rs:
                need_split.add(name)
        elif p_ == X3:
            if rs and rs <= {F16}:
                store[name] = F16                              # PPN_CONV_X3_PLAIN_OUT
            else:
                assert rs <= {X3}, f"{name}: a half-pair tensor read by {rs}"
                store[name] = X3
        elif p_ == F16:
            if rs == {BF16}:
                store[name] = BF16                             # PPN_CONV_OUT_BF16
            else:
                assert rs <= {F16}, f"{name}: a half tensor read by {rs}"
                store[name] = F16
        else:
            assert rs <= {BF16}, f"{name}: a bf16 tensor read by {rs}"
            store[name] = BF16
    # round 5: when the fused stem's RAW output is read by nothing but the first BasicBlock's 1x1 stride-2 projection
    # (drn.py:53-54), the stem writes only the pixels that projection reads (even row and column: PPN_STEM_RAW_S2) and the
    # projection runs at stride 1 over the dense quarter-size tensor -- same values, 19 instead of 75 MB written and read
    s2_tensor, stem = None, ops[0]
    if stem.k == 7 and stem.next_s2 is not None and stem.out_raw and raw_s2:
        rd = [o for o in ops if stem.out_raw in (o.src, o.residual, o.ds_src)]
        if (len(rd) == 1 and rd[0].src == stem.out_raw and rd[0].k == 1 and rd[0].stride == 2 and rd[0].pad == 0 and
                not rd[0].ds_src and store[stem.out_raw] in (BF16, F16)):
            s2_tensor = stem.out_raw
    table = {"input": ((batch, h, w, 3), U8) if src_is_u8 else ((batch, 3, h, w), F32)}
    for name, (th, tw, tc) in A.tensor_shapes(ops, h, w).items():
        if name == "input":
            continue
        if name == s2_tensor:
            th, tw = (th + 1) // 2, (tw + 1) // 2
        if name == "head":
            table[name] = ((batch, tc, th, tw), F32)           # the reference's NCHW f32
        elif store[name] == X3:
            table[name] = ((batch, th, tw, 2 * tc), X3)        # [hi(C) | lo'(C)]
        else:
            table[name] = ((batch, th, tw, tc), store[name])
            if name in need_split:
                table[name + "#x3"] = ((batch, th, tw, 2 * tc), X3)
    return table, need_split, s2_tensor


# ---- one-launch BasicBlocks (csrc/block64.hip) -------------------------------------------------------------------
def _plain64(c: A.ConvOp, dtype: int) -> bool:
    return (c.cin == 64 and c.cout == 64 and c.k == 3 and c.stride == 1 and c.dilation == 1 and c.pad == 1 and
            not c.ds_src and not c.nchw_f32_out and weight_geometry(dtype, c)[3:] == (576, 64))


def _block_tail_ok(mode, c1, c2, dtype, table) -> bool:
    outs = [table[n][1] for n in (c2.out_raw, c2.out_act) if n]
    return bool(outs) and all(o == dtype for o in outs) and all(a in (A.ACT_NONE, A.ACT_RELU, A.ACT_LRELU)
                                                                for a in (c1.act1, c2.act1, c2.act2))


def block64_pair(ops, oi: int, mode: Mode, table) -> bool:
    """Do ops oi, oi + 1 form a 64-channel stride-1 BasicBlock that csrc/block64.hip runs as one launch?  (16-bit modes;
    conv1 64 -> 64 3x3 -> bn2 -> ReLU -> conv2 64 -> 64 3x3 (+ x) with the mid tensor read by conv2 alone.)"""
    if not mode.fuse_block or oi + 1 >= len(ops):
        return False
    c1, c2 = ops[oi], ops[oi + 1]
    odt = op_dtype(mode, c1)
    if odt not in (BF16, F16) or op_dtype(mode, c2) != odt:
        return False
    if not (_plain64(c1, odt) and c1.next3x3 is None and _plain64(c2, odt) and c2.next3x3 is None):
        return False
    if not (c1.out_raw and c2.src == c1.out_raw and not c1.out_act and not c1.residual and c1.bias is None):
        return False
    return _n_readers(ops, c1.out_raw) == 1 and _block_tail_ok(mode, c1, c2, odt, table)


def block64_first(ops, oi: int, mode: Mode, table, s2_tensor) -> bool:
    """Do ops oi .. oi + 2 form layer3's first block -- 1x1 stride-2 projection of the (subsampled) raw stem output, conv1 3x3
    stride 2 from 32 channels, conv2 64 -> 64 + the projection -- that csrc/block64.hip runs as one launch?"""
    if not mode.fuse_block or s2_tensor is None or oi + 2 >= len(ops):
        return False
    ds, c1, c2 = ops[oi], ops[oi + 1], ops[oi + 2]
    odt = op_dtype(mode, ds)
    if odt not in (BF16, F16) or op_dtype(mode, c1) != odt or op_dtype(mode, c2) != odt:
        return False
    if not (ds.src == s2_tensor and ds.k == 1 and ds.stride == 2 and ds.cin == 32 and ds.cout == 64 and ds.out_raw and
            not ds.out_act and ds.act1 == A.ACT_NONE and ds.bias is None and not ds.residual):
        return False
    if not (c1.cin == 32 and c1.cout == 64 and c1.k == 3 and c1.stride == 2 and c1.dilation == 1 and c1.pad == 1 and
            c1.out_raw and not c1.out_act and not c1.residual and c1.bias is None and not c1.ds_src and
            c1.src == ops[0].out_act):
        return False
    if not (c2.src == c1.out_raw and c2.residual == ds.out_raw and _plain64(c2, odt)):
        return False
    if _n_readers(ops, ds.out_raw) != 1 or _n_readers(ops, c1.out_raw) != 1:      # read by conv2 alone
        return False
    for c in (ds, c1):                                         # tap-major packed rows [64][k_total]
        _, korder, _, _, cpad = weight_geometry(odt, c)
        if korder != 0 or cpad < 64:
            return False
    return _block_tail_ok(mode, c1, c2, odt, table)


# ---- low-latency plans (csrc/conv_splitk.hip) --------------------------------------------------------------------
LATENCY = os.environ.get("PPN_LATENCY", "0") == "1"     # PPN_LATENCY=1: plans are built with latency=True unless told otherwise
SPLITK_SLAB = 512                      # K values per slab (csrc/splitk_partition.h kSlabElems)
SPLITK_MAX_WORKGROUPS = 64             # an ordinary launch of fewer workgroups fills less than a quarter of the 256 CUs
SPLITK_MAX_BATCH = 4                   # latency plans are the batch 1-4 plans
# Measured (profiles/latency_b1_parent.txt / latency_b1.txt: every in-scope launch under the size test alone, against the parent's launch
# on the same box, batches 1 / 2 / 4; a class stays only if it gains >= 10 % at all three):
#   16-bit modes: the 24 x 24 512-wide 3x3 layers (K = 4608, 50-55 us as one launch) -60 / -52 / -24 %; everything shallower
#     (K <= 2304: 12-24 us launches at 48 x 48 and the neck's 128-wide 3x3) +0 .. +155 % -- two launches and the workspace
#     round trip cost what the idle CUs would have saved.  So: K >= 4608.
#   float32 (MFMA at the vector rate: the same layers take 75-290 us): every candidate -16 .. -83 %, except the 128 -> 256 3x3 at
#     48 x 48 (K = 1152 over 36 ordinary workgroups per image: -0.4 % at batch 4).  So: K >= 1152 and at least 64 K values per
#     ordinary workgroup of one image.
SPLITK_MIN_K = {F32: 1152, BF16: 4608, F16: 4608}
SPLITK_MIN_K_PER_WORKGROUP = 64


def splitk_eligible(launch: "Launch") -> bool:
    """Does a latency plan run this record as a split-K pair of launches?  A pure function of the record.

    Scope of the kernel: a plain NHWC conv launch (no fused shortcut, NCHW head, arg-max, edge tile or pixel range) in
    f32 / bf16 / f16, 3x3 or 1x1, cin a multiple of the K step, channel rows padded to the 64-channel tile.  Worth it: a
    batch of at most SPLITK_MAX_BATCH, so few pixels x channels PER IMAGE that the ordinary launch of one frame -- whose
    smallest tile is 128 pixels x 128 channels (64 below 128 channels) when there are fewer tiles than CUs -- would start
    fewer than SPLITK_MAX_WORKGROUPS workgroups, and a GEMM depth the table above found to pay (SPLITK_MIN_K by dtype,
    SPLITK_MIN_K_PER_WORKGROUP).  The size test looks at one image, not at the batch: the batch 1, 2 and 4 plans of a model
    then split the SAME layers, so image i's head is bit for bit the one it gets alone (a split launch and the one-launch
    kernel sum in different orders).  The block64 / stem / split / head records never qualify."""
    if launch.kind != "conv":
        return False
    s, t = launch.scalars, launch.tensors
    if s["dtype"] not in (F32, BF16, F16) or s["ksize"] not in (1, 3) or s["out_nchw_f32"] or s["batch"] > SPLITK_MAX_BATCH:
        return False
    if any(f in t for f in ("src2", "argmax_keys", "unary_out")) or s.get("limb_edge_pad") or s.get("m_count"):
        return False
    if s["cin"] % (32 if s["dtype"] == F32 else 64) or s["cout"] % 8 or s["cout_pad"] % 64:
        return False
    if s["k_total"] != s["ksize"] ** 2 * s["cin"] or s["k_total"] < max(2 * SPLITK_SLAB, SPLITK_MIN_K[s["dtype"]]):
        return False
    bc = 128 if s["cout"] >= 128 else 64
    workgroups = -(-(s["out_h"] * s["out_w"]) // 128) * -(-s["cout"] // bc)
    return workgroups < SPLITK_MAX_WORKGROUPS and s["k_total"] // workgroups >= SPLITK_MIN_K_PER_WORKGROUP


# ---- launches ----------------------------------------------------------------------------------------------------
@dataclass
class Launch:
    """One ``ppn_plan_add_*`` call with its operands by name.  ``tensors``: descriptor field -> tensor-table row (the
    OUTPUTS fields are written, the others read); ``params``: field -> key of ``PoseProposalNet._dev`` (a key the model
    does not hold is a NULL operand), in argument order for the stem kinds; ``scalars``: the other fields."""
    kind: str                          # stem | stem01 | stem012 | conv | block | split | memset
    name: str                          # display name: the plan's entries, profile_layers
    flops: int
    tensors: Dict[str, str] = field(default_factory=dict)
    params: Dict[str, str] = field(default_factory=dict)
    scalars: Dict[str, int] = field(default_factory=dict)

    @property
    def reads(self) -> List[str]:
        return [t for f, t in self.tensors.items() if f not in OUTPUTS]

    @property
    def writes(self) -> List[str]:
        return [t for f, t in self.tensors.items() if f in OUTPUTS]


@dataclass
class Lowered:
    tensors: Dict[str, tuple]          # name -> (shape, storage type): one buffer each, in allocation order
    launches: List[Launch]
    flops: int

    @property
    def entries(self):
        return [(l.name, l.flops) for l in self.launches]


def _params(op, **fields):
    return {f: f"{op.name}.{suffix}" for f, suffix in fields.items()}


def lower(ops: List[A.ConvOp], mode: Mode, batch: int, h: int, w: int, src_is_u8: bool = True, fused: bool = False,
          conv_flags: int = 0, raw_s2: bool = True, prefetch: bool = True, head_edge: bool = True,
          n_unary: int = 0, n_edges: int = 0, limb_window: int = 0, latency: bool = False) -> Lowered:
    """The plan of one input shape.  fused: the decode front end runs in the head conv (compact ``unary`` + arg-max
    ``keys`` instead of ``head``; the head is n_unary + n_edges * limb_window channels); conv_flags: ppn_conv_desc.flags of
    every conv; raw_s2 / prefetch / head_edge: the plan-time knobs PPN_STEM_RAW_S2 / PPN_PREFETCH / PPN_HEAD_EDGE; latency: the
    records ``splitk_eligible`` picks carry PPN_CONV_SPLIT_K (nothing else changes: same records, tensors and operands)."""
    shapes = A.tensor_shapes(ops, h, w)
    table, need_split, s2_tensor = tensor_table(ops, mode, batch, h, w, src_is_u8, raw_s2)
    if fused:
        # decode front end fused into the head conv: the head tensor is never materialised
        (_, _, th, tw), _ = table.pop("head")
        table["unary"] = ((batch, n_unary, th, tw), F32)
        table["keys"] = ((batch, n_edges, th, tw), I64)
    edge_pad = head_edge_pad(mode, limb_window, head_edge) if fused else 0
    launches: List[Launch] = []

    def rd(name, odt):                                # the buffer a launch of dtype `odt` reads tensor `name` from
        return name + "#x3" if (odt == X3 and table[name][1] == F32 and name != "input") else name

    def outputs(op):
        return {f: n for f, n in (("out_raw", op.out_raw), ("out_act", op.out_act)) if n and n in table}

    def add_splits(op):                               # behind an f32 launch: convert the outputs split launches read
        for name in (op.out_raw, op.out_act):
            if name and name in need_split:
                th_, tw_, tc_ = shapes[name]
                launches.append(Launch("split", f"split({name})", 0, {"src": name, "dst": name + "#x3"},
                                       scalars={"rows": batch * th_ * tw_, "channels": tc_}))

    def block(name, flops, odt, c1, c2, **extra):
        l = Launch("block", name, flops, dict(outputs(c2), src=rd(c1.src, odt)),
                   dict(_params(c1, weight1="w", scale_mid="s1", shift_mid="b1"),
                        **_params(c2, weight2="w", scale1="s1", shift1="b1", scale2="s2", shift2="b2")),
                   dict(dtype=odt, batch=batch, channels=64, act_mid=c1.act1, act1=c2.act1, act2=c2.act2))
        for part, more in extra.items():
            getattr(l, part).update(more)
        launches.append(l)

    oi = 0
    while oi < len(ops):
        op = ops[oi]
        ih, iw, _ = shapes[op.src]
        oh, ow = A.out_hw(op, ih, iw)
        flops = A.op_flops(op, shapes) * batch
        odt = op_dtype(mode, op)
        if block64_first(ops, oi, mode, table, s2_tensor):
            # layer3's FIRST block as one launch (csrc/block64.hip, stride 2): the 1x1 stride-2 projection + BN of the raw
            # stem output (read at the even pixels the stem wrote), conv1 3x3 stride 2 from the pre-activated stem output,
            # bn2 + ReLU, conv2 + shortcut, second output.  Bit-identical to the three launches.
            ds, c1, c2 = ops[oi:oi + 3]
            ih1, iw1, _ = shapes[c1.src]
            oh1, ow1 = A.out_hw(c1, ih1, iw1)
            block(f"{ds.name}+conv1+conv2", sum(A.op_flops(o, shapes) for o in (ds, c1, c2)) * batch, odt, c1, c2,
                  tensors={"proj_src": ds.src}, params=_params(ds, proj_weight="w", proj_scale="s1", proj_shift="b1"),
                  scalars=dict(h=oh1, w=ow1, stride=2, in_h=ih1, in_w=iw1, w1_ld=weight_geometry(odt, c1)[3],
                               proj_ld=weight_geometry(odt, ds)[3]))
            oi += 3
            continue
        if block64_pair(ops, oi, mode, table):
            # a whole 64-channel stride-1 BasicBlock as ONE launch (csrc/block64.hip, round 5): conv1 -> bn2 -> ReLU -> conv2
            # (+ x, second output); the tensor between the convolutions stays in LDS.  Bit-identical to the two launches.
            c2 = ops[oi + 1]
            block(f"{op.name}+conv2", (A.op_flops(op, shapes) + A.op_flops(c2, shapes)) * batch, odt, op, c2,
                  tensors={"residual": rd(c2.residual, odt)} if c2.residual else {}, scalars=dict(h=ih, w=iw))
            oi += 2
            continue
        oi += 1
        if op.k == 7:
            # the stem family: layer 0 alone (csrc/stem.hip), with layer 1 (stem01.hip), with layers 1 and 2 (stem012.hip /
            # stem012_x3.hip); a tensor a split launch reads gets its half-pair twin right behind
            assert op.src == "input"
            sdt, kind, params = odt, "stem", _params(op, weight="w", scale="s1", shift="b1")
            if op.next3x3 is not None:
                kind, params = "stem01", dict(params, **_params(op, weight1="w1", scale1="s1b", shift1="b1b"))
            if op.next_s2 is not None:
                assert mode.compute_dtype in (BF16, F16, X3)
                kind = "stem012"
                params.update(_params(op, weight2="w2", scale2="s1c", shift2="b1c", scale_act="s2", shift_act="b2"))
                out_dt = table[op.out_raw or op.out_act][1]
                if is_x3_stem(mode, op):                      # exact modes: split-f16 internals, f32 outputs
                    assert out_dt == F32 and s2_tensor is None
                    sdt = L.PPN_STEM_X3_F32
                else:
                    sdt = mode.stem_dtype if mode.stem_dtype is not None else mode.compute_dtype
                    if sdt != out_dt:
                        sdt = L.PPN_STEM_IO(sdt, out_dt)
                if s2_tensor is not None:
                    sdt |= L.PPN_STEM_RAW_S2
            else:
                assert op.out_act is None
            launches.append(Launch(kind, op.name, flops, dict(outputs(op), src="input"), params,
                                   dict(dtype=sdt, src_is_u8=int(src_is_u8), batch=batch, h=h, w=w)))
            add_splits(op)
            continue
        kt, cpad = weight_geometry(odt, op)[3:]
        s = dict(dtype=odt, flags=conv_flags, batch=batch, in_h=ih, in_w=iw, cin=op.cin, out_h=oh, out_w=ow, cout=op.cout,
                 ksize=op.k, stride=op.stride, dilation=op.dilation, pad=op.pad, k_total=kt, cout_pad=cpad, act1=op.act1,
                 act2=op.act2, out_nchw_f32=int(op.nchw_f32_out))
        outs = [table[n][1] for n in (op.out_raw, op.out_act) if n and n in table and n != "head"]
        if odt == F16 and outs:
            if all(o == BF16 for o in outs):
                s["flags"] |= L.PPN_CONV_OUT_BF16                                # last launch of the IEEE-half prefix
            else:
                assert all(o == F16 for o in outs), f"{op.name}: outputs of mixed storage types"
        if odt == X3 and outs:
            if all(o == F16 for o in outs):
                s["flags"] |= L.PPN_CONV_X3_PLAIN_OUT                            # last launch of an exact prefix
            else:
                assert all(o == X3 for o in outs), f"{op.name}: outputs of mixed storage types"
        if op.src == s2_tensor:                       # the stem wrote only the pixels this 1x1 stride-2 projection reads
            s.update(in_h=(ih + 1) // 2, in_w=(iw + 1) // 2, stride=1)
        t = {"src": rd(op.src, odt)}
        if op.residual:
            t["residual"] = rd(op.residual, odt)
        if op.ds_src:
            sh2, sw2, sc2 = shapes[op.ds_src]
            t["src2"] = op.ds_src
            s.update(in2_h=sh2, in2_w=sw2, cin2=sc2, stride2=op.ds_stride)
        p = dict(_params(op, weight="w", scale1="s1", shift1="b1"), zero_page="zero")
        # prefetch hint (ppn_conv_desc.prefetch, round 5): every large-tile launch touches the packed weights of the NEXT
        # launch before its epilogue -- a layer's weights were last read a whole pass ago and its first round of workgroups
        # otherwise fetches them from HBM in lockstep (prefetch=False switches the hint off; results do not depend on it)
        if prefetch and oi < len(ops):
            p["prefetch"] = ops[oi].name + (".w_unary" if (ops[oi].nchw_f32_out and edge_pad) else ".w")
        if op.nchw_f32_out and edge_pad:
            # fused decode, limb window fits the edge-aligned tile: the head conv as TWO launches -- (1) the unary
            # channels, an ordinary sigmoid NCHW conv straight into the compact unary tensor; (2) the limb channels, one
            # channel tile per edge: keys are stored, not accumulated -- no zero fill
            ktu, cpu_ = L.conv_tiling(mode.compute_dtype, op.cin, n_unary, 1)[3:]
            pu = dict(p, prefetch=op.name + ".w_edge", **_params(op, weight="w_unary", shift1="b_unary"))
            if not prefetch:
                del pu["prefetch"]
            launches.append(Launch("conv", op.name + ".unary", flops * n_unary // op.cout, dict(t, out_raw="unary"), pu,
                                   dict(s, cout=n_unary, k_total=ktu, cout_pad=cpu_)))
            pe = dict(_params(op, weight="w_edge", scale1="s1", shift1="b_edge"), zero_page="zero")
            launches.append(Launch("conv", op.name + ".limbs", flops - flops * n_unary // op.cout,
                                   dict(t, argmax_keys="keys"), pe,
                                   dict(s, cout=op.cout - n_unary, cout_pad=n_edges * edge_pad, limb_edge_pad=edge_pad,
                                        limb_window=limb_window)))
            continue
        t.update(outputs(op))
        if fused and op.nchw_f32_out:
            # ... any other window: ONE head conv whose epilogue accumulates the keys with atomicMax, behind a zero fill
            (kb, ke, kh, kw_), _ = table["keys"]
            launches.append(Launch("memset", "zero arg-max keys", 0, {"dst": "keys"}, scalars={"bytes": kb * ke * kh * kw_ * 8}))
            t.update(unary_out="unary", argmax_keys="keys")
            s.update(unary_channels=n_unary, limb_window=limb_window)
        p.update(_params(op, scale2="s2", shift2="b2"))
        # two launches with different tiles where the launcher would cut the pixel range (ppn_conv_split): listed as
        # two plan entries so that each launch is timed and named by itself
        m_all, cut = batch * oh * ow, C.c_int64(0)
        L.check(L.load().ppn_conv_split(mode.compute_dtype, op.cin, op.cout, m_all, C.byref(cut)), "ppn_conv_split")
        if cut.value:
            assert not (odt == F32 and need_split & set(t.values())), f"{op.name}: a cut launch with a split behind it"
            for lo, n in ((0, cut.value), (cut.value, m_all - cut.value)):
                launches.append(Launch("conv", f"{op.name}[{lo}:{lo + n}]", flops * n // m_all, dict(t), dict(p),
                                       dict(s, m_begin=lo, m_count=n)))
            continue
        launches.append(Launch("conv", op.name, flops, t, p, s))
        if odt == F32:
            add_splits(op)
    if latency:
        for l in launches:
            if splitk_eligible(l):
                l.scalars["flags"] |= L.PPN_CONV_SPLIT_K
    return Lowered(table, launches, A.conv_flops(ops, h, w) * batch)
