"""``PoseProposalNet`` with the reference's surface (model.py:51-136) over the HIP conv stack.

    backbone = drn.drn_d_22()                       # spec object, mirrors rt_test.py:56-61
    model = PoseProposalNet(backbone, local_grid_size=(21, 21)).cuda()
    model.load_state_dict(checkpoint['state_dict']) # reference names
    model.eval()
    head = model(image)                             # f32 [B,3,S,S] cuda -> f32 [B,7605,S/16,S/16]

``forward`` launches one fused HIP kernel per convolution through libppn.so (ctypes, C ABI); PyTorch
is used for device memory and streams only.  ``compute_dtype='float32'`` is the exact-f32 MFMA parity
mode (1e-4 on the head), ``'bfloat16'`` the performance mode (bf16 operands, f32 accumulation, f32 head).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import arch as A
from . import config as cfg
from . import lib as L
from . import lowering as LW


class DRNSpec:
    """What ``drn.drn_d_22()`` returns here: the architecture name (there are no nn.Modules to hold)."""

    def __init__(self, arch: str):
        if arch not in A.DRN_D:
            raise ValueError(f"unknown DRN-D variant {arch!r}; have {sorted(A.DRN_D)}")
        self.arch = arch

    def children(self):            # `nn.Sequential(*list(model.children())[:-2])` keeps working
        return [self, None, None]

    def __repr__(self):
        return f"DRNSpec({self.arch})"


def _arch_of(backbone) -> str:
    if isinstance(backbone, str):
        return backbone
    if isinstance(backbone, DRNSpec):
        return backbone.arch
    if isinstance(backbone, (list, tuple)) and backbone and isinstance(backbone[0], DRNSpec):
        return backbone[0].arch
    raise TypeError("backbone must be a DRN-D name or the object returned by drn.drn_d_*()")


class _Plan:
    def __init__(self, handle, buffers, head, entries, flops, input, workspace=None):
        self.handle, self.buffers, self.head, self.flops = handle, buffers, head, flops
        self.workspace = workspace      # the split-K scratch of a latency plan (one per plan, shared by its launches in turn)
        self.entries = entries          # [(name, flops)] aligned with the plan's launches
        self.n_ops = len(entries)
        self.input = input              # plan-owned input buffer: the captured hipGraph never depends on a caller's pointer


class PoseProposalNet:
    def __init__(self, backbone="drn_d_22", insize=(384, 384), outsize=(24, 24),
                 keypoint_names=cfg.KEYPOINT_NAMES, local_grid_size=(21, 21), edges=cfg.EDGES,
                 compute_dtype: str = "float32", fuse_stem=None, fuse_shortcut: Optional[bool] = None,
                 stem_dtype: Optional[str] = None, half_prefix: Optional[int] = None, exact_prefix: int = -1,
                 fuse_block: Optional[bool] = None, latency: Optional[bool] = None):
        self.arch = _arch_of(backbone)
        # low-latency plans (batch 1-4): launches too small to fill the GPU run as split-K pairs (csrc/conv_splitk.hip,
        # lowering.splitk_eligible); None: the PPN_LATENCY knob, off by default
        self.latency = LW.LATENCY if latency is None else bool(latency)
        self.insize = insize
        self.outsize = outsize
        self.keypoint_names = keypoint_names
        self.edges = edges
        self.local_grid_size = local_grid_size
        inW, inH = insize
        outW, outH = outsize
        sW, sH = local_grid_size
        self.gridsize = (int(inW / outW), int(inH / outH))
        self.lastsize = 6 * len(keypoint_names) + sW * sH * len(edges)          # model.py:64
        # everything the arguments and the environment decide about the inference mode: lowering.resolve_mode
        self.mode = mode = LW.resolve_mode(compute_dtype, fuse_stem, fuse_shortcut, stem_dtype, half_prefix, exact_prefix,
                                           fuse_block)
        self.compute_dtype, self.stem_dtype, self.fuse_block = mode.compute_dtype, mode.stem_dtype, mode.fuse_block
        self.half_prefix, self._half_names = mode.half_prefix, mode.half_names
        self.exact_prefix, self._exact_names = mode.exact_prefix, mode.exact_names
        self.training = False
        self.device = torch.device("cuda")
        self._ops: List[A.ConvOp] = A.build_program(self.arch, self.lastsize, fuse_stem=mode.fuse_stem,
                                                    fuse_shortcut=mode.fuses_shortcut)
        self._spec = dict(A.param_spec(self.arch, self.lastsize))
        self._sd: Dict[str, torch.Tensor] = {}
        self._dev: Dict[str, torch.Tensor] = {}      # packed weights / folded BN on the device
        self._plans: Dict[tuple, _Plan] = {}
        self._lib = None
        self._trainer = None                          # trainer.PPNTrainer behind train(): same object, both modes
        self._trainer_dirty = False
        self._mean = (C.c_float * 3)(*cfg.MEAN)
        self._std = (C.c_float * 3)(*cfg.STD)

    # ---- nn.Module-like surface -------------------------------------------------------------
    def cuda(self, device=None):
        self.device = torch.device("cuda" if device is None else device)
        return self

    def eval(self):
        return self.train(False)

    def train(self, mode: bool = True):
        """nn.Module.train(): the SAME object serves both modes, as in main.py:643 / rt_test.py:94.

        mode=True: forward() runs the train-mode network (batch statistics, running statistics updated with momentum
        0.1, activations taped) of ``self.trainer`` -- a trainer.PPNTrainer created on first use from this model's
        state_dict; the training loop then calls ``model.trainer.train_step(x, targets)``.
        mode=False: back to the folded-BN inference plan; parameters and running statistics the trainer changed are
        folded again first."""
        if mode and self.compute_dtype in (L.PPN_F16, L.PPN_F16X3):
            raise RuntimeError("PoseProposalNet.train(): the float16 / float16x3 modes are inference only (train in "
                               "bfloat16 / float32)")
        if mode and not self.training:
            if not self._sd:
                raise RuntimeError("PoseProposalNet.train(): call load_state_dict() first")
            if self._trainer is None:
                from .trainer import PPNTrainer
                self._trainer = PPNTrainer(self.arch, self._sd, compute_dtype=self.compute_dtype, insize=self.insize,
                                           device=self.device)
            self._trainer_dirty = True                # train_step / train-mode forwards change parameters and statistics
        if not mode and self.training and self._trainer is not None and self._trainer_dirty:
            self._trainer_dirty = False
            self.load_state_dict(self._trainer.state_dict(), _from_trainer=True)
        self.training = bool(mode)
        return self

    @property
    def trainer(self):
        """The PPNTrainer behind train mode (None before the first train())."""
        return self._trainer

    def state_dict(self):
        if self._trainer is not None and self._trainer_dirty:        # train mode: the trainer holds the live values
            return {k: v.detach().cpu() for k, v in self._trainer.state_dict().items()}
        return dict(self._sd)

    def load_state_dict(self, state_dict, strict: bool = True, _from_trainer: bool = False):
        """Accepts the reference checkpoint's ``state_dict`` (rt_test.py:74-75); ``module.``-prefixed DDP
        checkpoints are stripped as main.py:311-318 does."""
        sd = {}
        for k, v in state_dict.items():
            if k.startswith("module."):
                k = k[len("module."):]
            t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
            sd[k] = t.detach().cpu()
        missing = [k for k in self._spec if k not in sd]
        unexpected = [k for k in sd if k not in self._spec]
        if strict and (missing or unexpected):
            raise RuntimeError(f"load_state_dict: missing {missing[:5]} ({len(missing)}), "
                               f"unexpected {unexpected[:5]} ({len(unexpected)})")
        for k, shape in self._spec.items():
            if k in sd and tuple(sd[k].shape) != tuple(shape):
                raise RuntimeError(f"load_state_dict: {k} has shape {tuple(sd[k].shape)}, expected {tuple(shape)}")
        self._sd = sd
        self._prepare()
        if self._trainer is not None and not _from_trainer:
            self._trainer.load_state_dict(sd)
        return self

    # ---- weight preparation -------------------------------------------------------------------
    def _fold_bn(self, prefix: str):
        sd = self._sd
        g = sd[prefix + ".weight"].double()
        b = sd[prefix + ".bias"].double()
        m = sd[prefix + ".running_mean"].double()
        v = sd[prefix + ".running_var"].double()
        s = g / torch.sqrt(v + 1e-5)                         # nn.BatchNorm2d eps
        return s, b - m * s

    def _prepare(self):
        lib = self._lib = L.load()
        dev = self.device
        self._dev.clear()
        for p in self._plans.values():
            lib.ppn_plan_destroy(p.handle)
        self._plans.clear()
        self._dev["zero"] = torch.zeros(64, dtype=torch.float32, device=dev)
        stream = L.current_stream_ptr()

        def pack(dtype, wd, cout, cin, k, cpad, ktot, korder, kstep, tdt):
            """[cpad][ktot] packed copy of the device weight `wd` (asynchronous: `wd` must outlive the pack kernel)."""
            packed = torch.empty(cpad, ktot, dtype=tdt, device=dev)
            L.check(lib.ppn_pack_weight(dtype, wd.data_ptr(), cout, cin, k, cpad, ktot, korder, kstep, packed.data_ptr(),
                                        stream), "ppn_pack_weight")
            return packed
        for op in self._ops:
            w = self._sd[op.weight].float().contiguous()
            s1 = b1 = None
            if op.bn1:
                s1, b1 = self._fold_bn(op.bn1)
            if op.bias:
                bias = self._sd[op.bias].double()
                b1 = bias * s1 + b1 if s1 is not None else bias
            if s1 is not None:
                self._dev[op.name + ".s1"] = s1.float().to(dev)
            if b1 is not None:
                self._dev[op.name + ".b1"] = b1.float().to(dev)
            if op.bn2:
                s2, b2 = self._fold_bn(op.bn2)
                self._dev[op.name + ".s2"] = s2.float().to(dev)
                self._dev[op.name + ".b2"] = b2.float().to(dev)
            if op.k == 7:                                     # stem keeps the reference layout in f32
                self._dev[op.name + ".w"] = w.to(dev)
                # layer1 (w1, s1b, b1b) and layer2 (w2, s1c, b1c) fused into the same launch
                for nxt, sfx in ((op.next3x3, ("w1", "s1b", "b1b")), (op.next_s2, ("w2", "s1c", "b1c"))):
                    if nxt is not None:
                        sn, bn_ = self._fold_bn(nxt.bn1)
                        for key, t in zip(sfx, (self._sd[nxt.weight].float().contiguous(), sn.float(), bn_.float())):
                            self._dev[f"{op.name}.{key}"] = t.to(dev)
                continue
            odt = self._op_dtype(op)
            kstep, korder, kmain, ktot, cpad = LW.weight_geometry(odt, op)
            if odt == L.PPN_F16X3:
                # split-f16 weights: three half copies of w * 2^s per 64-channel slab (csrc/conv_big.hip, X3); 2^-s is
                # folded into scale1 (a power of two: exact)
                wmax = float(w.abs().max())
                sl2 = int(np.floor(np.log2(32768.0 / wmax))) if wmax > 0 else 0
                sl2 = max(-24, min(24, sl2))
                wd = w.to(dev)
                packed = torch.empty(cpad, ktot, dtype=torch.float16, device=dev)
                L.check(lib.ppn_pack_weight_x3(wd.data_ptr(), op.cout, op.cin, op.k, cpad, sl2, packed.data_ptr(), stream),
                        "ppn_pack_weight_x3")
                base = s1 if s1 is not None else torch.ones(op.cout, dtype=torch.float64)
                self._dev[op.name + ".s1"] = (base * (2.0 ** -sl2)).float().to(dev)
                self._dev[op.name + ".w"] = packed
                torch.cuda.synchronize(dev)
                continue
            wd = w.to(dev)
            tdt = self._tdt(odt)
            packed = pack(odt, wd, op.cout, op.cin, op.k, cpad, kmain, korder, kstep, torch.float32 if korder == 2 else tdt)
            if op.ds_src:
                # fused projection shortcut: [main | 1x1 weights * BN scale] per packed row, BN shift -> shift1
                assert korder == 1 and s1 is None and op.ds_cin % kstep == 0
                sds, bds = self._fold_bn(op.ds_bn)
                wds = (self._sd[op.ds_weight].double() * sds.view(-1, 1, 1, 1)).float().contiguous().to(dev)
                pds = pack(odt, wds, op.cout, op.ds_cin, 1, cpad, op.ds_cin, 1, kstep, tdt)
                packed = torch.cat([packed, pds], dim=1).contiguous()
                self._dev[op.name + ".b1"] = (bds if b1 is None else b1 + bds).float().to(dev)
            self._dev[op.name + ".w"] = packed
            if op.nchw_f32_out and self._head_edge_pad():
                # fused-decode plans (forward_u8(fused_decode=True)): the head conv as TWO launches -- the 6K unary
                # channels as an ordinary NCHW conv of their own, and the limb channels with one 448-row channel tile per
                # edge (ppn_conv_desc.limb_edge_pad), whose epilogue reduces each window's arg-max on the accumulators
                ep, nun = self._head_edge_pad(), 6 * len(self.keypoint_names)
                win, ne = self.local_grid_size[0] * self.local_grid_size[1], len(self.edges)
                bias = self._sd[op.bias].float() if op.bias else torch.zeros(op.cout)
                assert op.bn1 is None and op.k == 1 and op.cout == nun + ne * win
                wu = w[:nun].contiguous().to(dev)
                ks_u, _, ko_u, kt_u, cp_u = L.conv_tiling(self.compute_dtype, op.cin, nun, 1)
                self._dev[op.name + ".w_unary"] = pack(self.compute_dtype, wu, nun, op.cin, 1, cp_u, kt_u, ko_u, ks_u, tdt)
                self._dev[op.name + ".b_unary"] = bias[:nun].contiguous().to(dev)
                we = torch.zeros(ne, ep, op.cin, 1, 1)
                we[:, :win] = w[nun:].view(ne, win, op.cin, 1, 1)
                we = we.view(ne * ep, op.cin, 1, 1).contiguous().to(dev)
                pe = pack(self.compute_dtype, we, ne * ep, op.cin, 1, ne * ep, ktot, korder, kstep, tdt)
                be = torch.zeros(ne, ep)
                be[:, :win] = bias[nun:].view(ne, win)
                self._dev[op.name + ".w_edge"], self._dev[op.name + ".b_edge"] = pe, be.view(-1).contiguous().to(dev)
                torch.cuda.synchronize(dev)               # `wu` / `we` die here: their pack kernels must have run
        torch.cuda.synchronize(dev)

    _TORCH = {LW.F32: torch.float32, LW.BF16: torch.bfloat16, LW.F16: torch.float16, LW.X3: torch.float16,
              LW.U8: torch.uint8, LW.I64: torch.int64}

    def _tdt(self, dtype=None):
        return self._TORCH[self.compute_dtype if dtype is None else dtype]

    def _op_dtype(self, op) -> int:
        return LW.op_dtype(self.mode, op)

    def _is_x3_stem(self, op) -> bool:
        return LW.is_x3_stem(self.mode, op)

    def _head_edge_pad(self) -> int:
        """lowering.head_edge_pad for this model's limb window; PPN_HEAD_EDGE=0 forces the chunked epilogue."""
        return LW.head_edge_pad(self.mode, self.local_grid_size[0] * self.local_grid_size[1],
                                os.environ.get("PPN_HEAD_EDGE", "1") != "0")

    # ---- plans ------------------------------------------------------------------------------------
    def _ptr(self, key: Optional[str]):
        t = self._dev.get(key) if key else None
        return t.data_ptr() if t is not None else None

    def _build_plan(self, batch: int, h: int, w: int, src_is_u8: bool, fused: bool = False, conv_flags: int = 0) -> _Plan:
        """lowering.lower decides; this allocates one buffer per tensor-table row (first the plan's own input: u8 [B,H,W,3]
        frames or the f32 [B,3,H,W] normalised image of model.forward) and adds one plan entry per launch record."""
        env = os.environ
        low = LW.lower(self._ops, self.mode, batch, h, w, src_is_u8, fused, conv_flags,
                       raw_s2=env.get("PPN_STEM_RAW_S2", "1") != "0", prefetch=env.get("PPN_PREFETCH", "1") != "0",
                       head_edge=env.get("PPN_HEAD_EDGE", "1") != "0", n_unary=6 * len(self.keypoint_names),
                       n_edges=len(self.edges), limb_window=self.local_grid_size[0] * self.local_grid_size[1],
                       **({"latency": True} if self.latency else {}))
        tensors = {}
        for name, (shape, st) in low.tensors.items():
            if name == "unary":
                # the compact outputs of a fused-decode plan are carved from the block a materialised head would take (taken
                # and handed back to the caching allocator here): plans have always been laid out in HBM this way, and one
                # same-box round without it ran 0.7-2.6 % slower in every pair (profiles/ab_lowering_refactor.txt)
                torch.empty(batch, self.lastsize, *shape[2:], dtype=torch.float32, device=self.device)
            tensors[name] = torch.empty(*shape, dtype=self._TORCH[st], device=self.device)
        # ONE split-K workspace per plan, sized to the largest need among its flagged launches: the launches of a plan run
        # one after the other on one stream, and each writes every byte it reads
        need = 0
        for launch in low.launches:
            if launch.kind == "conv" and launch.scalars.get("flags", 0) & L.PPN_CONV_SPLIT_K:
                nbytes = C.c_int64(0)
                L.check(self._lib.ppn_conv_splitk_workspace(C.byref(L.ConvDesc(**launch.scalars)), C.byref(nbytes), None),
                        f"ppn_conv_splitk_workspace({launch.name})")
                need = max(need, nbytes.value)
        workspace = torch.empty(need, dtype=torch.uint8, device=self.device) if need else None
        handle = C.c_void_p()
        L.check(self._lib.ppn_plan_create(C.byref(handle)), "ppn_plan_create")
        for launch in low.launches:
            L.check(self._emit(handle, launch, tensors, workspace), f"ppn_plan_add_{launch.kind}({launch.name})")
        bufs = {k: t for k, t in tensors.items() if k != "input"}
        head = (bufs["unary"], bufs["keys"]) if fused else bufs["head"]
        return _Plan(handle, bufs, head, low.entries, low.flops, tensors["input"], workspace)

    def _emit(self, handle, launch: LW.Launch, tensors, workspace=None) -> int:
        """One ppn_plan_add_* call: the record's tensor names become buffer pointers, its parameter keys `_dev` pointers
        (a key `_dev` does not hold: NULL)."""
        lib, s = self._lib, launch.scalars
        t = {f: tensors[n].data_ptr() for f, n in launch.tensors.items()}
        p = {f: self._ptr(k) for f, k in launch.params.items()}
        if launch.kind in ("conv", "block"):
            d = (L.ConvDesc if launch.kind == "conv" else L.BlockDesc)(**s, **t, **p)
            pf = self._dev.get(launch.params.get("prefetch"))
            if pf is not None:
                d.prefetch_bytes = pf.numel() * pf.element_size()
            if launch.kind == "conv" and s.get("flags", 0) & L.PPN_CONV_SPLIT_K:
                d.splitk_ws, d.splitk_ws_bytes = workspace.data_ptr(), workspace.numel()
            return (lib.ppn_plan_add_conv if launch.kind == "conv" else lib.ppn_plan_add_block)(handle, C.byref(d))
        if launch.kind == "split":
            return lib.ppn_plan_add_split(handle, t["src"], s["rows"], s["channels"], t["dst"])
        if launch.kind == "memset":
            return lib.ppn_plan_add_memset(handle, t["dst"], s["bytes"])
        # the stem family: layer 0's parameters, the normalisation, the fused layers' parameters, the outputs
        p = list(p.values())
        args = [handle, s["dtype"], s["src_is_u8"], t["src"], s["batch"], s["h"], s["w"], *p[:3], self._mean, self._std,
                *p[3:], t.get("out_raw")]
        if launch.kind == "stem012":
            return lib.ppn_plan_add_stem012_dt(*args, t.get("out_act"))
        return (lib.ppn_plan_add_stem01 if launch.kind == "stem01" else lib.ppn_plan_add_stem)(*args)

    def _get_plan(self, b: int, h: int, w: int, src_is_u8: bool, fused: bool = False, slot: int = 0,
                  conv_flags: int = 0) -> _Plan:
        if not self._dev:
            raise RuntimeError("PoseProposalNet: call load_state_dict() first")
        # slot: independent output buffers (pipelined serving); conv_flags: ppn_conv_desc.flags of every conv of the plan
        key = (b, h, w, src_is_u8, fused, slot) if not conv_flags else (b, h, w, src_is_u8, fused, slot, conv_flags)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = self._build_plan(b, h, w, src_is_u8, fused, conv_flags)
        return plan

    def _plan_for(self, x: torch.Tensor, src_is_u8: bool, fused: bool = False, slot: int = 0, conv_flags: int = 0) -> _Plan:
        if src_is_u8:
            b, h, w, _ = x.shape
        else:
            b, _, h, w = x.shape
        plan = self._get_plan(b, h, w, src_is_u8, fused, slot, conv_flags)
        # Frames go through the plan's own input buffer (a D2D copy on the caller's stream: 442 KB per 384x384 u8
        # frame), so the hipGraph captured for this plan is replayed whatever tensor the caller hands in -- a server
        # that uploads a fresh tensor per frame would otherwise re-capture ~35 nodes on every call.  Callers that
        # want zero copies write into `input_buffer(...)` and pass that tensor.
        if x.data_ptr() != plan.input.data_ptr():
            plan.input.copy_(x)
        return plan

    def input_buffer(self, batch: int, h: int, w: int, u8: bool = True, fused_decode: bool = False,
                     slot: int = 0, conv_flags: int = 0) -> torch.Tensor:
        """The plan-owned input tensor for this shape (u8 [B,H,W,3] or f32 [B,3,H,W]): fill it (e.g. an H2D copy
        straight into it) and pass it to forward_u8 / forward to skip the D2D copy."""
        return self._get_plan(batch, h, w, u8, fused_decode, slot, conv_flags).input

    # ---- forward --------------------------------------------------------------------------------
    def forward(self, input: torch.Tensor) -> torch.Tensor:
        """model.py:104-136: f32 [B,3,H,W] normalised image -> sigmoid head f32 [B,lastsize,H/16,W/16].

        The returned tensor is owned by the model's plan for this input buffer and is overwritten by the
        next forward of the same shape (clone it to keep it)."""
        if not (input.is_cuda and input.dtype == torch.float32 and input.dim() == 4 and input.shape[1] == 3):
            raise ValueError("forward expects a float32 CUDA tensor [B,3,H,W]")
        if self.training:                                  # model.train(): batch statistics, running stats advance
            return self._trainer.forward(input)
        x = input.contiguous()
        plan = self._plan_for(x, False)
        L.check(self._lib.ppn_plan_run(plan.handle, L.current_stream_ptr()), "ppn_plan_run")
        return plan.head

    __call__ = forward

    def forward_u8(self, frames: torch.Tensor, fused_decode: bool = False, slot: int = 0, conv_flags: int = 0):
        """Fused rt_test.py:97-101 + forward: u8 [B,H,W,3] RGB frames on the device -> head.

        With ``fused_decode=True`` the head conv's epilogue runs the decode's limb arg-max itself and the
        17.5 MB/image head is never written: returns ``(unary f32 [B,6K,H,W], keys i64 [B,E,H,W])`` for
        ``Decoder.decode_fused`` (results bit-identical to decoding the materialised head).  Plans of different
        ``slot`` own different output buffers, so a consumer on another stream may still be reading slot 0's
        outputs while slot 1's forward runs (rt.InferencePipeline).  ``conv_flags``: ppn_conv_desc.flags of the plan's
        convolutions (lib.PPN_CONV_NO_FILTER_BANK: the choice of a plan that shares the GPU with other lanes)."""
        if not (frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3):
            raise ValueError("forward_u8 expects a uint8 CUDA tensor [B,H,W,3]")
        if self.training:
            raise RuntimeError("forward_u8 is the inference entry point (folded BN): call model.eval() first")
        x = frames.contiguous()
        plan = self._plan_for(x, True, fused_decode, slot, conv_flags)
        L.check(self._lib.ppn_plan_run(plan.handle, L.current_stream_ptr()), "ppn_plan_run")
        return plan.head

    def profile_layers(self, x: torch.Tensor, src_is_u8: bool = False, repeats: int = 1, fused_decode: bool = False,
                       conv_flags: int = 0):
        """Per-launch durations (ms) measured with HIP events on the launch stream: [(op name, kernel, ms, flops)].
        `repeats` launches of each op are issued back to back between its events (amortises the event gap).
        conv_flags: as forward_u8 -- pass the timed path's flags to time the kernels THAT path runs."""
        plan = self._plan_for(x.contiguous(), src_is_u8, fused_decode, conv_flags=conv_flags)
        ms = (C.c_float * plan.n_ops)()
        L.check(self._lib.ppn_plan_run_timed(plan.handle, L.current_stream_ptr(), ms, plan.n_ops, repeats),
                "ppn_plan_run_timed")
        return [(name, self._lib.ppn_plan_kernel_name(plan.handle, i).decode(), float(ms[i]), fl)
                for i, (name, fl) in enumerate(plan.entries)]

    def half_range_report(self, frames: torch.Tensor) -> Dict[str, float]:
        """max |value| / 65504 of every tensor a plan stores in IEEE half for these u8 frames (the bf16 mode's half PREFIX --
        stem + layer3-4 -- and every tensor of the float16 mode).  Half stores CLAMP at +-65504 instead of overflowing
        (csrc/conv_common.h clamp_f16), so a checkpoint whose early activations exceed that range saturates silently: a
        value of 1.0 here says it did (tests/test_16bit_floors_gpu.py::test_half_prefix_saturates_at_65504); run such a
        checkpoint with half_prefix=-1, stem_dtype="bfloat16" (pure bf16: the f32 exponent range) or in float32."""
        self.forward_u8(frames)
        b, h, w, _ = frames.shape
        plan = self._get_plan(b, h, w, True)
        torch.cuda.synchronize(self.device)
        return {name: float(t.abs().max().item()) / 65504.0 for name, t in plan.buffers.items()
                if isinstance(t, torch.Tensor) and t.dtype == torch.float16 and not name.endswith("#x3")}

    def graph_captures(self) -> Dict[tuple, int]:
        """How often each plan (batch, h, w, u8, fused, slot) has captured its launch sequence into a hipGraph."""
        return {k: int(self._lib.ppn_plan_graph_captures(p.handle)) for k, p in self._plans.items()}

    def __del__(self):
        try:
            for p in self._plans.values():
                self._lib.ppn_plan_destroy(p.handle)
        except Exception:
            pass
