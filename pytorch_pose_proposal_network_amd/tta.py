"""Horizontal-flip test-time averaging over csrc/tta.hip (the reference has no counterpart).

The network sees a frame and its left-right mirror image in one doubled batch; the second head is mapped back -- left/right
keypoint channels, the cell-relative x offset, the limb windows' relative column and the left/right edge pairs all change
under mirroring -- and averaged with the first, and only then the decode runs (rules: include/ppn.h, ppn_tta_merge; NumPy
restatement tests/tta_ref.py).

* ``mirror_tables()``                      -- (kp_mirror, edge_mirror) of a skeleton, pure Python.
* ``FlipMerger(batch, out_hw, local_grid)`` -- ``stage(x)`` builds the doubled batch [x | x mirrored] (straight into a plan's
                                              input buffer), ``merge(head_pair)`` reads the two heads once and returns the
                                              ``(unary, keys)`` pair ``Decoder.decode_fused`` takes; the merged head itself
                                              only on request.  The steady state allocates nothing.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

from . import config as cfg


def _swap_side(name: str) -> str:
    if name.startswith("left_"):
        return "right_" + name[len("left_"):]
    if name.startswith("right_"):
        return "left_" + name[len("right_"):]
    return name


def mirror_tables(keypoint_names: Sequence[str] = cfg.KEYPOINT_NAMES,
                  edges_by_name: Sequence[Tuple[str, str]] = cfg.EDGES_BY_NAME) -> Tuple[List[int], List[int]]:
    """kp_mirror[k]: the keypoint whose name has ``left_`` / ``right_`` swapped (itself without such a prefix);
    edge_mirror[e]: the edge (kp_mirror[src], kp_mirror[dst]).  Both are involutions.  A skeleton whose keypoints or edges
    are not closed under the swap has no mirror: ValueError."""
    names = list(keypoint_names)
    index = {n: i for i, n in enumerate(names)}
    if len(index) != len(names):
        raise ValueError("keypoint names are not unique")
    kp_mirror = []
    for n in names:
        m = _swap_side(n)
        if m not in index:
            raise ValueError(f"keypoint {n!r} has no mirror partner {m!r}")
        kp_mirror.append(index[m])
    edges = [(s, d) for s, d in edges_by_name]
    edge_index = {e: i for i, e in enumerate(edges)}
    if len(edge_index) != len(edges):
        raise ValueError("edges are not unique")
    edge_mirror = []
    for s, d in edges:
        if s not in index or d not in index:
            raise ValueError(f"edge {(s, d)!r} names an unknown keypoint")
        m = (_swap_side(s), _swap_side(d))
        if m not in edge_index:
            raise ValueError(f"edge {(s, d)!r} has no mirror partner {m!r}: the skeleton is not closed under the swap")
        edge_mirror.append(edge_index[m])
    return kp_mirror, edge_mirror


def make_cfg(out_hw=(24, 24), local_grid=cfg.LOCAL_GRID_SIZE, kp_mirror: Optional[Sequence[int]] = None,
             edge_mirror: Optional[Sequence[int]] = None):
    """ppn_tta_cfg for a grid ``out_hw`` = (H, W) and a limb window ``local_grid`` = (sW, sH); the project's skeleton unless
    both tables are given."""
    from . import lib as L
    if (kp_mirror is None) != (edge_mirror is None):
        raise ValueError("give both mirror tables or neither")
    if kp_mirror is None:
        kp_mirror, edge_mirror = mirror_tables()
    if len(kp_mirror) > L.PPN_MAX_KP or len(edge_mirror) > L.PPN_MAX_EDGES:
        raise ValueError(f"{len(kp_mirror)} keypoints / {len(edge_mirror)} edges beyond {L.PPN_MAX_KP} / {L.PPN_MAX_EDGES}")
    c = L.TtaCfg()
    c.K, c.E = len(kp_mirror), len(edge_mirror)
    c.sW, c.sH = local_grid
    c.H, c.W = out_hw
    for i, m in enumerate(kp_mirror):
        c.kp_mirror[i] = m
    for i, m in enumerate(edge_mirror):
        c.edge_mirror[i] = m
    return c


class FlipMerger:
    """Owns ``unary`` f32 [B,6K,H,W] and ``keys`` i64 [B,E,H,W] (and, from the first ``want_head`` call on, ``head`` f32
    [B,C,H,W]) for a fixed batch and grid, so repeated calls allocate nothing."""

    def __init__(self, batch: int, out_hw=(24, 24), local_grid=cfg.LOCAL_GRID_SIZE, device="cuda"):
        import torch
        from . import lib as L
        self.lib = L.load()
        self.cfg = make_cfg(out_hw, local_grid)
        self.batch = int(batch)
        if self.batch < 1:
            raise ValueError("FlipMerger needs a batch of at least one image")
        c = self.cfg
        self.channels = 6 * c.K + c.E * c.sH * c.sW
        self.device = torch.device(device)
        self.unary = torch.empty(self.batch, 6 * c.K, c.H, c.W, dtype=torch.float32, device=self.device)
        self.keys = torch.empty(self.batch, c.E, c.H, c.W, dtype=torch.int64, device=self.device)
        self.head = None

    def stage(self, x, out=None):
        """The doubled batch of ``x`` -- u8 [B,H,W,3] frames or an f32 [B,3,H,W] input on the device: ``out[:B] = x``,
        ``out[B:]`` = x mirrored left-right.  ``out`` may be the model's own input buffer of batch 2B
        (``model.input_buffer(2 * B, ...)``): the forward then runs without a further copy."""
        import torch
        from . import lib as L
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4):
            raise ValueError("stage expects a CUDA tensor: uint8 [B,H,W,3] or float32 [B,3,H,W]")
        if x.dtype == torch.uint8 and x.shape[3] == 3:
            b, h, w, _ = x.shape
            rows, elem = b * h, 3
        elif x.dtype == torch.float32 and x.shape[1] == 3:
            b, _, h, w = x.shape
            rows, elem = b * 3 * h, 4
        else:
            raise ValueError("stage expects uint8 [B,H,W,3] frames or a float32 [B,3,H,W] input")
        x = x.contiguous()
        shape = (2 * b,) + tuple(x.shape[1:])
        if out is None:
            out = torch.empty(shape, dtype=x.dtype, device=x.device)
        if tuple(out.shape) != shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {x.dtype} tensor {shape} on {x.device}")
        L.check(self.lib.ppn_tta_stage(x.data_ptr(), out.data_ptr(), rows, w, elem, L.current_stream_ptr()),
                "ppn_tta_stage")
        return out

    def merge(self, head_pair, want_head: bool = False):
        """``head_pair`` f32 [2B,C,H,W]: the heads of the frames (first half) and of the mirrored frames (second half).
        Returns ``(unary, keys)`` for ``Decoder.decode_fused``, or ``(unary, keys, head)`` with the merged head."""
        import torch
        from . import lib as L
        c = self.cfg
        shape = (2 * self.batch, self.channels, c.H, c.W)
        if not (isinstance(head_pair, torch.Tensor) and head_pair.is_cuda and head_pair.dtype == torch.float32
                and head_pair.is_contiguous() and tuple(head_pair.shape) == shape):
            raise ValueError(f"head_pair must be a contiguous float32 CUDA tensor {shape}")
        if want_head and self.head is None:
            self.head = torch.empty(self.batch, self.channels, c.H, c.W, dtype=torch.float32, device=self.device)
        half = self.batch * self.channels * c.H * c.W * 4
        L.check(self.lib.ppn_tta_merge(C.byref(c), head_pair.data_ptr(), head_pair.data_ptr() + half, self.batch,
                                       self.unary.data_ptr(), self.keys.data_ptr(),
                                       self.head.data_ptr() if want_head else None, L.current_stream_ptr()),
                "ppn_tta_merge")
        if want_head:
            return self.unary, self.keys, self.head
        return self.unary, self.keys
