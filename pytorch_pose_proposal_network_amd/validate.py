"""A validation epoch on the device (reference: main.py:1017-1172 `validate`, 886-1014 `test_output`) over csrc/validate.hip.

* ``GroundTruth(gt_kps_list, gt_bboxes_list)``        -- the validation set's people, packed and uploaded once.
* ``Records(n_images, max_humans)``                   -- the epoch-long (score, label) buffers ppn_pckh_match fills.
* ``match_people(result, gt, image_index, records)``  -- one batch: the DecodeResult as it lives on the device against the
                                                         ground truth, on the current stream, no host synchronisation.
* ``Validator(net, gt, batch, ...)``                  -- reset() / step(x, image_index, targets) / finish() ->
                                                         (loss_avg, ap_vals), the return value of main.validate; step reads
                                                         nothing back, finish does the epoch's one D2H.

The matching is eval_helpers.assignGTmulti as evaluate.assign_gt_multi restates it (rules: include/ppn.h, ppn_pckh_match;
NumPy restatement tests/validate_ref.py); the AP curve stays evaluate.compute_metrics on the host, fed by
evaluate.metrics_from_records.  Not built: validation sharded over ranks, dataset reading, savefig / show_sample.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import decode as D
from . import evaluate
from . import lib as L

N_JOINTS = evaluate.N_JOINTS
MAX_GT = L.PPN_MATCH_MAX_GT                  # ground-truth people per image the kernel takes (one wave lane each)


class GroundTruth:
    """The reference's per-image `gt_kps` (f32 [G,17,2] (x, y), or anything that reshapes to it) and `gt_bboxes`
    ((cx, cy, w, h) per person) of a whole validation set as three resident tensors: gt_xy f32 [N,gmax,17,2], gt_head f32
    [N,gmax] (evaluate._head_sizes, computed here on the host, once), gt_count i32 [N].  `gmax` defaults to the largest G
    of the set; more than MAX_GT = 64 people in one image raise."""

    def __init__(self, gt_kps_list: Sequence, gt_bboxes_list: Sequence, device="cuda", gmax: Optional[int] = None):
        if len(gt_kps_list) != len(gt_bboxes_list):
            raise ValueError(f"{len(gt_kps_list)} keypoint arrays for {len(gt_bboxes_list)} box lists")
        n = len(gt_bboxes_list)
        if n == 0:
            raise ValueError("GroundTruth needs at least one image")
        counts = np.array([len(b) for b in gt_bboxes_list], np.int32)
        largest = int(counts.max())
        if largest > MAX_GT:
            raise ValueError(f"image {int(counts.argmax())} has {largest} ground-truth people, at most {MAX_GT} are supported")
        gmax = max(largest, 1) if gmax is None else int(gmax)
        if not largest <= gmax <= MAX_GT or gmax < 1:
            raise ValueError(f"gmax {gmax} must hold the largest image ({largest}) and be in 1..{MAX_GT}")
        xy = np.zeros((n, gmax, N_JOINTS, 2), np.float32)
        head = np.zeros((n, gmax), np.float32)
        for i, (kps, boxes) in enumerate(zip(gt_kps_list, gt_bboxes_list)):
            g = int(counts[i])
            if g == 0:
                continue
            kps = np.asarray(kps, np.float32)
            if kps.size != g * N_JOINTS * 2:
                raise ValueError(f"image {i}: {kps.size} keypoint values for {g} people")
            xy[i, :g] = kps.reshape(g, N_JOINTS, 2)
            head[i, :g] = evaluate._head_sizes(boxes)
        self._upload(xy, head, counts, device)

    def _upload(self, xy, head, counts, device):
        self.n_images, self.gmax = int(xy.shape[0]), int(xy.shape[1])
        self.counts = counts                                          # host copy: metrics_from_records' n_gt
        self.device = torch.device(device)
        self.gt_xy = torch.from_numpy(xy).to(self.device)
        self.gt_head = torch.from_numpy(head).to(self.device)
        self.gt_count = torch.from_numpy(counts).to(self.device)

    @classmethod
    def from_arrays(cls, gt_xy, gt_head, gt_count, device="cuda") -> "GroundTruth":
        """Tables packed elsewhere: gt_xy f32 [N,gmax,17,2], gt_head f32 [N,gmax], gt_count i32 [N] with every count in
        0..gmax and gmax in 1..MAX_GT."""
        xy = np.ascontiguousarray(gt_xy, np.float32)
        head = np.ascontiguousarray(gt_head, np.float32)
        counts = np.ascontiguousarray(gt_count, np.int32)
        if xy.ndim != 4 or xy.shape[2:] != (N_JOINTS, 2) or head.shape != xy.shape[:2] or counts.shape != xy.shape[:1]:
            raise ValueError("from_arrays takes gt_xy [N,gmax,17,2], gt_head [N,gmax] and gt_count [N]")
        if xy.shape[0] < 1 or not 1 <= xy.shape[1] <= MAX_GT:
            raise ValueError(f"{xy.shape[0]} images x {xy.shape[1]} people: at least one image, 1..{MAX_GT} people")
        if counts.min() < 0 or counts.max() > xy.shape[1]:
            raise ValueError(f"gt_count must lie in 0..{xy.shape[1]}")
        gt = cls.__new__(cls)
        gt._upload(xy, head, counts, device)
        return gt


class Records:
    """rec_score f32 [N,M,17], rec_label u8 [N,M,17], rec_count i32 [N] and the error flag word of one epoch."""

    def __init__(self, n_images: int, max_humans: int, device="cuda"):
        if n_images < 1 or not 1 <= max_humans <= L.PPN_MATCH_MAX_PEOPLE:
            raise ValueError(f"records for {n_images} images x {max_humans} people (at most {L.PPN_MATCH_MAX_PEOPLE})")
        dev = torch.device(device)
        self.n_images, self.max_humans = int(n_images), int(max_humans)
        self.score = torch.zeros(n_images, max_humans, N_JOINTS, dtype=torch.float32, device=dev)
        self.label = torch.zeros(n_images, max_humans, N_JOINTS, dtype=torch.uint8, device=dev)
        self.count = torch.zeros(n_images, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(1, dtype=torch.int32, device=dev)

    def reset(self):
        """An image no step reaches afterwards counts as one without predictions."""
        self.count.zero_()
        self.flags.zero_()

    def to_host(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
        return self.score.cpu().numpy(), self.label.cpu().numpy(), self.count.cpu().numpy(), int(self.flags.cpu()[0])


def _dense(name, t, shape, dtype, device):
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()
            and t.device == device):
        raise ValueError(f"{name} must be a contiguous {dtype} tensor {tuple(shape)} on {device}")
    return t


def match_people(result: D.DecodeResult, gt: GroundTruth, image_index: torch.Tensor, records: Records,
                 dist_thresh: float = 0.5) -> Records:
    """ppn_pckh_match: match the batch's people to the ground truth of the images `image_index` (i32 [B] on the device,
    -1 for a padding image) names and write their rows of `records`.  One launch on the current stream."""
    dev = records.score.device
    if not dev.type == "cuda":
        raise ValueError("match_people runs on the device: the records live on " + str(dev))
    B, M, K = result.kp_cell.shape
    if K != N_JOINTS + 1 or M != result.max_humans or M != records.max_humans:
        raise ValueError(f"result holds {M} people x {K} keypoints, the records {records.max_humans} x {N_JOINTS + 1}")
    if gt.n_images != records.n_images:
        raise ValueError(f"ground truth of {gt.n_images} images, records of {records.n_images}")
    _dense("result.count", result.count, (B,), torch.int32, dev)
    _dense("result.kp_cell", result.kp_cell, (B, M, K), torch.int32, dev)
    _dense("result.bbox", result.bbox, (B, M, K, 4), torch.float32, dev)
    _dense("result.score", result.score, (B, M, K), torch.float32, dev)
    _dense("image_index", image_index, (B,), torch.int32, dev)
    _dense("gt.gt_xy", gt.gt_xy, (gt.n_images, gt.gmax, N_JOINTS, 2), torch.float32, dev)
    L.check(L.load().ppn_pckh_match(result.count.data_ptr(), result.kp_cell.data_ptr(), result.bbox.data_ptr(),
                                    result.score.data_ptr(), B, M, gt.gt_xy.data_ptr(), gt.gt_head.data_ptr(),
                                    gt.gt_count.data_ptr(), gt.n_images, gt.gmax, image_index.data_ptr(), float(dist_thresh),
                                    records.score.data_ptr(), records.label.data_ptr(), records.count.data_ptr(),
                                    records.flags.data_ptr(), L.current_stream_ptr()), "ppn_pckh_match")
    return records


class Validator:
    """main.validate for an eval-mode `net` (model.PoseProposalNet) and a resident GroundTruth.

        v = Validator(net, gt, batch=32, criterion=PPNLoss(...), task_weights=trainer.task.w)
        v.reset()
        for x, image_index, targets in loader:       # x f32 [b,3,H,W] on the device, b <= batch
            v.step(x, image_index, targets)
        loss_avg, ap_vals = v.finish()

    step runs the forward with a materialised head (the loss needs it; the fused-decode path is out of scope), the five
    eval losses when `targets` is given, Decoder.__call__ and match_people, and reads nothing back.  A last batch of fewer
    than `batch` images is padded here: its head rows beyond b are decoded but marked -1, and its loss is taken over the b
    images only.  An image_index of -1 inside a full batch skips that image's records (its loss still counts: leave such
    images out of `targets` batches).

    flip_tta=True: horizontal-flip test-time averaging (tta.py).  The forward runs on the doubled batch [x | x mirrored]; the
    loss stays on the plain head of x, and only the decode that feeds match_people sees the merged pair (ppn_tta_merge ->
    Decoder.decode_fused)."""

    def __init__(self, net, gt: GroundTruth, batch: int, criterion=None, task_weights=None, detection_thresh: float = 0.15,
                 max_humans: int = 64, nms_thresh: float = 0.3, min_num_keypoints: int = 1, dist_thresh: float = 0.5,
                 flip_tta: bool = False):
        if getattr(net, "training", False):
            raise ValueError("Validator needs the network in eval mode (net.eval())")
        self.net, self.gt, self.batch, self.criterion = net, gt, int(batch), criterion
        self.dist_thresh = float(dist_thresh)
        dev = gt.device
        (inW, inH), (outW, outH) = net.insize, net.outsize
        self.decoder = D.Decoder(self.batch, (outH, outW), (inH, inW), net.local_grid_size, detection_thresh, nms_thresh,
                                 min_num_keypoints, max_humans, dev)
        self.records = Records(gt.n_images, max_humans, dev)
        self.merger = None
        if flip_tta:
            from .tta import FlipMerger
            self.merger = FlipMerger(self.batch, (outH, outW), net.local_grid_size, dev)
        self.task_weights = task_weights                     # read at finish(): the trainer's live tensor may be handed in
        self._x = torch.zeros(self.batch, 3, inH, inW, dtype=torch.float32, device=dev)
        self._index = torch.full((self.batch,), -1, dtype=torch.int32, device=dev)
        self._loss_sum = torch.zeros(5, dtype=torch.float64, device=dev)     # sum of losses * B
        self._seen = torch.zeros(1, dtype=torch.float64, device=dev)         # sum of B
        self._most_people = torch.zeros(1, dtype=torch.int32, device=dev)    # largest decode count of a recorded image

    def reset(self):
        self.records.reset()
        self._loss_sum.zero_()
        self._seen.zero_()
        self._most_people.zero_()

    def step(self, x: torch.Tensor, image_index, targets: Optional[Dict[str, torch.Tensor]] = None):
        b = x.shape[0]
        if not 1 <= b <= self.batch or tuple(x.shape[1:]) != tuple(self._x.shape[1:]):
            raise ValueError(f"x {tuple(x.shape)}: at most {self.batch} images of {tuple(self._x.shape[1:])}")
        index = torch.as_tensor(image_index, dtype=torch.int32).to(self._index.device).reshape(-1)
        if index.numel() != b:
            raise ValueError(f"{index.numel()} image indices for {b} images")
        if b < self.batch:                                   # ragged last batch: pad with images that record nothing
            self._x[:b].copy_(x)
            self._x[b:].zero_()
            self._index[:b].copy_(index)
            self._index[b:].fill_(-1)
            x, index = self._x, self._index
        if self.merger is not None:                          # [x | x mirrored] straight into the plan's input of batch 2B
            x = self.merger.stage(x, out=self.net.input_buffer(2 * self.batch, x.shape[2], x.shape[3], u8=False))
        head = self.net(x)
        if targets is not None:
            if self.criterion is None:
                raise ValueError("targets given, but the Validator has no criterion")
            losses, _ = self.criterion.forward_backward(head[:b], targets, want_grad=False)
            self._loss_sum.add_(losses.double(), alpha=b)
            self._seen.add_(b)
        if self.merger is not None:
            result = self.decoder.decode_fused(*self.merger.merge(head))
        else:
            result = self.decoder(head)
        torch.maximum(self._most_people, torch.where(index >= 0, result.count, 0).max().reshape(1), out=self._most_people)
        match_people(result, self.gt, index, self.records, self.dist_thresh)

    def finish(self) -> Tuple[Optional[float], List[float]]:
        """The epoch's one read-back -> (loss_avg, the 8 AP values); loss_avg is None when no step had targets."""
        rec_score, rec_label, rec_count, flags = self.records.to_host()
        loss_sum, seen, most = self._loss_sum.cpu().numpy(), float(self._seen.cpu()[0]), int(self._most_people.cpu()[0])
        if flags:
            what = [s for bit, s in ((L.PPN_MATCH_FLAG_INDEX, f"an image index outside [-1, {self.gt.n_images})"),
                                     (L.PPN_MATCH_FLAG_GT_COUNT, f"a ground-truth count outside [0, {self.gt.gmax}]"))
                    if flags & bit]
            raise RuntimeError("validation epoch: " + " and ".join(what or [f"flag word {flags}"]))
        if most > self.records.max_humans:
            raise RuntimeError(f"validation epoch: an image decoded to {most} people, the Validator keeps max_humans = "
                               f"{self.records.max_humans}; nothing is truncated silently -- raise max_humans")
        ap_vals = evaluate.metrics_from_records(rec_score, rec_label, rec_count, self.gt.counts)
        loss_avg = None
        if seen > 0:
            w = np.ones(5) if self.task_weights is None else \
                torch.as_tensor(self.task_weights).detach().double().cpu().numpy().reshape(5)
            loss_avg = float((w * (loss_sum / seen)).sum() / 5.0)
        return loss_avg, ap_vals
