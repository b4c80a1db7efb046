"""The multi-stage training loss on the device: ``Loss`` with the surface of the reference's modules/loss.py:17-64 over
the fused kernels of csrc/loss.hip (decnet_stage_loss_forward / _backward, include/decnet_hip.h).

One ``StageLossFunction`` call per pyramid level replaces the reference's dozen ``x[mask]`` gathers of that level
(loss.py:201-239): nothing is compacted, no value is read back to the host and no shape depends on the data, so the whole
forward + backward runs under ``torch.cuda.graph`` (a ``graphs.GraphedStep`` can end at the loss instead of at the SpaMat
output) and replays the bits of the eager call.  The ground truth of a level is downsampled by torch, with the very call
the reference makes (loss.py:188-194): these ops are tiny and capturable, and every ``down_func_name`` keeps working.

Supported loss types: ``multi_stage_regression_uploss`` (loss.py:168-242) and ``multi_stage_regression_upsampleloss``
(loss.py:362-395).  ``chamfer``, ``lr_consistency`` and ``multi_stage_regression_upmaskloss`` raise NotImplementedError.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function

from . import ops

LOSS_TYPES = ("chamfer", "multi_stage_regression_uploss", "lr_consistency", "multi_stage_regression_upsampleloss",
              "multi_stage_regression_upmaskloss")
OVERMASK_ROWS = 108                     # full-resolution rows if_overmask drops from the top (loss.py:204-205)
# positions in the terms tensor: the order the reference appends a composite stage to loss_list (loss.py:233-237)
T_DENSE, T_SPARSE, T_SOFT, T_FUSION, T_PRED = range(5)


class StageLossFunction(Function):
    """One level: planes [B,H,W] float32 -> terms [5] float32 (dense, sparse, soft-mask mean, fusion, pred).
    ``dense, sparse, fusion, soft_mask, left_mask`` all None: the simple form (only the pred term, the others 0).
    ``gt`` is at the level's resolution; ``gt`` and ``left_mask`` never get a gradient."""

    @staticmethod
    def forward(ctx, pred, dense, sparse, fusion, soft_mask, left_mask, gt, gt_max, down_size, skip_rows):
        if not isinstance(pred, torch.Tensor) or pred.dim() != 3:
            raise ValueError("pred must be [B,H,W]")
        B, H, W = pred.shape
        # row sums and totals in one float64 allocation: the totals are what the backward reads
        acc = torch.empty(B * H * 8 + 8, dtype=torch.float64, device=pred.device)
        row_sums, sums = acc[:B * H * 8].view(B * H, 8), acc[B * H * 8:]
        terms = torch.empty(5, dtype=torch.float32, device=pred.device)
        ops.stage_loss_forward(pred, dense, sparse, fusion, soft_mask, left_mask, gt, gt_max, down_size, skip_rows,
                               row_sums, sums, terms)
        ctx.save_for_backward(pred, dense, sparse, fusion, soft_mask, left_mask, gt, sums)
        ctx.args = (float(gt_max), float(down_size), int(skip_rows))
        return terms

    @staticmethod
    def backward(ctx, grad_terms):
        pred, dense, sparse, fusion, soft_mask, left_mask, gt, sums = ctx.saved_tensors
        # (pred, dense, sparse, fusion, soft_mask) are inputs 0..4; a simple-form call has only pred
        want = [ctx.needs_input_grad[i] and t is not None
                for i, t in enumerate((pred, dense, sparse, fusion, soft_mask))]
        grads = [None] * 5
        if any(want):
            planes = torch.empty((sum(want),) + tuple(pred.shape), dtype=pred.dtype, device=pred.device).unbind(0)
            it = iter(planes)
            grads = [next(it) if w else None for w in want]
            # an expanded gradient (terms.sum()) has stride 0: the kernel reads five floats
            ops.stage_loss_backward(pred, dense, sparse, fusion, soft_mask, left_mask, gt, *ctx.args, sums,
                                    grad_terms.contiguous(), *grads)
        return (*grads, None, None, None, None, None)


def stage_loss(pred, gt, gt_max, down_size=1.0, skip_rows=0, dense=None, sparse=None, fusion=None, soft_mask=None,
               left_mask=None):
    """``StageLossFunction.apply`` with keywords; returns the [5] terms tensor."""
    return StageLossFunction.apply(pred, dense, sparse, fusion, soft_mask, left_mask, gt, gt_max, down_size, skip_rows)


def downsample_gt(gt, down_size, down_func_name):
    """The ground truth [B,H,W] of the level ``down_size`` times coarser, values divided by down_size: the torch call the
    reference makes for each ``down_func_name`` (loss.py:188-194)."""
    x = gt.unsqueeze(1)
    if down_func_name in ("bilinear", "bicubic"):
        y = F.interpolate(x / down_size, scale_factor=1 / down_size, mode=down_func_name)
    elif down_func_name == "max":
        y = F.max_pool2d(x / down_size, down_size, down_size, 0, 1, False, False)
    elif down_func_name == "min":                       # the smallest POSITIVE value: zeros (no measurement) become 1e6
        filled = (gt * (gt > 0) + 1e6 * (gt == 0)).unsqueeze(1)
        y = -F.max_pool2d(-filled / down_size, down_size, down_size, 0, 1, False, False)
    else:
        raise ValueError("down_func_name must be bilinear, bicubic, max or min, got %r" % (down_func_name,))
    return y.squeeze(1).contiguous()


class Loss(nn.Module):
    def __init__(self, loss_type, if_overmask=False, stop_stage_id=4, if_train=True, thold=0.5, alpha=0.1):
        super().__init__()
        self.loss_type = loss_type.lower()
        self.if_overmask = if_overmask
        self.stop_stage_id = stop_stage_id
        self.if_train = if_train
        self.thold = thold
        self.alpha = alpha
        if self.loss_type not in LOSS_TYPES:
            raise ValueError("No such loss: %s" % self.loss_type)

    def forward(self, pred_list=None, fusion_list=None, dense_list=None, sparse_list=None, left_mask_list=None, gt=None,
                weights=None, num_stage=None, down_func_name=None, down_scale=None, max_disp=None, sparse_mask_list=None,
                left_feature_map_all=None, right_feature_map_all=None, left_detail_list=None, right_detail_list=None,
                right_mask_list=None):
        """Returns ``gt_list, pred_list, tot_loss, loss_list`` (loss.py:242).  pred_list: the predictions of the
        num_stage levels, coarsest first, each [B,H/s,W/s]; fusion / dense / sparse / left_mask / sparse_mask lists:
        entry i belongs to stage i + 1; gt [B,H,W]; weights: a number per stage."""
        if self.loss_type == "multi_stage_regression_uploss":
            return self.multi_stage_regression_uploss(pred_list, fusion_list, dense_list, sparse_list, left_mask_list,
                                                      gt, weights, num_stage, down_func_name, down_scale, max_disp,
                                                      sparse_mask_list)
        if self.loss_type == "multi_stage_regression_upsampleloss":
            return self.multi_stage_regression_upsampleloss(pred_list, gt, weights, num_stage, down_func_name,
                                                            down_scale, max_disp)
        raise NotImplementedError("decnet_amd.Loss: loss type %r is not implemented (supported: "
                                  "multi_stage_regression_uploss, multi_stage_regression_upsampleloss)" % self.loss_type)

    @staticmethod
    def _check_sizes(pred_list, gt):
        if tuple(pred_list[-1].shape[-2:]) != tuple(gt.shape[-2:]):
            raise ValueError("the last prediction is %s, the ground truth %s"
                             % (tuple(pred_list[-1].shape[-2:]), tuple(gt.shape[-2:])))

    def multi_stage_regression_uploss(self, pred_list, fusion_list, dense_list, sparse_list, left_mask_list, gt, weights,
                                      num_stage, down_func_name, down_scale, max_disp, sparse_mask_list=None):
        self._check_sizes(pred_list, gt)
        if sparse_mask_list is None and min(num_stage, self.stop_stage_id) > 1:
            raise ValueError("the stages 1 .. %d take the composite form: sparse_mask_list is needed"
                             % (min(num_stage, self.stop_stage_id) - 1))
        tot_loss = 0.
        gt_list, loss_list = [], []
        for stage_id in range(num_stage):
            if stage_id + 1 < num_stage:
                down_size = down_scale ** (num_stage - stage_id - 1)
                cur_gt = downsample_gt(gt, down_size, down_func_name)
            else:
                down_size, cur_gt = 1., gt
            gt_list.append(cur_gt)
            skip_rows = int(OVERMASK_ROWS // down_size) if self.if_overmask else 0
            gt_max = max_disp / down_size
            if stage_id == 0 or stage_id >= self.stop_stage_id:
                depth_loss = stage_loss(pred_list[stage_id], cur_gt, gt_max, down_size, skip_rows)[T_PRED]
                tot_loss = tot_loss + depth_loss * weights[stage_id]
                loss_list.append(depth_loss)
                continue
            i = stage_id - 1
            dense_loss, sparse_loss, soft_mean, fusion_loss, pred_loss = stage_loss(
                pred_list[stage_id], cur_gt, gt_max, down_size, skip_rows, dense=dense_list[i], sparse=sparse_list[i],
                fusion=fusion_list[i], soft_mask=sparse_mask_list[i], left_mask=left_mask_list[i]).unbind(0)
            loss_list += [dense_loss, sparse_loss, soft_mean, fusion_loss, pred_loss]
            tot_loss = tot_loss + (pred_loss * 0.5 + dense_loss * 0.1 + sparse_loss * 0.2 * 1 / (10 + stage_id * 3.75)
                                   + fusion_loss * 0.2) * weights[stage_id]
        return gt_list, pred_list, tot_loss, loss_list

    def multi_stage_regression_upsampleloss(self, pred_list, gt, weights, num_stage, down_func_name, down_scale, max_disp):
        self._check_sizes(pred_list, gt)
        tot_loss = 0.
        gt_list, loss_list = [], []
        for stage_id in range(num_stage):
            pred = pred_list[stage_id]
            if stage_id + 1 < num_stage:                # to full resolution by torch; autograd carries it back
                down_size = down_scale ** (num_stage - stage_id - 1)
                cur_pred = F.interpolate(pred.unsqueeze(1) * down_size, scale_factor=down_size,
                                         mode=down_func_name).squeeze(1).contiguous()
            else:
                cur_pred = pred
            pred_list.append(pred)                      # the reference grows the caller's list like this (loss.py:385)
            gt_list.append(gt)
            loss = stage_loss(cur_pred, gt, max_disp)[T_PRED]
            tot_loss = tot_loss + loss * weights[stage_id]
            loss_list.append(loss)
        return gt_list, pred_list, tot_loss, loss_list
