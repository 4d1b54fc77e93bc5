"""CrossEntropyLoss and FocalLoss entries of the LOSSES registry (reference: pointcept/models/losses/misc.py).

FocalLoss (the multi-class sigmoid form, misc.py:96-172): on a GPU prediction the loss and its backward are HIP kernels
(csrc/seg_loss.hip through ptv3_hip.autograd); a CPU tensor, more than 1024 classes, N * C >= 2^31 or `use_hip = False`
take `focal_loss_torch`, the same function as a torch composition without the reference's boolean-mask compaction (a
host read).  Differences from the reference, on purpose: a label outside [0, C) that is not `ignore_index` makes the
row ignored (F.one_hot faults there); with no valid row the loss is a 0-d zero tensor (the reference returns the float
0.0); reduction="sum" returns the sum (the reference calls a method that does not exist, `loss.total()`).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .builder import LOSSES


@LOSSES.register_module()
class CrossEntropyLoss(nn.Module):
    def __init__(self, weight=None, size_average=None, reduce=None, reduction="mean", label_smoothing=0.0,
                 loss_weight=1.0, ignore_index=-1):
        super().__init__()
        weight = torch.tensor(weight).cuda() if weight is not None else None
        self.loss_weight = loss_weight
        self.loss = nn.CrossEntropyLoss(weight=weight, size_average=size_average, ignore_index=ignore_index,
                                        reduce=reduce, reduction=reduction, label_smoothing=label_smoothing)

    def forward(self, pred, target):
        return self.loss(pred, target) * self.loss_weight


def focal_loss_torch(pred, target, alpha, gamma=2.0, ignore_index=-1, loss_weight=1.0, reduction="mean"):
    """misc.py:151-172 on (N, C) logits with the ignored rows masked instead of removed; alpha: float or (C) tensor."""
    n, c = pred.shape
    valid = (target >= 0) & (target < c)
    if ignore_index is not None:
        valid = valid & (target != ignore_index)
    t = ((target.unsqueeze(1) == torch.arange(c, device=target.device)) & valid.unsqueeze(1)).to(pred.dtype)
    s = pred.sigmoid()
    one_minus_pt = (1 - s) * t + s * (1 - t)
    focal_weight = (alpha * t + (1 - alpha) * (1 - t)) * one_minus_pt.pow(gamma)
    loss = (F.binary_cross_entropy_with_logits(pred, t, reduction="none") * focal_weight * valid.unsqueeze(1)).sum()
    if reduction == "mean":
        loss = loss / (valid.sum() * c).clamp(min=1)
    return loss_weight * loss


@LOSSES.register_module()
class FocalLoss(nn.Module):
    def __init__(self, gamma=2.0, alpha=0.5, reduction="mean", loss_weight=1.0, ignore_index=-1):
        super().__init__()
        assert reduction in ("mean", "sum"), "AssertionError: reduction should be 'mean' or 'sum'"
        assert isinstance(alpha, (float, list)), "AssertionError: alpha should be of type float"
        assert isinstance(gamma, float), "AssertionError: gamma should be of type float"
        assert isinstance(loss_weight, float), "AssertionError: loss_weight should be of type float"
        assert isinstance(ignore_index, int), "ignore_index must be of type int"
        self.gamma = gamma
        self.alpha = alpha
        self.reduction = reduction
        self.loss_weight = loss_weight
        self.ignore_index = ignore_index
        self.use_hip = True
        self._alpha_dev = {}

    def _alpha(self, c, device, dtype):
        """alpha as a (C) tensor on `device` (a scalar is broadcast), built once per device."""
        key = (c, str(device), dtype)
        if key not in self._alpha_dev:
            a = self.alpha if isinstance(self.alpha, list) else [self.alpha] * c
            self._alpha_dev[key] = torch.tensor(a, dtype=dtype, device=device)
        return self._alpha_dev[key]

    def forward(self, pred, target, **kwargs):
        # (B, C, d1, ...) -> (N, C), misc.py:133-140
        pred = pred.transpose(0, 1)
        pred = pred.reshape(pred.size(0), -1).transpose(0, 1).contiguous()
        target = target.view(-1).contiguous()
        assert pred.size(0) == target.size(0), "The shape of pred doesn't match the shape of target"
        n, c = pred.shape
        if self.use_hip and pred.is_cuda and pred.is_floating_point() and self.gamma >= 0:
            from ptv3_hip import autograd as A, ops
            if ops.seg_loss_capable(n, c):
                return A.focal_loss(pred.float(), target.long(), self._alpha(c, pred.device, torch.float32), self.gamma,
                                    self.ignore_index, self.loss_weight, self.reduction)
        return focal_loss_torch(pred, target, self._alpha(c, pred.device, pred.dtype), self.gamma, self.ignore_index,
                                self.loss_weight, self.reduction)
