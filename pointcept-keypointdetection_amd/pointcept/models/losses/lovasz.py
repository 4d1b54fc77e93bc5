"""LovaszLoss entry of the LOSSES registry (reference: pointcept/models/losses/lovasz.py), multiclass mode.

On a GPU prediction the loss and its backward are HIP kernels (csrc/seg_loss.hip through ptv3_hip.autograd): the
reference's `labels.unique()` loop with its per-class host reads becomes a fixed set of launches.  Anywhere else - a CPU
tensor, more than 1024 classes, N * C >= 2^31, or `use_hip = False` - `lovasz_softmax_torch` computes the same function
in torch, vectorised over the classes, with no `unique()` and no host read.

Differences from the reference, on purpose:
  - the Lovasz weights jaccard[i] - jaccard[i-1] (:22-33) are evaluated in closed form in float64 from integer counts;
    the reference's fp32 subtraction of near-equal numbers is off by tens of percent at a few thousand rows;
  - ties in the errors are ordered by point index (a stable sort); the loss does not depend on the order inside a tie;
  - a label outside [0, C) that is not `ignore_index` makes the row ignored (the reference faults);
  - with no valid row the loss is a 0-d zero (the reference returns an empty tensor).
"""
import torch
import torch.nn as nn

from .builder import LOSSES

BINARY_MODE = "binary"
MULTICLASS_MODE = "multiclass"
MULTILABEL_MODE = "multilabel"


def lovasz_weights(fg_sorted, valid_sorted):
    """Closed-form Lovasz weights along a sorted order.  fg_sorted, valid_sorted: (N, C) bool, column c in class c's
    order, the valid rows first.  With F the running foreground count at position i (1-based), G the column's total:
    I = G - F, U = G + i - F; weight 1/U on foreground, I / (U (U - 1)) on background, 1 - I/U at i = 1 on background.
    -> (N, C) float64, 0 on rows that are not valid."""
    n = fg_sorted.shape[0]
    F = fg_sorted.long().cumsum(0)
    G = F[-1:] if n else F.new_zeros((1, fg_sorted.shape[1]))
    i = torch.arange(1, n + 1, device=fg_sorted.device).unsqueeze(1)
    I, U = (G - F).double(), (G + i - F).double()
    bg = torch.where(i == 1, 1.0 - I / U, I / (U * (U - 1.0).clamp(min=1.0)))
    return torch.where(fg_sorted, 1.0 / U, bg) * valid_sorted


def lovasz_softmax_torch(logits, labels, ignore_index=None, loss_weight=1.0):
    """Multiclass Lovasz-Softmax of (N, C) logits as one torch composition; the gradient flows through the errors, the
    weights are constants (as in the reference, where they come from the sorted labels alone)."""
    n, c = logits.shape
    p = logits.softmax(dim=1)
    valid = (labels >= 0) & (labels < c)
    if ignore_index is not None:
        valid = valid & (labels != ignore_index)
    fg = (labels.unsqueeze(1) == torch.arange(c, device=labels.device)) & valid.unsqueeze(1)
    err = (fg.to(p.dtype) - p).abs()
    # ascending -err = descending err; rows that are not valid last; stable: ties by point index
    key = torch.where(valid.unsqueeze(1), -err.detach(), torch.ones_like(err))
    order = torch.sort(key, dim=0, stable=True).indices
    fg_s, valid_s = fg.gather(0, order), valid[order]
    g = lovasz_weights(fg_s, valid_s)
    per_class = (err.gather(0, order).double() * g).sum(0)
    present = fg.any(0)
    total = (per_class * present).sum() / present.sum().clamp(min=1)
    return (total * loss_weight).to(logits.dtype)


@LOSSES.register_module()
class LovaszLoss(nn.Module):
    def __init__(self, mode, class_seen=None, per_image=False, ignore_index=None, loss_weight=1.0):
        assert mode in {BINARY_MODE, MULTILABEL_MODE, MULTICLASS_MODE}
        super().__init__()
        if mode != MULTICLASS_MODE:
            raise NotImplementedError(f"LovaszLoss: mode={mode!r} (the Lovasz hinge) is not built; only 'multiclass'")
        if per_image:
            raise NotImplementedError("LovaszLoss: per_image=True is not built")
        if class_seen is not None:
            raise NotImplementedError("LovaszLoss: class_seen is not built")
        self.mode = mode
        self.ignore_index = ignore_index
        self.per_image = per_image
        self.class_seen = class_seen
        self.loss_weight = loss_weight
        self.use_hip = True

    def forward(self, y_pred, y_true):
        if y_pred.dim() != 2:     # (B, C, d1, ...) -> (P, C), lovasz.py:167-184
            c = y_pred.shape[1]
            y_pred = torch.movedim(y_pred, 1, -1).reshape(-1, c)
        y_true = y_true.reshape(-1)
        n, c = y_pred.shape
        if self.use_hip and y_pred.is_cuda and y_pred.is_floating_point():
            from ptv3_hip import autograd as A, ops
            if ops.seg_loss_capable(n, c):
                return A.lovasz_softmax(y_pred.float(), y_true.long(), self.ignore_index, self.loss_weight)
        return lovasz_softmax_torch(y_pred, y_true, self.ignore_index, self.loss_weight)
