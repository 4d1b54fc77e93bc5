"""RegressionL1Loss: the L1 loss of the fork's body-size-and-weight regression (the reference's
pointcept/models/losses/weight_regression_loss.py:23-38, built by configs/my_dataset/ptv3_weight.py:43).  Plain torch
and therefore usable on CPU tensors; a classifier whose criteria is exactly one of these computes the same number inside
its fused head kernel instead (csrc/cls_head.hip)."""
import torch.nn as nn

from .builder import LOSSES


@LOSSES.register_module()
class RegressionL1Loss(nn.Module):
    def __init__(self, loss_weight=1.0):
        super().__init__()
        self.loss_weight = loss_weight
        self.criterion = nn.L1Loss()

    def forward(self, pred, target):
        # the literal view(-1, 7) of the reference: a numel that 7 does not divide raises here as it does there
        return self.criterion(pred.view(-1, 7), target.view(-1, 7)) * self.loss_weight
