"""OffsetKeypointOctFormer: per-point offsets and mask logits on the OctFormer backbone, on MI355X.

Counterpart of the reference's pointcept/models/offset_keypoint_octformer.py:25-206
(configs/my_dataset/offset_keypoint_octformer.py): the same constructor arguments, attribute names and state_dict keys,
the same output dict (the training curves stay device scalars instead of .item() reads).  In eval the head is two
ptv3_gemm calls with the BatchNorm and ReLU folded into the first.
"""
import torch
import torch.nn as nn

from pointcept.models.builder import MODELS
from pointcept.models.octformer.octformer_v1m1_base import OctFormerBackbone
from ptv3_hip import ops


@MODELS.register_module("OffsetKeypointOctFormer")
class OffsetKeypointOctFormer(OctFormerBackbone):
    fused = True

    def __init__(self, in_channels=4, num_keypoints=6, hidden_dim=256, fpn_channels=168, channels=(96, 192, 384, 384),
                 num_blocks=(2, 2, 18, 2), num_heads=(6, 12, 24, 24), patch_size=26, stem_down=2, head_up=2, dilation=4,
                 drop_path=0.5, nempty=True, octree_scale_factor=10.24, octree_depth=11, octree_full_depth=2, **kwargs):
        super().__init__()
        self.num_keypoints = num_keypoints
        self._build_backbone(in_channels, fpn_channels, channels, num_blocks, num_heads, patch_size, stem_down, head_up,
                             dilation, drop_path, nempty, octree_scale_factor, octree_depth, octree_full_depth)
        self.head = nn.Sequential(nn.Linear(fpn_channels, hidden_dim), nn.BatchNorm1d(hidden_dim), nn.ReLU(inplace=True),
                                  nn.Linear(hidden_dim, num_keypoints * 4))
        self.reg_criterion = nn.L1Loss(reduction="none")
        self.cls_criterion = nn.BCEWithLogitsLoss(reduction="none")

    def set_fused(self, fused):
        self.fused = bool(fused)
        return super().set_fused(fused)

    def forward(self, data_dict, taps=None):
        feats = self.backbone(data_dict, taps)
        h0, bn, _, h3 = self.head
        if self.fused and not self.training and feats.is_cuda and h0.in_features % 4 == 0 and h0.out_features % 4 == 0:
            scale, shift = ops.fold_batchnorm(bn, h0.bias)
            hidden = ops.gemm(feats.contiguous(), h0.weight, bn_scale=scale, bn_shift=shift, act=ops.ACT_RELU)
            pred_flat = ops.gemm(hidden, h3.weight, bias=h3.bias)
        else:
            pred_flat = self.head(feats)
        pred = pred_flat.view(-1, self.num_keypoints, 4)

        result_dict = {}
        if "target" in data_dict:
            target = data_dict["target"]
            offset_gt, mask_gt = target[..., :3], target[..., 3]
            offset_pred, mask_logits = pred[..., :3], pred[..., 3]
            cls_loss = self.cls_criterion(mask_logits, mask_gt).mean()
            valid = (mask_gt > 0.5).float()
            valid_exp = valid.unsqueeze(-1)
            reg_loss = (self.reg_criterion(offset_pred, offset_gt) * valid_exp).sum() / (valid_exp.sum() * 3 + 1e-6)
            result_dict["loss"] = cls_loss + reg_loss * 2.0
            if self.training:
                with torch.no_grad():
                    result_dict["train/cls_loss"] = cls_loss.detach()
                    result_dict["train/reg_loss"] = reg_loss.detach()
                    result_dict["train/offset_l1_err"] = ((torch.abs(offset_pred - offset_gt) * valid_exp).sum()
                                                          / (valid_exp.sum() * 3 + 1e-6))
                    dist = torch.norm(offset_pred - offset_gt, p=2, dim=-1)
                    if "scale" in data_dict:
                        scale = data_dict["scale"]
                        if scale.ndim == 0:
                            scale = scale.view(1)
                        if scale.ndim == 1 and len(scale) > 1:
                            dist = dist * scale[levels_batch(data_dict["offset"], dist.shape[0])].unsqueeze(-1)
                        else:
                            dist = dist * scale.view(-1, 1)
                    count = valid.sum(dim=0)
                    kp = (dist * valid).sum(dim=0) / count.clamp(min=1e-6)
                    kp = torch.where(count == 0, torch.zeros_like(kp), kp)
                    result_dict["train/mean_dist"] = kp.mean()
                    for i in range(self.num_keypoints):
                        result_dict[f"train/kp{i}_dist"] = kp[i]
        if not self.training:
            final_pred = pred.clone()
            final_pred[..., 3] = torch.sigmoid(pred[..., 3])
            result_dict["pred"] = final_pred
        return result_dict


def levels_batch(offset, n):
    """offset2batch: the scene of every one of the n points"""
    return torch.searchsorted(offset.long(), torch.arange(n, device=offset.device), right=True)
