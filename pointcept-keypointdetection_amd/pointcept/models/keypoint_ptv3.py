"""KeypointPTv3: global-regression keypoint head on the MI355X PTv3 backbone.

Counterpart of the reference's pointcept/models/keypoint_ptv3.py:7-98: same constructor (backbone_conf,
num_keypoints=6, hidden_dim=256), same `reg_head.{0,1,4,6}` parameters, same output dict.  Each scene's point features
are averaged into one row (torch_scatter.scatter_mean, :44) and a small MLP regresses the K keypoints from it.
Eval: ptv3_scene_mean_head - pooling and the whole fp32 head in two launches on the caller's stream.  Training: the
taped scene-mean Function, then one taped HIP Function per head layer (batch-statistic BatchNorm) and torch's Dropout.
Every scalar entry of the result is a detached 0-d device tensor (no `.item()` in forward).
The helpers below are shared with KeypointSwin3D (keypoint_swin3d.py).
"""
import torch
import torch.nn as nn

from ptv3_hip import ops
from ptv3_hip import autograd as A
from pointcept.models.builder import MODELS, build_model
from pointcept.models.utils.hip_layers import Linear, BatchNorm1d, ReLU, check_sync_batchnorm


def make_reg_head(in_channels, hidden_dim, num_keypoints):
    """reg_head of keypoint_ptv3.py:24-32 / keypoint_swin3d.py:30-38 (same module indices, so the same state_dict)."""
    return nn.Sequential(
        Linear(in_channels, hidden_dim),
        BatchNorm1d(hidden_dim),
        ReLU(inplace=True),
        nn.Dropout(0.3),
        Linear(hidden_dim, hidden_dim),
        ReLU(inplace=True),
        Linear(hidden_dim, num_keypoints * 3),
    )


def check_scene_count(model, offset, bn=None):
    """nn.BatchNorm1d refuses one row per channel in training (the reference fails there with one scene per batch);
    B = len(offset) is a host-side shape, so this needs no synchronisation.  bn: the first BatchNorm behind the pooling
    (default: reg_head[1]; DefaultClassifier hands in cls_head[1])."""
    bn = model.reg_head[1] if bn is None else bn
    if model.training and bn.training and offset.shape[0] == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size "
                         f"{torch.Size([1, bn.num_features])}")


def _wt(lin):
    return lin._cache.get("wt", [lin.weight], lambda: lin.weight.detach().float().t().contiguous())


def regress(head, feat, offset, training):
    """(B, 3K) fp32 = reg_head(per-scene mean of feat (N, C))."""
    if training:
        g = A.scene_mean(feat, offset)
        h = head[1](head[0](g), act=ops.ACT_RELU)      # Linear -> BatchNorm1d (batch statistics) + reg_head[2] ReLU
        h = head[5](head[4](head[3](h)))               # Dropout -> Linear -> ReLU
        return head[6](h)
    scale, shift = head[1].folded()
    return ops.scene_mean_head(feat.contiguous(), offset, _wt(head[0]), head[0].bias_f32(), scale, shift,
                               _wt(head[4]), head[4].bias_f32(), _wt(head[6]), head[6].bias_f32())


def loss_and_metrics(pred, data_dict, num_keypoints, training):
    """The result dict of keypoint_ptv3.py:50-98 (keypoint_swin3d.py:124-156): MSE loss against the collated (B*K, 3)
    target; in training the distance curves (scaled by `scale` when the batch carries it); in eval `pred`."""
    result = {}
    if "target" in data_dict:
        target = data_dict["target"]
        pred_for_loss = pred if pred.shape == target.shape else pred.view(-1, 3)
        result["loss"] = nn.functional.mse_loss(pred_for_loss, target)
        if training:
            with torch.no_grad():
                k = num_keypoints
                dist = torch.norm(pred.view(-1, k, 3) - target.view(-1, k, 3), p=2, dim=-1)   # (B, K)
                if "scale" in data_dict:
                    scale = data_dict["scale"]
                    if scale.ndim == 1:
                        scale = scale.view(-1, 1)
                    dist = dist * scale
                result["train/mean_dist"] = dist.mean()
                kp = dist.mean(dim=0)
                for i in range(k):
                    result[f"train/kp{i}_dist"] = kp[i]
    if not training:
        result["pred"] = pred
    return result


@MODELS.register_module()
class KeypointPTv3(nn.Module):
    def __init__(self, backbone_conf, num_keypoints=6, hidden_dim=256):
        super().__init__()
        self.backbone = build_model(backbone_conf)
        in_channels = backbone_conf["dec_channels"][0]
        self.num_keypoints = num_keypoints
        self.reg_head = make_reg_head(in_channels, hidden_dim, num_keypoints)
        self.criterion = nn.MSELoss()

    def forward(self, data_dict):
        check_sync_batchnorm(self)
        check_scene_count(self, data_dict["offset"])
        point = self.backbone(data_dict)
        pred = regress(self.reg_head, point.feat, point.offset, self.training).view(-1, self.num_keypoints, 3)
        return loss_and_metrics(pred, data_dict, self.num_keypoints, self.training)
