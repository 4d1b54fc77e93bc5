"""KeypointPTv2: global-regression keypoint head on a Point Transformer V2 backbone, on MI355X.

Counterpart of the reference's pointcept/models/keypoint_ptv2.py:17-133 (configs/my_dataset/keypoint_ptv2.py): same
constructor arguments, `backbone` / `reg_head` attribute names and state_dict keys, the same output dict, registry name
KeypointPTv2.  The backbone (PT-v2m2 with num_classes = 0) returns the per-point features of its last decoder stage;
their per-scene mean goes through the regression head shared with KeypointPTv3 (ptv3_scene_mean_head in eval).
Host reads of an eval forward: `offset` once at entry and one pooled row count per GridPool.
"""
import torch.nn as nn

from pointcept.models.builder import MODELS, build_model
from pointcept.models.keypoint_ptv3 import make_reg_head, check_scene_count, regress, loss_and_metrics
from pointcept.models.point_transformer.point_transformer_seg import SceneOffsets
from pointcept.models.utils.hip_layers import check_sync_batchnorm


@MODELS.register_module("KeypointPTv2")
class KeypointPTv2(nn.Module):
    def __init__(self, backbone_conf, num_keypoints=6, hidden_dim=256):
        super().__init__()
        self.backbone = build_model(backbone_conf)
        in_channels = backbone_conf["dec_channels"][0] if "dec_channels" in backbone_conf else 256
        self.num_keypoints = num_keypoints
        self.reg_head = make_reg_head(in_channels, hidden_dim, num_keypoints)
        self.criterion = nn.MSELoss()

    def set_fused(self, fused):
        self.backbone.set_fused(fused)
        return self

    def forward(self, data_dict):
        check_sync_batchnorm(self)
        check_scene_count(self, data_dict["offset"])
        so = SceneOffsets.read(data_dict["offset"])       # the forward's one read of `offset`
        for i, (a, b) in enumerate(zip([0] + so.host[:-1], so.host)):
            if b - a < 1:
                raise ValueError(f"KeypointPTv2: scene {i} has no points (its mean would divide by zero)")
        feat = self.backbone(dict(data_dict, scene_offsets=so))
        pred = regress(self.reg_head, feat, so.dev, self.training).view(-1, self.num_keypoints, 3)
        return loss_and_metrics(pred, data_dict, self.num_keypoints, self.training)
