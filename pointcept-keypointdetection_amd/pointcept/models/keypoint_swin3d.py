"""KeypointSwin3D: global-regression keypoint head on the Swin3D backbone.

Counterpart of the reference's pointcept/models/keypoint_swin3d.py:10-156: same constructor, `reg_head.{0,1,4,6}`
parameters, loss, curves and output dict as KeypointPTv3 (whose helpers it uses).  `coord_feat` is built as
OffsetKeypointSwin3D builds it (:45-70).  The per-scene mean loop over `offset` (:80-117) is the scene-mean kernel.
The reference's fallback for a backbone that returns fewer rows than points (:90-115) cannot trigger here: Swin3DUNet
returns one row per input point (swin3d_v1m1_base.py forward), which is asserted instead.
"""
import torch.nn as nn

from pointcept.models.utils.hip_layers import check_sync_batchnorm
from .builder import MODELS, build_model
from .keypoint_ptv3 import make_reg_head, check_scene_count, regress, loss_and_metrics
from .offset_keypoint_swin3d import build_coord_feat


@MODELS.register_module()
class KeypointSwin3D(nn.Module):
    def __init__(self, backbone_conf, num_keypoints=6, hidden_dim=256):
        super().__init__()
        self.backbone = build_model(backbone_conf)
        in_channels = backbone_conf["channels"][0] if "channels" in backbone_conf else 96
        self.num_keypoints = num_keypoints
        self.reg_head = make_reg_head(in_channels, hidden_dim, num_keypoints)
        self.criterion = nn.MSELoss()

    def forward(self, data_dict):
        check_sync_batchnorm(self)
        check_scene_count(self, data_dict["offset"])
        build_coord_feat(self.backbone, data_dict)
        feat = self.backbone(data_dict)
        n = data_dict["coord_feat"].shape[0]
        assert feat.shape[0] == n, f"KeypointSwin3D: backbone returned {feat.shape[0]} rows for {n} points"
        pred = regress(self.reg_head, feat, data_dict["offset"], self.training).view(-1, self.num_keypoints, 3)
        return loss_and_metrics(pred, data_dict, self.num_keypoints, self.training)
