"""KeypointOctFormer: global-regression keypoint head on the OctFormer backbone, on MI355X.

Counterpart of the reference's pointcept/models/keypoint_octformer.py:27-217 (configs/my_dataset/keypoint_octformer.py):
the same constructor arguments, attribute names and state_dict keys, the same output dict.  The decoder's features,
interpolated to the input points, are averaged per scene and regressed by the head shared with KeypointPTv3: one
ptv3_scene_mean_head call in eval, the taped HIP layers in training.
"""
import torch.nn as nn

from pointcept.models.builder import MODELS
from pointcept.models.keypoint_ptv3 import make_reg_head, check_scene_count, regress, loss_and_metrics
from pointcept.models.octformer.octformer_v1m1_base import OctFormerBackbone


@MODELS.register_module("KeypointOctFormer")
class KeypointOctFormer(OctFormerBackbone):
    def __init__(self, in_channels=4, num_keypoints=6, hidden_dim=256, fpn_channels=168, channels=(96, 192, 384, 384),
                 num_blocks=(2, 2, 18, 2), num_heads=(6, 12, 24, 24), patch_size=26, stem_down=2, head_up=2, dilation=4,
                 drop_path=0.5, nempty=True, octree_scale_factor=10.24, octree_depth=11, octree_full_depth=2, **kwargs):
        super().__init__()
        self.num_keypoints = num_keypoints
        self._build_backbone(in_channels, fpn_channels, channels, num_blocks, num_heads, patch_size, stem_down, head_up,
                             dilation, drop_path, nempty, octree_scale_factor, octree_depth, octree_full_depth)
        self.reg_head = make_reg_head(fpn_channels, hidden_dim, num_keypoints)
        self.criterion = nn.MSELoss()

    def forward(self, data_dict, taps=None):
        check_scene_count(self, data_dict["offset"])
        feats = self.backbone(data_dict, taps)
        pred = regress(self.reg_head, feats, data_dict["offset"], self.training).view(-1, self.num_keypoints, 3)
        return loss_and_metrics(pred, data_dict, self.num_keypoints, self.training)
