"""KeypointOACNNs: global-regression keypoint head on the OA-CNNs backbone, on MI355X.

Counterpart of the reference's pointcept/models/keypoint_oa_cnns.py:11-142 (configs/my_dataset/keypoint_oa_cnns.py): a
subclass of OACNNs with the same constructor arguments, `final` replaced by nn.Identity, the per-scene mean of the
decoder's output on the input sites, the `reg_head` shared with KeypointPTv3 (ptv3_scene_mean_head in eval), MSE loss
and the train/mean_dist, train/kp{i}_dist curves.  Eval reads the device five times: spatial shape and offsets at entry,
then the coarse row count of each of the four stages.
"""
import torch.nn as nn

from pointcept.models.builder import MODELS
from pointcept.models.oacnns import OACNNs
from pointcept.models.keypoint_ptv3 import make_reg_head, check_scene_count, regress, loss_and_metrics
from pointcept.models.utils.hip_layers import check_sync_batchnorm


@MODELS.register_module("KeypointOACNNs")
class KeypointOACNNs(OACNNs):
    def __init__(self, num_keypoints=6, hidden_dim=256, **kwargs):
        super().__init__(num_classes=num_keypoints, **kwargs)
        self.final = nn.Identity()
        in_channels = kwargs["dec_channels"][0] if "dec_channels" in kwargs else 96
        self.num_keypoints = num_keypoints
        self.reg_head = make_reg_head(in_channels, hidden_dim, num_keypoints)
        self.criterion = nn.MSELoss()

    def forward(self, input_dict, taps=None):
        check_sync_batchnorm(self)
        check_scene_count(self, input_dict["offset"])
        x, _ = self.backbone(input_dict, taps)
        pred = regress(self.reg_head, x.features, input_dict["offset"], self.training).view(-1, self.num_keypoints, 3)
        return loss_and_metrics(pred, input_dict, self.num_keypoints, self.training)
