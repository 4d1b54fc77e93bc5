"""KeypointSparseUNet: global-regression keypoint head on the SpUNet-v1m1 backbone, on MI355X.

Counterpart of the reference's pointcept/models/keypoint_sparse_unet.py:14-152 (configs/my_dataset/
keypoint_sparse_unet.py): a subclass of SpUNetBase built with num_classes = 0 (a `num_classes` in the config is dropped),
`final` an nn.Identity, the per-scene mean of the decoder's output on the input sites - or, with enc_mode = True, of the
deepest encoder level -, the `reg_head` shared with KeypointPTv3 (ptv3_scene_mean_head in eval), MSE loss (in eval too,
when the batch carries `target`) and the train/mean_dist, train/kp{i}_dist curves.  Eval reads the device five times:
spatial shape and offsets at entry, then the coarse row count of each of the four stages.
"""
import torch.nn as nn

from pointcept.models.builder import MODELS
from pointcept.models.sparse_unet.spconv_unet_v1m1_base import SpUNetBase
from pointcept.models.keypoint_ptv3 import make_reg_head, check_scene_count, regress, loss_and_metrics
from pointcept.models.utils.hip_layers import check_sync_batchnorm


@MODELS.register_module("KeypointSparseUNet")
class KeypointSparseUNet(SpUNetBase):
    def __init__(self, num_keypoints=6, hidden_dim=256, **kwargs):
        kwargs.pop("num_classes", None)
        super().__init__(num_classes=0, **kwargs)
        self.final = nn.Identity()
        in_channels = self.channels[self.num_stages - 1] if self.enc_mode else self.channels[-1]
        self.num_keypoints = num_keypoints
        self.reg_head = make_reg_head(in_channels, hidden_dim, num_keypoints)
        self.criterion = nn.MSELoss()

    def forward(self, input_dict, taps=None):
        check_sync_batchnorm(self)
        check_scene_count(self, input_dict["offset"])
        x, ends = self.backbone(input_dict, taps)
        pred = regress(self.reg_head, x.features, ends, self.training).view(-1, self.num_keypoints, 3)
        return loss_and_metrics(pred, input_dict, self.num_keypoints, self.training)
