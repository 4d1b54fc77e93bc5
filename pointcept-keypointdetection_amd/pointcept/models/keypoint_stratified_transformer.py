"""KeypointStratifiedTransformer: global-regression keypoint head on the Stratified Transformer backbone, on MI355X.

Counterpart of the reference's pointcept/models/keypoint_stratified_transformer.py:10-114
(configs/my_dataset/keypoint_stratified_transformer.py): the same constructor arguments, attribute names and state_dict
keys (the classifier is an Identity, so it owns none), the same output dict.  The backbone's point features are averaged
per scene and regressed by the head shared with KeypointPTv3: one ptv3_scene_mean_head call in eval, the taped HIP
layers in training.
"""
import torch.nn as nn

from pointcept.models.builder import MODELS
from pointcept.models.keypoint_ptv3 import make_reg_head, check_scene_count, regress, loss_and_metrics
from pointcept.models.stratified_transformer.stratified_transformer_v1m2_refine import StratifiedTransformer


@MODELS.register_module("KeypointStratifiedTransformer")
class KeypointStratifiedTransformer(StratifiedTransformer):
    def __init__(self, num_keypoints=6, hidden_dim=256, **kwargs):
        super().__init__(num_classes=num_keypoints, **kwargs)
        self.classifier = nn.Identity()
        in_channels = kwargs["channels"][0] if "channels" in kwargs else 48
        self.num_keypoints = num_keypoints
        self.reg_head = make_reg_head(in_channels, hidden_dim, num_keypoints)
        self.criterion = nn.MSELoss()

    def forward(self, data_dict):
        check_scene_count(self, data_dict["offset"])
        feats, so = self.backbone(data_dict)
        pred = regress(self.reg_head, feats, so.dev, self.training).view(-1, self.num_keypoints, 3)
        return loss_and_metrics(pred, data_dict, self.num_keypoints, self.training)
