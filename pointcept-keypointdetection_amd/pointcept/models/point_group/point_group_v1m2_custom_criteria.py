"""PointGroup with a configurable segmentation loss ("PG-v1m2", reference
pointcept/models/point_group/point_group_v1m2_custom_criteria.py): `criteria` builds the loss (:62), `freeze_backbone`
stops the backbone's gradients (:63-66), `return_point` hands back the backbone's Point (:69-70), and a decoder-less
backbone's levels are unrolled through `pooling_parent` / `pooling_inverse` (:76-83).  Everything else is PG-v1m1."""
from pointcept.models.builder import MODELS
from pointcept.models.default import _full_resolution
from pointcept.models.losses import build_criteria
from .point_group_v1m1_base import PointGroupBase


@MODELS.register_module("PG-v1m2")
class PointGroupV1m2(PointGroupBase):
    def __init__(self, backbone, backbone_out_channels=64, semantic_num_classes=20, semantic_ignore_index=-1,
                 segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1, cluster_thresh=1.5,
                 cluster_closed_points=300, cluster_propose_points=100, cluster_min_points=50, voxel_size=0.02,
                 criteria=None, freeze_backbone=False):
        super().__init__(backbone, backbone_out_channels, semantic_num_classes, semantic_ignore_index,
                         segment_ignore_index, instance_ignore_index, cluster_thresh, cluster_closed_points,
                         cluster_propose_points, cluster_min_points, voxel_size)
        self.seg_criteria = build_criteria(criteria)
        self.freeze_backbone = freeze_backbone
        if self.freeze_backbone:
            for p in self.backbone.parameters():
                p.requires_grad = False

    def _features(self, data_dict):
        return _full_resolution(self.backbone(data_dict))[1]

    def _seg_loss(self, logit_pred, segment):
        return self.seg_criteria(logit_pred, segment)

    def forward(self, data_dict, return_point=False):
        if return_point:
            return dict(point=self.backbone(data_dict))
        return super().forward(data_dict)
