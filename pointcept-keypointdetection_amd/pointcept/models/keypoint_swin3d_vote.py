"""KeypointSwin3DVote: per-point keypoint votes on the Swin3D backbone, aggregated by a per-scene median.

Counterpart of the reference's pointcept/models/keypoint_swin3d_plus.py:16-189: same constructor (backbone_conf,
num_keypoints=6, hidden_dim=256, vote_radius=0.4), same `vote_head.{0,1,4,5,7}` parameters, same output dicts.  Every
point predicts K offsets; its votes are `coord + offset` (:84).
Eval: the head with folded BatchNorm, then ptv3_scene_median with the coord add inside the kernel - the (N, K, 3) votes
are never materialised, and the per-scene mask / gather / median loop (:166-189) with its host synchronisations is one
exact radix select on the caller's stream.  Training: the taped head layers and torch's Dropout, then VoteLossFn - the
masked smooth-L1 loss and the 1 + K distance curves (:86-164) in two launches, its backward in one.
B is len(offset) (the reference reads batch_idx.max() back); every scalar of the result is a 0-d device tensor.
"""
import torch.nn as nn

from ptv3_hip import ops
from ptv3_hip import autograd as A
from pointcept.models.utils.hip_layers import Linear, BatchNorm1d, ReLU, check_sync_batchnorm
from .builder import MODELS, build_model
from .offset_keypoint_swin3d import build_coord_feat
from .swin3d import Swin3DUNet


@MODELS.register_module("KeypointSwin3DVote")
class KeypointSwin3DVote(nn.Module):
    def __init__(self, backbone_conf, num_keypoints=6, hidden_dim=256, vote_radius=0.4):
        super().__init__()
        self.backbone = build_model(backbone_conf)
        self.num_keypoints = num_keypoints
        self.vote_radius = vote_radius
        in_channels = backbone_conf["channels"][0] if "channels" in backbone_conf else 96
        self.vote_head = nn.Sequential(
            Linear(in_channels, hidden_dim),
            BatchNorm1d(hidden_dim),
            ReLU(inplace=True),
            nn.Dropout(0.3),
            Linear(hidden_dim, hidden_dim),
            BatchNorm1d(hidden_dim),
            ReLU(inplace=True),
            Linear(hidden_dim, num_keypoints * 3),
        )

    def votes(self, feat):
        """(N, 3K) fp32 raw offsets.  Each BatchNorm1d call carries the ReLU behind it (folded scale / shift in eval,
        batch statistics in training); Dropout is torch's (the identity in eval)."""
        h = self.vote_head
        x = h[1](h[0](feat.contiguous()), act=ops.ACT_RELU)
        x = h[5](h[4](h[3](x)), act=ops.ACT_RELU)
        return h[7](x).float()

    def forward(self, data_dict):
        check_sync_batchnorm(self)
        if "coord_feat" not in data_dict and isinstance(self.backbone, Swin3DUNet):
            build_coord_feat(self.backbone, data_dict)
        coord, offset = data_dict["coord"], data_dict["offset"]
        votes = self.votes(self.backbone(data_dict))
        if not self.training:
            pred = ops.scene_median(votes, coord.float().contiguous(), offset)
            return dict(pred=pred.view(-1, self.num_keypoints, 3))
        loss, curves, _ = A.vote_loss(votes, coord.float(), data_dict["target"].float(), offset, self.vote_radius,
                                      data_dict["scale"].float() if "scale" in data_dict else None)
        result = {"loss": loss, "train/masked_dist_err": curves[0]}
        for k in range(self.num_keypoints):
            result[f"train/kp{k}_dist_err"] = curves[1 + k]
        return result
