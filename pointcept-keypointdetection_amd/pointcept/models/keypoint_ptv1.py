"""KeypointPTv1: global-regression keypoint head on a Point Transformer V1 encoder, on MI355X.

Counterpart of the reference's pointcept/models/keypoint_ptv1.py:7-189 (configs/my_dataset/keypoint_ptv1.py): same
constructor arguments, `enc1..enc5` / `reg_head` attribute names and state_dict keys, the same output dict, and the
registry names KeypointPTv1, KeypointPTv1-26 / -38 / -50.  Five encoder stages (TransitionDown + Bottlenecks, strides
1, 4, 4, 4, 4), the per-scene mean of the last stage's points, then the regression head shared with KeypointPTv3.
Eval: `offset` is read from the device once; every stage's sample counts follow on the host and the rest of the
forward queues kernels only (farthest point sampling, kNN, grouping, ptv3_gemm, ptv3_vector_attn_fwd,
ptv3_scene_mean_head).  Training: the torch composition of the same formulas (batch-statistic BatchNorm) over the HIP
neighbour search and grouping, and the taped HIP head.  fp32 throughout, as the reference runs this config.
"""
import torch
import torch.nn as nn

from pointcept.models.builder import MODELS
from pointcept.models.point_transformer.point_transformer_seg import TransitionDown, Bottleneck, SceneOffsets
from pointcept.models.keypoint_ptv3 import make_reg_head, check_scene_count, regress, loss_and_metrics
from pointcept.models.utils.hip_layers import check_sync_batchnorm


PLANES = (32, 64, 128, 256, 512)     # stage widths
STRIDES = (1, 4, 4, 4, 4)            # points kept: one in `stride`, per scene, by farthest point sampling
NSAMPLE = (8, 16, 16, 16, 16)        # neighbours of the stage's TransitionDown and attention layers
SHARE_PLANES = 8


@MODELS.register_module()
class KeypointPTv1(nn.Module):
    def __init__(self, block=Bottleneck, blocks=[1, 2, 3, 5, 2], in_channels=6, num_keypoints=6, hidden_dim=256,
                 **kwargs):
        super().__init__()
        self.in_channels, self.num_keypoints = in_channels, num_keypoints
        self.strides = list(STRIDES)
        self.in_planes = in_channels      # width entering the next stage; ends at the backbone's output width
        for i, depth in enumerate(blocks):
            self.add_module(f"enc{i + 1}", self._make_enc(block, PLANES[i], depth, SHARE_PLANES, STRIDES[i], NSAMPLE[i]))
        self.reg_head = make_reg_head(self.in_planes, hidden_dim, num_keypoints)
        self.criterion = nn.MSELoss()

    def _make_enc(self, block, planes, blocks, share_planes=8, stride=1, nsample=16):
        """One stage: the TransitionDown counts as its first block (keypoint_ptv1.py:81), `blocks - 1` attention
        blocks follow at the stage's width."""
        width = planes * block.expansion
        stage = nn.Sequential(TransitionDown(self.in_planes, width, stride, nsample))
        for _ in range(blocks - 1):
            stage.append(block(width, width, share_planes, nsample=nsample))
        self.in_planes = width
        return stage

    def set_fused(self, fused):
        """fused = False: eval runs the training path's torch composition (running-statistic BatchNorm) instead of the
        fused kernels - what the fused path is tested against."""
        for m in self.modules():
            if hasattr(m, "fused"):
                m.fused = bool(fused)
        return self

    def forward(self, data_dict):
        check_sync_batchnorm(self)
        check_scene_count(self, data_dict["offset"])
        p0 = data_dict["coord"]
        ends = data_dict["offset"].tolist()   # the forward's one read from the device
        shrink = 1
        for s in self.strides:
            shrink *= s
        for i, (a, b) in enumerate(zip([0] + ends[:-1], ends)):
            if b - a < shrink:
                raise ValueError(f"KeypointPTv1: scene {i} has {b - a} points, fewer than the {shrink} that leave one "
                                 "point at stage 5 (its mean would divide by zero)")
        levels = SceneOffsets.chain(ends, p0.device, self.strides[1:])
        x0 = p0 if self.in_channels == 3 else torch.cat((p0, data_dict["feat"]), 1)
        pxo = [p0.float().contiguous(), x0.float().contiguous(), levels[0].dev, levels[0]]
        for i in range(5):
            pxo = getattr(self, f"enc{i + 1}")(pxo)
        pred = regress(self.reg_head, pxo[1], pxo[2], self.training).view(-1, self.num_keypoints, 3)
        return loss_and_metrics(pred, data_dict, self.num_keypoints, self.training)


def _fixed_depth(name, depths):
    """A registry name with its stage depths fixed (the reference's -26 / -38 / -50 subclasses)."""
    def __init__(self, **kwargs):
        KeypointPTv1.__init__(self, blocks=list(depths), **kwargs)
    cls = type(name.replace("-", "_"), (KeypointPTv1,), {"__init__": __init__, "__module__": __name__})
    return MODELS.register_module(name)(cls)


KeypointPTv1_26 = _fixed_depth("KeypointPTv1-26", (1, 1, 1, 1, 1))
KeypointPTv1_38 = _fixed_depth("KeypointPTv1-38", (1, 2, 2, 2, 2))
KeypointPTv1_50 = _fixed_depth("KeypointPTv1-50", (1, 2, 3, 5, 2))
