"""PointGroup instance segmentation ("PG-v1m1", reference pointcept/models/point_group/point_group_v1m1_base.py).

Constructor keywords, state_dict and the returned keys are the reference's.  The heads run on the library's Linear /
BatchNorm kernels.  The evaluation tail (:101-178) - ball query, copy of the neighbour lists, host search, dense mask
scatter, one masked mean and one copy per proposal - is ptv3_pg_cluster + ptv3_pg_proposals on the device (DESIGN.md
section 22): one read-back of a four-integer record decides the output shapes, and the three results are copied to the
host at the end because the reference returns CPU tensors (set_device_results(True) leaves them on the device).  When a point has more than 1000 neighbours the lists the
reference searches are cut and its graph is directed; clustering then takes the list path (pointgroup_ops), which
reproduces that search.  In training the two bias losses (:75-89) are one forward and one backward launch
(ptv3_pg_bias_loss_fwd / _bwd).  set_fused(False) takes the list path always and composes the bias losses in torch.

Differences, all on paths the reference cannot finish: with no point kept the reference indexes a 1-d tensor with two
indices (:120, :149) and raises; here the empty results it was heading for are returned.
"""
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from pointcept.models.utils.hip_layers import Linear, BatchNorm1d, ReLU
from pointcept.models.builder import MODELS, build_model
from ptv3_hip import ops
from ptv3_hip import autograd as A


class PointGroupBase(nn.Module):
    def __init__(self, backbone, backbone_out_channels=64, semantic_num_classes=20, semantic_ignore_index=-1,
                 segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1, cluster_thresh=1.5,
                 cluster_closed_points=300, cluster_propose_points=100, cluster_min_points=50, voxel_size=0.02):
        super().__init__()
        norm_fn = partial(BatchNorm1d, eps=1e-3, momentum=0.01)
        self.semantic_num_classes = semantic_num_classes
        self.segment_ignore_index = segment_ignore_index
        self.semantic_ignore_index = semantic_ignore_index
        self.instance_ignore_index = instance_ignore_index
        self.cluster_thresh = cluster_thresh
        self.cluster_closed_points = cluster_closed_points
        self.cluster_propose_points = cluster_propose_points
        self.cluster_min_points = cluster_min_points
        self.voxel_size = voxel_size
        self.backbone = build_model(backbone)
        self.bias_head = nn.Sequential(
            Linear(backbone_out_channels, backbone_out_channels),
            norm_fn(backbone_out_channels),
            ReLU(),
            Linear(backbone_out_channels, 3),
        )
        self.seg_head = Linear(backbone_out_channels, semantic_num_classes)
        self._fused = True
        self._device_results = False

    def set_device_results(self, on=True):
        """True: eval leaves pred_scores / pred_masks / pred_classes on the device (InsSegEvaluator reads them there);
        the default returns CPU tensors, as the reference does."""
        self._device_results = bool(on)
        return self

    def set_fused(self, on=True):
        """False: cluster through pointgroup_ops' lists and host search (the composition the reference runs)."""
        self._fused = bool(on)
        return self

    # -- what the subclasses differ in ---------------------------------------------------------------------------
    def _features(self, data_dict):
        return self.backbone(data_dict)

    def _seg_loss(self, logit_pred, segment):
        raise NotImplementedError

    # -- :69-97 -------------------------------------------------------------------------------------------------
    def _losses(self, data_dict, coord, bias_pred, logit_pred):
        seg_loss = self._seg_loss(logit_pred, data_dict["segment"])
        if self._fused and self.training and bias_pred.is_cuda:
            # forward + backward of the two bias losses as two launches (ahead of the composition)
            bias_l1_loss, bias_cosine_loss = A.pg_bias_loss(bias_pred, coord, data_dict["instance_centroid"],
                                                            data_dict["instance"].long(), self.instance_ignore_index)
        else:
            mask = (data_dict["instance"] != self.instance_ignore_index).float()
            bias_gt = data_dict["instance_centroid"] - coord
            denom = torch.sum(mask) + 1e-8
            bias_dist = torch.sum(torch.abs(bias_pred - bias_gt), dim=-1)
            bias_l1_loss = torch.sum(bias_dist * mask) / denom
            pred_dir = bias_pred / (torch.norm(bias_pred, p=2, dim=1, keepdim=True) + 1e-8)
            gt_dir = bias_gt / (torch.norm(bias_gt, p=2, dim=1, keepdim=True) + 1e-8)
            bias_cosine_loss = torch.sum(-(pred_dir * gt_dir).sum(-1) * mask) / denom
        return dict(loss=seg_loss + bias_l1_loss + bias_cosine_loss, seg_loss=seg_loss, bias_l1_loss=bias_l1_loss,
                    bias_cosine_loss=bias_cosine_loss)

    # -- :101-178 -----------------------------------------------------------------------------------------------
    def cluster(self, center, segment_pred, keep, offset):
        """(cluster_idxs (sum, 2) int32 over the rows of `center`, cluster_offsets int32, proposals or None) on the
        device: the kept points of every scene clustered by label within cluster_thresh."""
        rows = keep.nonzero().view(-1)
        dev = center.device
        if rows.numel() == 0:
            return (torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                    rows, 0)
        center_ = center.index_select(0, rows).contiguous()
        label_ = segment_pred.index_select(0, rows).int()
        # kept points per scene -> offsets with the leading 0 (:126-127)
        offset_ = torch.searchsorted(rows, offset.to(rows.dtype).contiguous()).int()
        offset_ = F.pad(offset_, (1, 0)).contiguous()
        found = None
        if self._fused:
            found = ops.pg_cluster(center_, label_, offset_, self.cluster_thresh, self.cluster_min_points,
                                   self.cluster_propose_points)
        if found is None:
            from pointgroup_ops import ballquery_batch_p, bfs_cluster
            batch_ = torch.bucketize(torch.arange(rows.numel(), device=dev, dtype=torch.int32), offset_[1:],
                                     right=True).int()
            idx, start_len = ballquery_batch_p(center_, batch_, offset_, self.cluster_thresh, self.cluster_closed_points)
            idxs, offs = bfs_cluster(label_.cpu(), idx.cpu(), start_len.cpu(), self.cluster_min_points)
            large = int(((offs[1:] - offs[:-1]) > self.cluster_propose_points).sum())
            found = idxs.to(dev), offs.to(dev), large
        return found[0], found[1], rows, found[2]

    def _proposals(self, coord, bias_pred, logit_pred, offset):
        center = ((coord + bias_pred) / self.voxel_size).float().contiguous()
        prob = F.softmax(logit_pred.float(), dim=-1).contiguous()
        segment_pred = torch.max(prob, 1)[1]
        keep = torch.ones_like(segment_pred, dtype=torch.bool)
        for index in self.segment_ignore_index:
            keep &= segment_pred != index
        idxs, offs, rows, large = self.cluster(center, segment_pred, keep, offset)
        if large == 0:
            # the reference's empty results (:146-174 with no proposal left)
            return dict(pred_scores=torch.tensor([]), pred_masks=torch.zeros((0, coord.shape[0]), dtype=torch.int),
                        pred_classes=torch.tensor([]))
        classes, scores, masks = ops.pg_proposals(idxs.contiguous(), offs.contiguous(), prob, segment_pred,
                                                  self.cluster_propose_points, large, row_map=rows)
        if self._device_results:
            return dict(pred_scores=scores, pred_masks=masks, pred_classes=classes)
        return dict(pred_scores=scores.cpu(), pred_masks=masks.cpu(), pred_classes=classes.cpu())

    def forward(self, data_dict):
        coord = data_dict["coord"]
        offset = data_dict["offset"]
        feat = self._features(data_dict).contiguous()
        hidden = self.bias_head[2](self.bias_head[1](self.bias_head[0](feat)))
        bias_pred = self.bias_head[3](hidden)
        logit_pred = self.seg_head(feat)
        return_dict = dict()
        if "segment" in data_dict.keys() and "instance" in data_dict.keys():
            return_dict = self._losses(data_dict, coord, bias_pred, logit_pred)
        if not self.training:
            return_dict.update(self._proposals(coord, bias_pred, logit_pred, offset))
        return return_dict


@MODELS.register_module("PG-v1m1")
class PointGroup(PointGroupBase):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.ce_criteria = torch.nn.CrossEntropyLoss(ignore_index=self.semantic_ignore_index)

    def _seg_loss(self, logit_pred, segment):
        return self.ce_criteria(logit_pred, segment)
