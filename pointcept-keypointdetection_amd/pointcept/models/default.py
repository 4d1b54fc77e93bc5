"""Segmentation wrapper around the MI355X PTv3 backbones: registry name "DefaultSegmentorV2".

Contract of the reference class (pointcept/models/default.py:41-95), which the semseg configs build
(`configs/scannet/semseg-pt-v3m1-0-base.py`, `configs/pigseg/semseg-ptv3-v1m1-0-base.py`): constructor keywords
`num_classes, backbone_out_channels, backbone, criteria, freeze_backbone`; state_dict = `seg_head.{weight,bias}` +
`backbone.*`; `forward(input_dict, return_point=False)` returns `loss` in training, `loss` + `seg_logits` when the
batch carries "segment" in eval, `seg_logits` alone otherwise (+ `point` on request).  The head is one ptv3_gemm.

"DefaultClassifier" (pointcept/models/default.py:289-338; configs/modelnet40/cls-*.py, and the base class of the fork's
PigBodyRegressor): per-scene mean of the backbone's features, then `cls_head`.  Its head is written for the batch of
pooled rows (csrc/cls_head.hip): eval = the pooling partials plus one workgroup for the whole
head, training = one forward and two backward launches; `set_fused(False)` (or a hook on the head, a frozen head
parameter, SyncBatchNorm, widths outside the kernels' limits) composes it from the per-layer modules instead.
"""
import torch
import torch.nn as nn

from pointcept.models.losses import build_criteria
from pointcept.models.utils.structure import Point
from pointcept.models.utils.hip_layers import Linear, BatchNorm1d, ReLU, check_sync_batchnorm
from ptv3_hip import ops
from ptv3_hip import autograd as A
from .builder import MODELS, build_model
from .keypoint_ptv3 import check_scene_count, _wt


def _full_resolution(point):
    """Point-order features at the input resolution.  A decoder-less backbone (enc_mode) hands back its deepest
    level: every level's features are broadcast to its parent through `pooling_inverse` and appended to the
    parent's channels until the unpooled root is reached (default.py:70-75)."""
    if not isinstance(point, Point):
        return point, point                      # legacy backbones return the feature matrix itself
    levels = [point]
    while "pooling_parent" in levels[-1].keys():
        child = levels[-1]
        if "pooling_inverse" not in child.keys():
            raise AssertionError("pooling_parent without pooling_inverse")
        levels.append(child["pooling_parent"])
    for child, parent in zip(levels[:-1], levels[1:]):
        inverse = child.pop("pooling_inverse")
        child.pop("pooling_parent")
        parent.feat = torch.cat((parent.feat, child.feat.index_select(0, inverse)), dim=1)
    root = levels[-1]
    return root, root.feat


@MODELS.register_module()
class DefaultSegmentor(nn.Module):
    """default.py:14-37: a backbone that returns per-point logits itself (Swin3D-v1m1 is built this way,
    configs/s3dis/semseg-swin3d-v1m1-0-small.py:9-31)."""

    def __init__(self, backbone=None, criteria=None):
        super().__init__()
        self.backbone = build_model(backbone)
        self.criteria = build_criteria(criteria)

    def forward(self, input_dict):
        if "condition" in input_dict.keys():
            input_dict["condition"] = input_dict["condition"][0]
        seg_logits = self.backbone(input_dict)
        if self.training:
            return dict(loss=self.criteria(seg_logits, input_dict["segment"]))
        if "segment" in input_dict.keys():
            return dict(loss=self.criteria(seg_logits, input_dict["segment"]), seg_logits=seg_logits)
        return dict(seg_logits=seg_logits)


@MODELS.register_module()
class DefaultSegmentorV2(nn.Module):
    def __init__(self, num_classes, backbone_out_channels, backbone=None, criteria=None, freeze_backbone=False):
        super().__init__()
        self.seg_head = Linear(backbone_out_channels, num_classes) if num_classes > 0 else nn.Identity()
        self.backbone = build_model(backbone)
        self.criteria = build_criteria(criteria)
        self.freeze_backbone = bool(freeze_backbone)
        if self.freeze_backbone:
            self.backbone.requires_grad_(False)

    def forward(self, input_dict, return_point=False):
        # the collated dict goes to the backbone as it is (the backbone wraps it in its own Point, as the reference's
        # does with the Point it is handed): the native executor then derives `batch` from `offset` on its geometry
        # stream instead of receiving one produced on the caller's stream a moment ago
        point, feat = _full_resolution(self.backbone(input_dict))
        seg_logits = self.seg_head(feat.contiguous()).float()
        result = {"point": point} if return_point else {}
        labelled = "segment" in input_dict.keys()
        if self.training or labelled:
            result["loss"] = self.criteria(seg_logits, input_dict["segment"])
        if not self.training:
            result["seg_logits"] = seg_logits
        return result


@MODELS.register_module()
class DefaultClassifier(nn.Module):
    # what the in-kernel column errors are multiplied by (PigBodyRegressor: 100, pig_regressor.py:42-43)
    metric_scale = 1.0
    # the one-workgroup eval head sums the scenes' slabs one after the other: measured faster than the composition at
    # 1, 4 and 8 scenes and slower at 32, so larger batches compose
    fused_eval_max_scenes = 8

    def __init__(self, backbone=None, criteria=None, num_classes=40, backbone_embed_dim=256):
        super().__init__()
        self.backbone = build_model(backbone)
        self.criteria = build_criteria(criteria)
        self.num_classes = num_classes
        self.backbone_embed_dim = backbone_embed_dim
        self.cls_head = nn.Sequential(
            Linear(backbone_embed_dim, 256),
            BatchNorm1d(256),
            ReLU(inplace=True),
            nn.Dropout(p=0.5),
            Linear(256, 128),
            BatchNorm1d(128),
            ReLU(inplace=True),
            nn.Dropout(p=0.5),
            Linear(128, num_classes),
        )
        self.fused = True

    def set_fused(self, on=True):
        """False: the head as a plain `self.cls_head(g)` call followed by `self.criteria` (the composition of per-layer
        entry points - the fallback, and the baseline the fused head is measured against)."""
        self.fused = bool(on)
        return self

    # ---- which path ------------------------------------------------------------------------------------------
    def _l1(self):
        """The single RegressionL1Loss whose value the head kernels compute themselves, or None."""
        from pointcept.models.losses import RegressionL1Loss
        crit = self.criteria.criteria
        return crit[0] if len(crit) == 1 and type(crit[0]) is RegressionL1Loss else None

    def _head_plain(self):
        """The head is the nine modules the kernels restate, with no hook (forward or backward) that has to see an
        intermediate tensor."""
        head = self.cls_head
        if len(head) != 9 or any(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or m._backward_pre_hooks
                                 for m in head.modules()):
            return False
        if not all(isinstance(head[i], t) for i, t in ((0, Linear), (1, BatchNorm1d), (2, nn.ReLU), (3, nn.Dropout),
                                                       (4, Linear), (5, BatchNorm1d), (6, nn.ReLU), (7, nn.Dropout),
                                                       (8, Linear))):
            return False
        if any(head[i].bias is None for i in (0, 4, 8)) or any(not head[i].affine for i in (1, 5)):
            return False
        return ops.cls_head_capable(head[0].in_features, head[0].out_features, head[4].out_features,
                                    head[8].out_features)

    def _fused_eval(self):
        head = self.cls_head
        return self.fused and self._head_plain() and not any(m.training for m in head) and \
            all(head[i].running_mean is not None for i in (1, 5))

    def _fused_train(self):
        head = self.cls_head
        if not (self.fused and torch.is_grad_enabled() and self._head_plain()):
            return False
        if not all(head[i].training for i in (1, 3, 5, 7)) or head[3].p != head[7].p or not head[3].p < 1.0:
            return False
        if any(not isinstance(head[i].momentum, float) or getattr(head[i], "sync_group", None) is not None
               or head[i].running_mean is None for i in (1, 5)):
            return False
        return all(p.requires_grad and p.dtype == torch.float32 for p in head.parameters())

    # ---- the head ----------------------------------------------------------------------------------------------
    def _target(self, input_dict, l1):
        """The flattened fp32 target the kernels take; the literal view(-1, 7) of RegressionL1Loss first, so a numel
        that 7 does not divide raises as the loss itself does."""
        if l1 is None or "category" not in input_dict:
            return None
        target = input_dict["category"]
        target.view(-1, 7)
        return target.float().contiguous()

    def _head(self, feat, offset, input_dict):
        """-> (cls_logits, loss or None, stats or None); stats = [loss, metric_scale * column errors] when a kernel
        computed them (criteria is one RegressionL1Loss)."""
        labelled = "category" in input_dict
        head, l1 = self.cls_head, self._l1()
        pooled = offset is None
        if self.training and self._fused_train():
            g = feat.float() if pooled else A.scene_mean(feat, offset)
            keep = 1.0 - head[3].p
            h1, h2 = head[0].out_features, head[4].out_features
            mask = torch.empty(g.shape[0] * (h1 + h2), dtype=torch.float32, device=g.device).bernoulli_(keep)
            masks = (mask[:g.shape[0] * h1].view(-1, h1), mask[g.shape[0] * h1:].view(-1, h2))
            for i in (1, 5):
                if head[i].num_batches_tracked is not None:
                    head[i].num_batches_tracked.add_(1)
            target = self._target(input_dict, l1)
            if target is not None and target.numel() == g.shape[0] * self.num_classes:
                logits, stats = A.cls_head_train(g, head, masks, keep, target, l1.loss_weight, self.metric_scale)
                return logits, stats[0], stats
            logits, _ = A.cls_head_train(g, head, masks, keep)
            return logits, self.criteria(logits, input_dict["category"]), None
        if not self.training and not pooled and offset.shape[0] <= self.fused_eval_max_scenes and self._fused_eval():
            target = self._target(input_dict, l1)
            if target is not None and target.numel() != offset.shape[0] * self.num_classes:
                target = None
            (s1, t1), (s2, t2) = head[1].folded(), head[5].folded()
            logits, stats = ops.cls_head_eval(feat.contiguous(), offset, _wt(head[0]), head[0].bias_f32(), s1, t1,
                                              _wt(head[4]), head[4].bias_f32(), s2, t2, _wt(head[8]),
                                              head[8].bias_f32(), target, l1.loss_weight if target is not None else 1.0,
                                              self.metric_scale)
            if stats is not None:
                return logits, stats[0], stats
            return logits, (self.criteria(logits, input_dict["category"]) if labelled else None), None
        # composed: one module after the other, then the criteria as they are
        if pooled:
            g = feat.float()
        else:
            g = A.scene_mean(feat, offset) if self.training else ops.scene_mean(feat.contiguous(), offset)
        logits = head(g)
        return logits, (self.criteria(logits, input_dict["category"]) if self.training or labelled else None), None

    def _forward(self, input_dict):
        check_sync_batchnorm(self)
        offset = input_dict["offset"]
        check_scene_count(self, offset, self.cls_head[1])
        if not input_dict["feat"].is_cuda:
            raise RuntimeError("DefaultClassifier: expected GPU tensors (the HIP path has no CPU fallback)")
        # the collated dict goes to the backbone as it is, as in DefaultSegmentorV2
        point = self.backbone(input_dict)
        if isinstance(point, Point):
            logits, loss, stats = self._head(point.feat, point.offset, input_dict)
        else:
            logits, loss, stats = self._head(point, None, input_dict)
        result = {}
        if loss is not None:
            result["loss"] = loss
        if not self.training:
            result["cls_logits"] = logits
        return result, logits, stats

    def forward(self, input_dict):
        return self._forward(input_dict)[0]
