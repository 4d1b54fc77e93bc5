"""Context-aware classifier ("CAC-v1m1", reference
pointcept/models/context_aware_classifier/context_aware_classifier_v1m1_base.py).

Constructor keywords, state_dict and the three result dicts are the reference's.  The reference's head is three Python
loops of full-size tensor operations: per scene (post_refine_proto_batch, :124-149), per class present with a unique()
read (get_adaptive_perspective, :78-90) and per class again (get_distill_loss, :180-193).  Here each is one pass
(csrc/cac.hip):
  - the confidence-masked softmax prototypes of every scene: ptv3_cac_proto_fwd, `proj` then runs once on B * K rows;
  - the label prototypes of the whole batch: the same kernel in its label form; a class is present when its count is
    positive, so nothing is read back; an absent class keeps the detached seg_head.weight row (:227);
  - the distillation loss and its gradient: ptv3_cac_distill_fwd / _bwd;
  - in eval the cosine logits of every scene: ptv3_cac_cos_logits_fwd; training composes get_pred in torch (that
    kernel has no backward).
The composed path - set_fused(False), a hook on a module of the head, detach_pre_logits=False, a CPU tensor, or (K, C)
outside ops.cac_capable - is the same arithmetic in torch without a loop over classes and without unique().

BatchNorm of feat_proj_layer, as the reference runs it: in training it takes the batch statistics of each scene's rows
inside the refine loop and once more over all rows in the adaptive branch (B + 1 momentum updates per step, scenes first).
Both paths keep that order, so they end a step with the same buffers; the per-scene slices are cut at the offsets, which
a training step reads once.  In eval nothing is read: the norm is its running statistics and the layer runs on all rows.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from pointcept.models.losses import build_criteria
from pointcept.models.utils.structure import Point
from pointcept.models.utils.hip_layers import Linear, BatchNorm1d, ReLU
from pointcept.models.builder import MODELS, build_model
from ptv3_hip import ops
from ptv3_hip import autograd as A


def wired(kernel, k, c, training):
    """Which kernels the model calls: by the wiring rule only those measured ahead of the composition on an MI355X
    (12 x 100 000 points, C = 48 / 96, K = 20 / 100 / 200; DESIGN.md section 23, profiles/cac/).  The kernels' inner
    products run on the vector unit and grow with K * C, the compositions' matrix products barely do, so each kernel is
    ahead up to a measured (K, C) and behind past it.  Between the measured shapes the rule extrapolates downwards only:
    a (K, C) is wired when a measured shape with at least its K and at least its C is ahead; nothing wider than the
    widest measured C = 96 is (the distillation pass does not see C)."""
    if kernel == "distill":               # 12 - 26 times ahead at K = 20 / 100 / 200
        return True
    if c > 96:
        return False
    narrow = c <= 48
    if kernel == "proto_softmax":         # forward + backward: ahead up to K = 100; forward alone also at (200, 48)
        return k <= 100 or (not training and narrow and k <= 200)
    if kernel == "proto_label":           # ahead at K = 20, and at (100, 48)
        return k <= 20 or (narrow and k <= 100)
    if kernel == "cos_logits":            # eval only; ahead at K = 20, and at C = 48 up to K = 200
        return not training and (k <= 20 or (narrow and k <= 200))
    raise KeyError(kernel)


def get_pred(x, proto):
    """:66-71; proto (K, C) or (B, K, C) with x (B, n, C)"""
    return F.normalize(x, 2, -1) @ F.normalize(proto, 2, -1).transpose(-1, -2)


def softmax_proto_torch(x, logits, conf_thresh):
    """:134-142 for one scene: (K, C)"""
    p = F.softmax(logits, 1).t()
    if conf_thresh > 0:
        p = p * (p.max(0)[0] >= conf_thresh).to(p.dtype).unsqueeze(0)
    return (p / (p.sum(-1, keepdim=True) + 1e-7)) @ x


def label_proto_torch(x, target, num_classes):
    """:78-90 without the loop: (proto (K, C), count (K)); rows of absent classes are zero"""
    onehot = F.one_hot(target.clamp(min=0), num_classes).to(x.dtype) * (target >= 0).to(x.dtype).unsqueeze(1)
    count = onehot.sum(0)
    return (onehot.t() @ x) / (count + 1e-4).unsqueeze(1), count


def distill_loss_torch(pred, soft, target):
    """get_distill_loss (:153-199) at smoothness 0.5, eps 0, without unique() and the loop over classes"""
    k = soft.shape[1]
    sm = F.softmax(soft.detach(), 1)
    valid = (target != -1).to(pred.dtype)
    onehot = F.one_hot(torch.where(target != -1, target, torch.zeros_like(target)), k).to(pred.dtype)
    loss = -(F.log_softmax(pred, 1) * (0.5 * sm + 0.5 * onehot)).sum(1)
    entropy = -(sm * torch.log(sm + 1e-4)).sum(1) * valid
    member = onehot * valid.unsqueeze(1)
    num, den, count = member.t() @ (loss * entropy), member.t() @ entropy, member.sum(0)
    present = count > 0
    ratio = torch.where(present, num / (den + 1e-4), torch.zeros_like(num))
    return ratio.sum() / (present.to(pred.dtype).sum() + 1e-4)


@MODELS.register_module("CAC-v1m1")
class CACSegmentor(nn.Module):
    def __init__(self, num_classes, backbone_out_channels, backbone=None, criteria=None, cos_temp=15, main_weight=1,
                 pre_weight=1, pre_self_weight=1, kl_weight=1, conf_thresh=0, detach_pre_logits=False):
        super().__init__()
        self.num_classes = num_classes
        self.cos_temp = cos_temp
        self.main_weight = main_weight
        self.pre_weight = pre_weight
        self.pre_self_weight = pre_self_weight
        self.kl_weight = kl_weight
        self.conf_thresh = conf_thresh
        self.detach_pre_logits = detach_pre_logits
        c = backbone_out_channels
        self.backbone = build_model(backbone)
        self.seg_head = Linear(c, num_classes)
        # proj / apd_proj see B * K (or K) rows: plain torch, as the library's other small heads
        self.proj = nn.Sequential(nn.Linear(c * 2, c * 2, bias=False), nn.ReLU(inplace=True), nn.Linear(c * 2, c))
        self.apd_proj = nn.Sequential(nn.Linear(c * 2, c * 2, bias=False), nn.ReLU(inplace=True), nn.Linear(c * 2, c))
        self.feat_proj_layer = nn.Sequential(Linear(c, c, bias=False), BatchNorm1d(c), ReLU(inplace=True), Linear(c, c))
        self.criteria = build_criteria(criteria)
        self._fused = True

    def set_fused(self, on=True):
        """False: the head as a torch composition (the arithmetic of the reference's loops, vectorised)."""
        self._fused = bool(on)
        return self

    def _hooked(self):
        return any(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks
                   for head in (self.seg_head, self.proj, self.apd_proj, self.feat_proj_layer) for m in head.modules())

    def _use_kernels(self, feat):
        return (self._fused and feat.is_cuda and self.detach_pre_logits and not self._hooked()
                and ops.cac_capable(self.num_classes, feat.shape[1]))

    def _feat_proj(self, x):
        f = self.feat_proj_layer
        return f[3](f[2](f[1](f[0](x))))

    # -- post_refine_proto_batch (:98-150) times cos_temp -----------------------------------------------------------
    def _refine(self, feat, seg_logits, offset, fused):
        pred = seg_logits.detach() if self.detach_pre_logits else seg_logits
        weight = self.seg_head.weight
        k, c = weight.shape
        b = offset.shape[0]
        scenes = None

        def cuts():
            nonlocal scenes
            if scenes is None:      # the one read of a step: training cuts the rows at the offsets, so does composing
                ends = [int(v) for v in offset.tolist()]
                scenes = list(zip([0] + ends[:-1], ends))
            return scenes

        if fused and wired("proto_softmax", k, c, self.training):
            proto, _ = A.cac_proto_softmax(feat, pred, offset, float(self.conf_thresh))
        else:
            proto = torch.stack([softmax_proto_torch(feat[s:e], pred[s:e], self.conf_thresh) for s, e in cuts()])
        proto = self.proj(torch.cat([proto, weight.unsqueeze(0).expand(b, k, c)], -1).view(b * k, 2 * c)).view(b, k, c)
        if self.training:           # batch statistics of each scene's rows
            out = [get_pred(self._feat_proj(feat[s:e]), proto[i]) for i, (s, e) in enumerate(cuts())]
            return torch.cat(out, 0) * self.cos_temp
        y = self._feat_proj(feat)
        if fused and wired("cos_logits", k, c, False):
            return ops.cac_cos_logits(y.contiguous(), proto.contiguous(), offset, float(self.cos_temp))
        return torch.cat([get_pred(y[s:e], proto[i]) for i, (s, e) in enumerate(cuts())]) * self.cos_temp

    # -- get_adaptive_perspective (:73-96) times cos_temp -----------------------------------------------------------
    def _adaptive(self, feat, target, fused):
        weight = self.seg_head.weight
        if fused and wired("proto_label", *weight.shape, True):
            proto, _, count = A.cac_proto_label(feat, target, self.num_classes)
        else:
            proto, count = label_proto_torch(feat, target, self.num_classes)
        new_proto = torch.where((count > 0).unsqueeze(1), proto, weight.detach())
        new_proto = self.apd_proj(torch.cat([new_proto, weight], -1))
        return get_pred(self._feat_proj(feat), new_proto) * self.cos_temp

    def head(self, feat, data_dict):
        """everything behind the backbone: feat (N, C) -> the result dict of forward (:208-275).  Under autocast the head
        runs in fp32, fused or composed: the features are upcast and autocast is off for everything behind them
        (the kernels are fp32; `proj`, `apd_proj` and get_pred's product would otherwise come out in half precision)."""
        with torch.autocast(device_type=feat.device.type, enabled=False):
            return self._head(feat, data_dict)

    def _head(self, feat, data_dict):
        offset = data_dict["offset"]
        feat = feat.float().contiguous()
        fused = self._use_kernels(feat)
        seg_logits = self.seg_head(feat)
        if self.training:
            target = data_dict["segment"].long()
            refine_logits = self._refine(feat, seg_logits, offset, fused)
            cac_pred = self._adaptive(feat, target, fused)
            seg_loss = self.criteria(refine_logits, target) * self.main_weight
            pre_loss = self.criteria(cac_pred, target) * self.pre_weight
            pre_self_loss = self.criteria(seg_logits, target) * self.pre_self_weight
            if fused and wired("distill", self.num_classes, feat.shape[1], True):
                kl_loss = A.cac_distill(refine_logits, cac_pred.detach(), target) * self.kl_weight
            else:
                kl_loss = distill_loss_torch(refine_logits, cac_pred.detach(), target) * self.kl_weight
            loss = seg_loss + pre_loss + pre_self_loss + kl_loss
            return dict(loss=loss, seg_loss=seg_loss, pre_loss=pre_loss, pre_self_loss=pre_self_loss, kl_loss=kl_loss)
        refine_logits = self._refine(feat, seg_logits, offset, fused)
        if "segment" in data_dict.keys():
            return dict(loss=self.criteria(seg_logits, data_dict["segment"]), seg_logits=refine_logits)
        return dict(seg_logits=refine_logits)

    def forward(self, data_dict):
        point = self.backbone(data_dict)
        return self.head(point.feat if isinstance(point, Point) else point, data_dict)
