"""The head of the context-aware classifier restated in torch from explicit tensors, vectorised: no loop over classes and
no unique() (context_aware_classifier_v1m1_base.py: post_refine_proto_batch :98-150, get_adaptive_perspective :73-96,
get_pred :66-71, get_distill_loss :153-199, forward :201-275).  The yardstick of test_hip_cac.py, pinned to the
reference's own outputs by test_cac_cpu.py.  Runs in the dtype and on the device of its inputs - float64 for the
reference, float32 for the error of the plain torch composition.  Gradients come from autograd."""
import torch
import torch.nn.functional as F

PARAMS = ("seg_head.weight", "seg_head.bias", "proj.0.weight", "proj.2.weight", "proj.2.bias", "apd_proj.0.weight",
          "apd_proj.2.weight", "apd_proj.2.bias", "feat_proj_layer.0.weight", "feat_proj_layer.1.weight",
          "feat_proj_layer.1.bias", "feat_proj_layer.3.weight", "feat_proj_layer.3.bias")
BN = "feat_proj_layer.1."


def scenes(offset):
    ends = [int(v) for v in offset.tolist()]
    return list(zip([0] + ends[:-1], ends))


def softmax_weights(logits, conf_thresh=0.0):
    """(N, K): softmax rows; with conf_thresh > 0 a row whose largest value is below it is zero"""
    p = F.softmax(logits, 1)
    if conf_thresh > 0:
        p = p * (p.max(1, keepdim=True)[0] >= conf_thresh).to(p.dtype)
    return p


def proto_softmax(x, logits, offset, conf_thresh=0.0):
    """-> (proto (B, K, C), den (B, K)): proto[b, k] = sum_i p[i, k] x[i] / (sum_i p[i, k] + 1e-7) over scene b"""
    w = softmax_weights(logits, conf_thresh)
    num = torch.stack([w[s:e].t() @ x[s:e] for s, e in scenes(offset)])
    den = torch.stack([w[s:e].sum(0) for s, e in scenes(offset)])
    return num / (den + 1e-7).unsqueeze(-1), den


def proto_label(x, labels, num_classes):
    """-> (proto (K, C), count (K)): proto[k] = sum_{t_i = k} x[i] / (count_k + 1e-4); labels outside [0, K) ignored"""
    ok = (labels >= 0) & (labels < num_classes)
    onehot = F.one_hot(torch.where(ok, labels, torch.zeros_like(labels)), num_classes).to(x.dtype) \
        * ok.to(x.dtype).unsqueeze(1)
    count = onehot.sum(0)
    return (onehot.t() @ x) / (count + 1e-4).unsqueeze(1), count


def cos_logits(y, q, offset=None, temp=1.0):
    """temp * get_pred: q (K, C) shared, or (B, K, C) per scene with offset"""
    yn = y / y.norm(dim=1, keepdim=True).clamp(min=1e-12)
    qn = q / q.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    if q.dim() == 2:
        return (yn @ qn.t()) * temp
    return torch.cat([yn[s:e] @ qn[b].t() for b, (s, e) in enumerate(scenes(offset))]) * temp


def distill_rows(pred, soft, labels):
    """per point (loss, entropy, valid) of get_distill_loss at smoothness 0.5, eps 0"""
    k = soft.shape[1]
    sm = F.softmax(soft, 1)
    valid = (labels >= 0) & (labels < k)
    onehot = F.one_hot(torch.where(valid, labels, torch.zeros_like(labels)), k).to(pred.dtype)
    loss = -(F.log_softmax(pred, 1) * (0.5 * sm + 0.5 * onehot)).sum(1)
    entropy = -(sm * torch.log(sm + 1e-4)).sum(1)
    return loss, entropy, valid, onehot


def distill_loss(pred, soft, labels):
    loss, entropy, valid, onehot = distill_rows(pred, soft.detach(), labels)
    member = onehot * valid.to(pred.dtype).unsqueeze(1)
    entropy = entropy * valid.to(pred.dtype)
    num, den, count = member.t() @ (loss * entropy), member.t() @ entropy, member.sum(0)
    present = count > 0
    ratio = torch.where(present, num / (den + 1e-4), torch.zeros_like(num))
    return ratio.sum() / (present.to(pred.dtype).sum() + 1e-4)


def _mlp(x, sd, name):
    return F.linear(F.relu(F.linear(x, sd[name + ".0.weight"])), sd[name + ".2.weight"], sd[name + ".2.bias"])


def _feat_proj(x, sd, stats, training, momentum=0.1, eps=1e-5):
    """feat_proj_layer; stats = [running_mean, running_var, num_batches_tracked], updated in place when training"""
    h = F.linear(x, sd["feat_proj_layer.0.weight"])
    if training:
        n = h.shape[0]
        mean = h.mean(0)
        var = ((h - mean) ** 2).mean(0)
        stats[0] = (1 - momentum) * stats[0] + momentum * mean.detach()
        stats[1] = (1 - momentum) * stats[1] + momentum * var.detach() * (n / (n - 1))
        stats[2] = stats[2] + 1
    else:
        mean, var = stats[0], stats[1]
    h = (h - mean) / torch.sqrt(var + eps) * sd[BN + "weight"] + sd[BN + "bias"]
    return F.linear(F.relu(h), sd["feat_proj_layer.3.weight"], sd["feat_proj_layer.3.bias"])


def _stats(sd):
    return [sd[BN + "running_mean"], sd[BN + "running_var"], int(sd[BN + "num_batches_tracked"])]


def refine(feat, seg_logits, sd, offset, conf_thresh, temp, stats, training):
    """post_refine_proto_batch times temp with detach_pre_logits=True"""
    w = sd["seg_head.weight"]
    proto, _ = proto_softmax(feat, seg_logits.detach(), offset, conf_thresh)
    b = proto.shape[0]
    q = _mlp(torch.cat([proto, w.unsqueeze(0).expand(b, *w.shape)], -1), sd, "proj")
    if training:
        y = torch.cat([_feat_proj(feat[s:e], sd, stats, True) for s, e in scenes(offset)])
    else:
        y = _feat_proj(feat, sd, stats, False)
    return cos_logits(y, q, offset, temp)


def head_eval(feat, sd, offset, conf_thresh, temp):
    """-> (seg_logits, refined seg_logits) of the eval-mode head"""
    seg_logits = F.linear(feat, sd["seg_head.weight"], sd["seg_head.bias"])
    return seg_logits, refine(feat, seg_logits, sd, offset, conf_thresh, temp, _stats(sd), False)


def cross_entropy(logits, target):
    return F.cross_entropy(logits, target, ignore_index=-1)


def head_train(feat, sd, offset, target, conf_thresh, temp):
    """-> (dict of the five losses with CrossEntropyLoss(ignore_index=-1) as criteria and all weights 1, BatchNorm
    statistics after the step: running_mean, running_var, num_batches_tracked)"""
    stats = _stats(sd)
    w = sd["seg_head.weight"]
    k = w.shape[0]
    seg_logits = F.linear(feat, w, sd["seg_head.bias"])
    refined = refine(feat, seg_logits, sd, offset, conf_thresh, temp, stats, True)
    proto, count = proto_label(feat, target, k)
    new_proto = torch.where((count > 0).unsqueeze(1), proto, w.detach())
    q = _mlp(torch.cat([new_proto, w], -1), sd, "apd_proj")
    cac_pred = cos_logits(_feat_proj(feat, sd, stats, True), q, None, temp)
    out = dict(seg_loss=cross_entropy(refined, target), pre_loss=cross_entropy(cac_pred, target),
               pre_self_loss=cross_entropy(seg_logits, target), kl_loss=distill_loss(refined, cac_pred.detach(), target))
    out["loss"] = out["seg_loss"] + out["pre_loss"] + out["pre_self_loss"] + out["kl_loss"]
    return out, stats


def train_step(feat, sd, offset, target, conf_thresh, temp):
    """One step through autograd: the five losses, `dfeat`, the gradient of every head parameter as 'd' + key, and
    `stats` after the step."""
    feat = feat.detach().clone().requires_grad_(True)
    sd = {k: (v.detach().clone().requires_grad_(True) if k in PARAMS else v) for k, v in sd.items()}
    losses, stats = head_train(feat, sd, offset, target, conf_thresh, temp)
    losses["loss"].backward()
    out = {k: v.detach() for k, v in losses.items()}
    out["dfeat"] = feat.grad
    out.update({"d" + k: sd[k].grad for k in PARAMS})
    out["stats"] = stats
    return out
