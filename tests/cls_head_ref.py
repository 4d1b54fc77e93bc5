"""The classifier / regressor head, its L1 loss and column errors restated in torch from explicit tensors (the yardstick
of test_hip_cls_head.py and test_body_regressor_cpu.py; pinned to the reference's own outputs by the latter):
pointcept/models/default.py:303-313 (cls_head), losses/weight_regression_loss.py:30-38, pig_regressor.py:36-55.
Runs in the dtype and on the device of its inputs - float64 for the reference, float32 on the GPU for the error of the
plain torch composition.  Gradients come from autograd."""
import torch
import torch.nn.functional as F

PARAMS = ("0.weight", "0.bias", "1.weight", "1.bias", "4.weight", "4.bias", "5.weight", "5.bias", "8.weight", "8.bias")


def head_eval(g, sd, eps=1e-5):
    """logits of the eval-mode head; sd: the Sequential's state_dict ('0.weight' ... '8.bias', BatchNorm buffers)."""
    h = F.linear(g, sd["0.weight"], sd["0.bias"])
    h = F.relu((h - sd["1.running_mean"]) / torch.sqrt(sd["1.running_var"] + eps) * sd["1.weight"] + sd["1.bias"])
    h = F.linear(h, sd["4.weight"], sd["4.bias"])
    h = F.relu((h - sd["5.running_mean"]) / torch.sqrt(sd["5.running_var"] + eps) * sd["5.weight"] + sd["5.bias"])
    return F.linear(h, sd["8.weight"], sd["8.bias"])


def _bn_train(z, weight, bias, eps):
    mean = z.mean(0)
    var = ((z - mean) ** 2).mean(0)
    return (z - mean) / torch.sqrt(var + eps) * weight + bias, mean, var * (z.shape[0] / (z.shape[0] - 1))


def head_train(g, sd, mask1, mask2, keep, momentum=0.1, eps=1e-5):
    """(logits, running statistics after the step) of the training-mode head with the given 0 / 1 keep-masks."""
    y, m1, v1 = _bn_train(F.linear(g, sd["0.weight"], sd["0.bias"]), sd["1.weight"], sd["1.bias"], eps)
    h = F.relu(y) * mask1 / keep
    y, m2, v2 = _bn_train(F.linear(h, sd["4.weight"], sd["4.bias"]), sd["5.weight"], sd["5.bias"], eps)
    h = F.relu(y) * mask2 / keep
    run = {"1.running_mean": (1 - momentum) * sd["1.running_mean"] + momentum * m1.detach(),
           "1.running_var": (1 - momentum) * sd["1.running_var"] + momentum * v1.detach(),
           "5.running_mean": (1 - momentum) * sd["5.running_mean"] + momentum * m2.detach(),
           "5.running_var": (1 - momentum) * sd["5.running_var"] + momentum * v2.detach()}
    return F.linear(h, sd["8.weight"], sd["8.bias"]), run


def l1_stats(logits, target, loss_weight=1.0, metric_scale=100.0):
    """[loss_weight * mean |logits - target|, metric_scale * column means of |logits - target|] as one (1 + out) vector
    (RegressionL1Loss; the e_* of PigBodyRegressor are the mean |100 pred - 100 target| per column)."""
    d = (logits - target.reshape(logits.shape)).abs()
    return torch.cat([(loss_weight * d.mean()).reshape(1), metric_scale * d.mean(0)])


def train_step(g, sd, mask1, mask2, keep, target=None, loss_weight=1.0, metric_scale=100.0, dlogits=None, dloss=1.0,
               momentum=0.1, eps=1e-5):
    """One step through autograd: dict with logits, stats (L1 mode), run (running statistics), dg, and the gradient of
    every parameter.  L1 mode (target given): the loss's gradient scaled by dloss; otherwise dlogits is fed in."""
    g = g.detach().clone().requires_grad_(True)
    sd = {k: (v.detach().clone().requires_grad_(True) if k in PARAMS else v) for k, v in sd.items()}
    logits, run = head_train(g, sd, mask1, mask2, keep, momentum, eps)
    out = {"logits": logits.detach(), "run": run}
    if target is not None:
        stats = l1_stats(logits, target, loss_weight, metric_scale)
        out["stats"] = stats.detach()
        (stats[0] * dloss).backward()
    else:
        (logits * dlogits).sum().backward()
    out["dg"] = g.grad
    out.update({"d" + k: sd[k].grad for k in PARAMS})
    return out
