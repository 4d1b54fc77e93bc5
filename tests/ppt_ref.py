"""Restatement of the two pieces Point Prompt Training adds, in plain torch and in the dtype of their arguments (the tests
call them in float64 as the yardstick and in float32 as the torch baseline of the tolerance rule).

head:    the language-guided head of PPT-v1m1: project into the text space, normalise each row, take the inner products
         with the valid class embeddings, scale by exp(logit_scale).
pdnorm:  prompt-driven normalisation: the norm of the active condition - a BatchNorm1d (running statistics in eval, batch
         statistics with the biased variance in training) or a LayerNorm - then, if adaptive, feat * (1 + scale) + shift
         with (shift, scale) the two halves of Linear(SiLU(context)).
"""
import torch


def head(feat, weight, bias, class_embedding, valid, logit_scale):
    """feat (N, C), weight (D, C), bias (D) or None, class_embedding (names, D), valid: indices of the K valid names,
    logit_scale: the logarithm of the scale -> (N, K)"""
    h = feat @ weight.t()
    if bias is not None:
        h = h + bias
    h = h / torch.sqrt((h * h).sum(-1, keepdim=True))
    e = class_embedding[torch.as_tensor(list(valid), device=class_embedding.device)]
    return torch.exp(torch.as_tensor(logit_scale, dtype=feat.dtype, device=feat.device)) * (h @ e.t())


def pdnorm(x, kind, params, index, training=False, eps=None, context=None, modulation=None):
    """x (N, C); kind "bn" | "ln"; params: per condition a dict with weight, bias (and running_mean, running_var for
    "bn"); index: the active condition.  modulation: (weight (2C, ctx), bias (2C)) of the adaptive form with context
    (1, ctx).  Returns the output; running statistics are not updated here."""
    p = params[index]
    if kind == "bn":
        eps = 1e-3 if eps is None else eps
        if training:
            mean, var = x.mean(0), x.var(0, unbiased=False)
        else:
            mean, var = p["running_mean"], p["running_var"]
        y = (x - mean) / torch.sqrt(var + eps)
    else:
        eps = 1e-5 if eps is None else eps
        mean, var = x.mean(1, keepdim=True), x.var(1, unbiased=False, keepdim=True)
        y = (x - mean) / torch.sqrt(var + eps)
    if p.get("weight") is not None:
        y = y * p["weight"] + p["bias"]
    if modulation is not None:
        w, b = modulation
        c = context * torch.sigmoid(context)
        shift, scale = (c @ w.t() + b).chunk(2, dim=1)
        y = y * (1.0 + scale) + shift
    return y
