"""Float64 references for the segmentation-loss tests (test_seg_losses_cpu.py, test_hip_seg_losses.py): restatements of the
formulas of losses/lovasz.py:22-33, :118-164 and losses/misc.py:151-172 of the reference, written with the cumulative-sum
form of the Lovasz weights (jaccard[i] - jaccard[i-1]) that the kernels and the torch composition replace by a closed
form."""
import torch


def valid_rows(labels, c, ignore_index):
    v = (labels >= 0) & (labels < c)
    return v if ignore_index is None else v & (labels != ignore_index)


def errors64(logits, labels, ignore_index):
    """(err (N, C) float64, fg (N, C) bool, valid (N) bool, p (N, C) float64) of the fp32-valued logits."""
    n, c = logits.shape
    p = logits.double().softmax(1)
    valid = valid_rows(labels, c, ignore_index)
    fg = (labels.unsqueeze(1) == torch.arange(c)) & valid.unsqueeze(1)
    return (fg.double() - p).abs(), fg, valid, p


def cumsum_weights(fg_sorted, dtype=torch.float64):
    """_lovasz_grad (lovasz.py:22-33) down each column of fg_sorted (M, C), in `dtype`."""
    f = fg_sorted.to(dtype)
    gts = f.sum(0, keepdim=True)
    inter = gts - f.cumsum(0)
    union = gts + (1 - f).cumsum(0)
    jac = 1.0 - inter / union
    out = jac.clone()
    out[1:] = jac[1:] - jac[:-1]
    return out


def jaccard_step_weights(fg_sorted):
    """The same jaccard[i] - jaccard[i-1] down each column of fg_sorted (M, C) as ONE float64 division per weight:
    I_{i-1}/U_{i-1} - I_i/U_i = (I_{i-1} U_i - I_i U_{i-1}) / (U_{i-1} U_i) with the numerator in exact int64 (and
    1 - I_1/U_1 = (U_1 - I_1) / U_1 at i = 1).  cumsum_weights in float64 subtracts two numbers near 1 whose difference
    is about 1/M^2: 1e-16 / 1e-11 = 1e-5 relative at M = 260k, too coarse a yardstick for a 1e-6 check."""
    m = fg_sorted.shape[0]
    f = fg_sorted.long()
    F = f.cumsum(0)
    G = F[-1:]
    i = torch.arange(1, m + 1).unsqueeze(1)
    inter, union = G - F, G + i - F
    out = torch.empty(fg_sorted.shape, dtype=torch.float64)
    out[:1] = (union[:1] - inter[:1]).double() / union[:1].double()
    num = inter[:-1] * union[1:] - inter[1:] * union[:-1]
    out[1:] = num.double() / (union[:-1].double() * union[1:].double())
    return out


def weights_along(order, fg, valid):
    """Float64 Lovasz weights in POINT order (N, C) for a given per-class order (C, N) that lists the valid rows first;
    0 on rows that are not valid."""
    n, c = fg.shape
    nv = int(valid.sum())
    w = torch.zeros(n, c, dtype=torch.float64)
    if nv == 0:
        return w
    head = order[:, :nv].t()                                  # (nv, C) point ids
    g = jaccard_step_weights(fg.gather(0, head))
    w.scatter_(0, head, g)
    return w


def lovasz_from_weights(err, w, fg, loss_weight=1.0):
    per_class = (err * w).sum(0)
    present = fg.any(0)
    k = int(present.sum())
    return float(per_class[present].sum() / k * loss_weight) if k else 0.0


def lovasz_grad_from_weights(p, w, fg, valid, loss_weight=1.0):
    """d loss / d logits (float64) with the weights held constant: the softmax backward of dP = +-w / n_present."""
    present = fg.any(0)
    k = int(present.sum())
    if k == 0:
        return torch.zeros_like(p)
    dp = w * torch.where(fg, -1.0, 1.0) * present * (loss_weight / k)
    g = p * (dp - (p * dp).sum(1, keepdim=True))
    return g * valid.unsqueeze(1)


def focal64(logits, labels, alpha, gamma, ignore_index, loss_weight=1.0, reduction="mean"):
    """(loss, grad) of the focal formula by float64 autograd; alpha a float or a list of C values."""
    n, c = logits.shape
    x = logits.double().requires_grad_(True)
    valid = valid_rows(labels, c, ignore_index)
    t = ((labels.unsqueeze(1) == torch.arange(c)) & valid.unsqueeze(1)).double()
    a = torch.tensor(alpha, dtype=torch.float64) if isinstance(alpha, list) else alpha
    q = torch.sigmoid(torch.where(t > 0, -x, x))      # (1 - s) t + s (1 - t) without 1 - s, which is 0 past x = 37
    aw = a * t + (1 - a) * (1 - t)
    bce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    loss = (aw * q.pow(gamma) * bce * valid.unsqueeze(1)).sum()
    if reduction == "mean":
        loss = loss / max(int(valid.sum()) * c, 1)
    loss = loss * loss_weight
    loss.backward()
    return float(loss.detach()), x.grad
