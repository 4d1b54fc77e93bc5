"""Plain float64 statements of the two bottleneck-CPE kernels (csrc/cpe_plus.hip), shared by the tests:
ptv3_subm_conv_ln and ptv3_rows_linear_ln.  Inputs are taken as given (already rounded to the kernel's dtype) and
widened; nothing is rounded on the way."""
import torch


def _ln_act(y, gamma, beta, eps, relu):
    mean = y.mean(1, keepdim=True)
    var = ((y - mean) ** 2).mean(1, keepdim=True)
    out = (y - mean) / torch.sqrt(var + eps) * gamma.double().cpu() + beta.double().cpu()
    return torch.relu(out) if relu else out


def ref_subm_conv_ln(x, w, nbr, bias, gamma, beta, eps=1e-5, relu=True, rows=None):
    """relu(LayerNorm(sum_t w[:, t, :] x[nbr[i][t]] + bias)) in float64 for the output rows `rows` (default: all).
    x (m, c); w (c, kvol, c) or (c, kvol * c); nbr (m, kvol) with -1 for absent taps."""
    x = x.detach().double().cpu()
    nbr = nbr.detach().cpu().long()
    if rows is not None:
        nbr = nbr[rows]
    c, kvol = x.shape[1], nbr.shape[1]
    w = w.detach().double().cpu().reshape(c, kvol, c)
    y = torch.zeros(nbr.shape[0], c, dtype=torch.float64)
    for t in range(kvol):
        hit = torch.nonzero(nbr[:, t] >= 0)[:, 0]
        if hit.numel():
            y[hit] += x[nbr[hit, t]] @ w[:, t].t()
    if bias is not None:
        y = y + bias.double().cpu()
    return _ln_act(y, gamma, beta, eps, relu)


def ref_rows_linear_ln(x, w, bias, gamma, beta, eps=1e-5, relu=True):
    """relu(LayerNorm(x @ w^T + bias)) in float64: x (m, c), w (cout, c)."""
    y = x.detach().double().cpu() @ w.detach().double().cpu().t()
    if bias is not None:
        y = y + bias.double().cpu()
    return _ln_act(y, gamma, beta, eps, relu)
