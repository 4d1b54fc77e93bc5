"""The modulation of SpUNet-v1m3's PDBatchNorms stated in torch, in the dtype and on the device of its inputs (the tests
call it in float64 as the yardstick and in float32 on the device as the statement order to be compared with).

A layer is a dict: W (2C, Cc), b (2C), gamma (C) | None, beta (C) | None, mean (C) | None, var (C) | None.  Rows [0, C) of
W give shift, rows [C, 2C) give scale: the order of `.chunk(2, dim=1)` in the reference's PDBatchNorm.forward."""
import torch
import torch.nn.functional as F


def silu_grad(x):
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def forward(context, layers, fold=False, eps=1e-3):
    """context (1, Cc) -> per layer (out0, out1, one_plus): gamma_eff, beta_eff, or the folded (s, t) with fold=True"""
    out = []
    a = F.silu(context)
    for ly in layers:
        shift, scale = F.linear(a, ly["W"], ly["b"]).chunk(2, dim=1)
        one_plus = (1.0 + scale).reshape(-1)
        shift = shift.reshape(-1)
        g = one_plus if ly["gamma"] is None else ly["gamma"] * one_plus
        be = shift if ly["beta"] is None else ly["beta"] * one_plus + shift
        if fold:
            g = g * torch.rsqrt(ly["var"] + eps)
            be = be - ly["mean"] * g
        out.append((g, be, one_plus))
    return out


def backward(context, layers, d0, d1):
    """from d gamma_eff (d0) and d beta_eff (d1) per layer -> (dW, db, dgamma, dbeta) per layer and dcontext (1, Cc);
    dgamma / dbeta are None for a layer without affine parameters"""
    a = F.silu(context).reshape(-1)
    acc = torch.zeros_like(a)
    outs = []
    for ly, g0, g1, (_, _, one_plus) in zip(layers, d0, d1, forward(context, layers)):
        dshift = g1
        dscale = g0 * (1.0 if ly["gamma"] is None else ly["gamma"]) + (0.0 if ly["beta"] is None else g1 * ly["beta"])
        d = torch.cat([dshift, dscale])
        acc = acc + ly["W"].t() @ d
        outs.append((torch.outer(d, a), d, None if ly["gamma"] is None else g0 * one_plus,
                     None if ly["beta"] is None else g1 * one_plus))
    return outs, (silu_grad(context.reshape(-1)) * acc).reshape(context.shape)


def make_layers(widths, cc, affine, seed, dtype=torch.float64, device="cpu", magnitude=0.1, min_var=1e-6):
    """seeded layers and a context of the given magnitude; running_var spans [min_var, 1.5]"""
    g = torch.Generator().manual_seed(seed)
    layers = []
    for c in widths:
        ly = dict(W=torch.randn(2 * c, cc, generator=g, dtype=torch.float64) / max(cc, 1) ** 0.5,
                  b=0.1 * torch.randn(2 * c, generator=g, dtype=torch.float64),
                  gamma=1 + 0.1 * torch.randn(c, generator=g, dtype=torch.float64) if affine else None,
                  beta=0.1 * torch.randn(c, generator=g, dtype=torch.float64) if affine else None,
                  mean=0.1 * torch.randn(c, generator=g, dtype=torch.float64),
                  var=min_var + 1.5 * torch.rand(c, generator=g, dtype=torch.float64) ** 4)
        ly["var"][0] = min_var
        layers.append({k: None if v is None else v.float().to(dtype).to(device).contiguous() for k, v in ly.items()})
    context = (magnitude * torch.randn(1, cc, generator=g, dtype=torch.float64)).float().to(dtype).to(device)
    return layers, context
