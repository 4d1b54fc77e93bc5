"""Build-container-only: run the reference's own FocalLoss (pointcept/models/losses/misc.py:96-172) and LovaszLoss
(losses/lovasz.py, mode="multiclass"), imported in place through ref_loader, on FLOAT64 logits and store, in
seg_losses_ref.npz, per case: logits (fp32 values), labels, both losses (float64) and both gradients (computed in float64, stored as fp32).  Float64 gives the
reference's algorithm without the fp32 cancellation of `jaccard[1:] - jaccard[:-1]`.  Its code is dtype-generic but for
the two `.float()` casts of _lovasz_grad (lovasz.py:28-29), which make torch.dot fail on mixed dtypes; while the
reference's LovaszLoss runs, torch.Tensor.float is therefore replaced by torch.Tensor.double (nothing else is touched).

Cases (N, C): (1, 2), (2, 2), (65, 2), (65, 13) with 3 classes present, (300, 13) with a third of the labels -1 (5 classes
present), (64, 2) with every label -1.  FocalLoss: gamma 2.0, alpha [0.1, 0.9] at C = 2 and the scalar 0.25 at C = 13;
both losses with loss_weight 1.0 and ignore_index -1.

The Lovasz gradient depends on the sort order, so the inputs are built to make that order unambiguous in fp32 too: the
probabilities of the present classes sit on jittered grids (one grid per class, rows permuted), the rest of each row's mass
goes to the absent classes, logits = log p + a per-row shift.  The script asserts, for every class in the labels, that the
smallest gap between consecutive sorted float64 errors exceeds 1e-4, and takes the first seed for which that holds.
Where no row is valid the reference returns the float 0.0 (focal) / an empty tensor (Lovasz): stored as loss 0, zero
gradient.
usage: python tests/golden/make_golden_seg_losses.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_loader  # noqa: E402

# name, N, C, present classes, share of ignored labels
CASES = [("n1c2", 1, 2, 2, 0.0), ("n2c2", 2, 2, 2, 0.0), ("n65c2", 65, 2, 2, 0.0), ("n65c13", 65, 13, 3, 0.0),
         ("n300c13", 300, 13, 5, 1.0 / 3.0), ("n64c2_ignored", 64, 2, 2, 1.0)]
MIN_GAP = 1e-4


def make_case(n, c, k, ignored, seed):
    g = torch.Generator().manual_seed(seed)
    present = torch.randperm(c, generator=g)[:k].sort().values
    p = torch.zeros(n, c, dtype=torch.float64)
    if c == 2:
        grid = (torch.randperm(n, generator=g) + 0.5 + 0.4 * (torch.rand(n, generator=g) - 0.5).double()) / n
        p[:, 1] = 0.02 + 0.96 * grid
        p[:, 0] = 1.0 - p[:, 1]
    else:
        for cls in present.tolist():
            grid = (torch.randperm(n, generator=g) + 0.5 + 0.4 * (torch.rand(n, generator=g) - 0.5).double()) / n
            p[:, cls] = 0.9 / k * grid
        absent = [i for i in range(c) if i not in present.tolist()]
        share = torch.rand(n, len(absent), generator=g).double() + 0.1
        p[:, absent] = share / share.sum(1, keepdim=True) * (1.0 - p.sum(1, keepdim=True))
    logits = (p.log() + torch.randn(n, 1, generator=g).double()).float()
    labels = present[torch.randint(0, k, (n,), generator=g)]
    if n >= k:
        labels[:k] = present            # every present class has a row
    if ignored >= 1.0:
        labels = torch.full((n,), -1, dtype=torch.int64)
    elif ignored > 0:
        labels[torch.randperm(n, generator=g)[:int(round(n * ignored))]] = -1
        for j, cls in enumerate(present.tolist()):
            if not (labels == cls).any():
                labels[j] = cls
    return logits, labels


def min_gap(logits, labels):
    p = logits.double().softmax(1)
    keep = labels != -1
    p, lab = p[keep], labels[keep]
    gap = float("inf")
    for cls in lab.unique().tolist():
        err = ((lab == cls).double() - p[:, cls]).abs().sort().values
        if err.numel() > 1:
            gap = min(gap, (err[1:] - err[:-1]).min().item())
    return gap


def run(module, logits, labels, float_is_double=False):
    x = logits.double().requires_grad_(True)
    keep = torch.Tensor.float
    if float_is_double:
        torch.Tensor.float = torch.Tensor.double
    try:
        out = module(x, labels)
    finally:
        torch.Tensor.float = keep
    if not torch.is_tensor(out) or out.numel() != 1:
        return np.float64(0.0), np.zeros(tuple(logits.shape), dtype=np.float32)
    out = out.reshape(())
    out.backward()
    return np.float64(out.item()), x.grad.numpy().astype(np.float32)


def main():
    assert ref_loader.available()
    L = ref_loader.load().losses
    res = {}
    for name, n, c, k, ignored in CASES:
        seed = 0
        while True:
            logits, labels = make_case(n, c, k, ignored, seed)
            gap = min_gap(logits, labels)
            if gap > MIN_GAP:
                break
            seed += 1
        focal = L.FocalLoss(gamma=2.0, alpha=[0.1, 0.9] if c == 2 else 0.25, loss_weight=1.0, ignore_index=-1)
        lovasz = L.LovaszLoss(mode="multiclass", loss_weight=1.0, ignore_index=-1)
        fl, fg = run(focal, logits, labels)
        ll, lg = run(lovasz, logits, labels, float_is_double=True)
        res.update({f"{name}_logits": logits.numpy(), f"{name}_labels": labels.numpy(), f"{name}_seed": np.array(seed),
                    f"{name}_focal_loss": fl, f"{name}_focal_grad": fg, f"{name}_lovasz_loss": ll,
                    f"{name}_lovasz_grad": lg})
        print(f"{name}: seed {seed}, min gap {gap:.3e}, present {sorted(set(labels.tolist()) - {-1})}, "
              f"focal {fl:.9f}, lovasz {ll:.9f}")
    path = os.path.join(HERE, "seg_losses_ref.npz")
    np.savez_compressed(path, **res)
    print("seg_losses_ref.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
