"""csrc/seg_loss.hip on the GPU: ptv3_lovasz_fwd / _bwd and ptv3_focal_fwd / _bwd through the C ABI (ptv3_hip.ops) and
through the LovaszLoss / FocalLoss modules, against float64 torch on the same fp32-valued inputs (seg_loss_ref.py), and
the pigseg criteria under DefaultSegmentorV2.

The Lovasz checks are robust to near-ties: the kernel's own per-class order is checked to be a descending order of the
float64 errors up to 1e-6, and the weights, the loss and the gradient are then compared with float64 values computed
ALONG THAT ORDER.  Bounds: weights 1e-6 relative (an fp32 rounding of a float64 value is 6e-8); loss 2e-6 absolute (a
class's loss is sum err_i g_i with sum g_i <= 1, |d err| a few fp32 ulps); gradient 3e-5 * max|ref| ((C + 5) * 2^-24 at
C = 200, doubled); fixture gradients 1e-5 * max|ref|; focal 1e-5 relative / 1e-5 * max|ref|."""
import os

import numpy as np
import pytest
import torch

import seg_loss_ref as R

pytestmark = pytest.mark.gpu
T = 1024             # SL_TILE of csrc/seg_loss.hip: sorted positions per workgroup of the scan (checked below)
SCAN_PASS = 256      # tiles one pass of lovasz_tile_scan_kernel covers (SL_THREADS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _inputs(n, c, present, ignored=0.0, seed=0, scale=2.0):
    g = torch.Generator().manual_seed(seed * 7919 + n * 31 + c)
    logits = torch.randn(n, c, generator=g) * scale
    classes = torch.randperm(c, generator=g)[:present]
    labels = classes[torch.randint(0, present, (n,), generator=g)]
    if ignored > 0:
        labels[torch.rand(n, generator=g) < ignored] = -1
    return logits, labels


def _saturated(n, c):
    g = torch.Generator().manual_seed(n + c)
    hot = torch.randint(0, c, (n,), generator=g)
    logits = torch.full((n, c), -40.0)
    logits[torch.arange(n), hot] = 40.0
    labels = torch.randint(0, c, (n,), generator=g)
    labels[::9] = -1
    return logits, labels


def _out_of_range(n, c):
    logits, labels = _inputs(n, c, c, 0.1, seed=3)
    labels[5], labels[n // 2], labels[n - 1] = c, -7, 2 ** 40
    return logits, labels


LOVASZ_CASES = {
    "n1_c2": lambda: _inputs(1, 2, 2),
    "n2_c2": lambda: _inputs(2, 2, 2),
    "tile_minus_1_c2": lambda: _inputs(T - 1, 2, 2),
    "tile_c3": lambda: _inputs(T, 3, 3),
    "tile_plus_1_c13_3_present": lambda: _inputs(T + 1, 13, 3),
    "3_tiles_plus_5_c13_third_ignored": lambda: _inputs(3 * T + 5, 13, 13, 1.0 / 3.0),
    "n4097_c200_30_present": lambda: _inputs(4097, 200, 30),
    "two_scan_passes_c2": lambda: _inputs(SCAN_PASS * T + 7, 2, 2, 0.05),
    "all_ignored": lambda: (_inputs(300, 5, 5)[0], torch.full((300,), -1, dtype=torch.int64)),
    "out_of_range_labels": lambda: _out_of_range(T + 9, 7),
    "saturated_ties": lambda: _saturated(2 * T + 3, 3),
}


def test_scan_tile_is_the_stated_one():
    from ptv3_hip import ops
    assert ops.lovasz_scan_tile() == T


@pytest.mark.parametrize("name", list(LOVASZ_CASES))
def test_lovasz_c_abi_vs_float64(dev, name):
    from ptv3_hip import ops
    logits, labels = LOVASZ_CASES[name]()
    n, c = logits.shape
    err, fg, valid, p = R.errors64(logits, labels, -1)
    nv = int(valid.sum())
    x, y = logits.to(dev), labels.to(dev)
    out, weight, order, count = ops.lovasz_softmax(x, y, -1, 1.0)
    dl = torch.ones(1, device=dev)
    grad = ops.lovasz_softmax_bwd(dl, x, y, weight, count, -1, 1.0)
    out2, weight2, order2, count2 = ops.lovasz_softmax(x, y, -1, 1.0)
    grad2 = ops.lovasz_softmax_bwd(dl, x, y, weight2, count2, -1, 1.0)
    torch.cuda.synchronize()
    order_h, weight_h = order.cpu(), weight.cpu().double()
    # (a) every row of `order` is a permutation, descending in the float64 error, valid rows first
    assert torch.equal(order_h.sort(1).values, torch.arange(n).expand(c, n))
    valid_s = valid[order_h]                                        # (C, N)
    assert valid_s[:, :nv].all() and not valid_s[:, nv:].any()
    err_s = err.t().gather(1, order_h)[:, :nv]
    if nv > 1:
        worst = (err_s[:, 1:] - err_s[:, :-1]).max().item()
        print(f"{name}: largest rise along the order {worst:.2e}")
        assert worst <= 1e-6
    # (b) the weights are the float64 weights along the kernel's own order; 0 on rows that are not valid
    w64 = R.weights_along(order_h, fg, valid)
    rel = ((weight_h - w64).abs() / w64.abs().clamp(min=1e-300))[w64 != 0]
    print(f"{name}: weight max relative error {rel.max().item() if rel.numel() else 0.0:.2e}")
    assert (weight_h[w64 == 0] == 0).all() and (weight_h[~valid] == 0).all()
    assert rel.numel() == 0 or rel.max().item() <= 1e-6
    # (c) counts
    assert torch.equal(count.cpu()[:c].long(), fg.sum(0)) and int(count[c]) == int(fg.any(0).sum())
    # (d) loss
    ref_loss = R.lovasz_from_weights(err, w64, fg)
    print(f"{name}: loss {out.item():.9f} ref {ref_loss:.9f}")
    assert abs(out.item() - ref_loss) <= 2e-6
    if nv == 0:
        assert out.item() == 0.0
    # (e) gradient
    ref_grad = R.lovasz_grad_from_weights(p, w64, fg, valid)
    top = ref_grad.abs().max().item()
    diff = (grad.cpu().double() - ref_grad).abs().max().item()
    print(f"{name}: grad diff {diff:.2e}, max|ref| {top:.2e}")
    assert diff <= 3e-5 * top
    assert (grad.cpu()[~valid] == 0).all()
    # (f) bitwise reproducible
    assert torch.equal(out, out2) and torch.equal(weight, weight2) and torch.equal(grad, grad2)
    assert torch.equal(order, order2) and torch.equal(count, count2)


def test_lovasz_saturated_is_the_hard_jaccard_loss(dev):
    """+-40 logits: exact ties everywhere; whatever the order inside a tie, the loss is the Jaccard loss of the hard
    prediction, and permuting the rows changes it by no more than fp32 rounding."""
    from ptv3_hip import ops
    logits, labels = _saturated(2 * T + 3, 3)
    valid = labels != -1
    pred, lab = logits.argmax(1)[valid], labels[valid]
    jac = [1.0 - ((pred == k) & (lab == k)).sum().item() / ((pred == k) | (lab == k)).sum().item()
           for k in lab.unique().tolist()]
    out = ops.lovasz_softmax(logits.to(dev), labels.to(dev), -1, 1.0)[0].item()
    perm = torch.randperm(logits.shape[0], generator=torch.Generator().manual_seed(1))
    out_p = ops.lovasz_softmax(logits[perm].to(dev), labels[perm].to(dev), -1, 1.0)[0].item()
    assert abs(out - sum(jac) / len(jac)) <= 2e-6 and abs(out - out_p) <= 2e-6


def test_lovasz_limits_are_errors(dev):
    from ptv3_hip import ops
    y = torch.zeros(4, dtype=torch.int64, device=dev)
    for c in (1, 1025):
        assert not ops.seg_loss_capable(4, c)
        with pytest.raises(RuntimeError, match="classes"):
            ops.lovasz_softmax(torch.zeros(4, c, device=dev), y, -1, 1.0)
    assert not ops.seg_loss_capable(2 ** 21, 1024)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "seg_losses_ref.npz"))


@pytest.mark.parametrize("name", ["n1c2", "n2c2", "n65c2", "n65c13", "n300c13", "n64c2_ignored"])
def test_modules_match_reference_fixture(dev, golden, name):
    """(g) LovaszLoss / FocalLoss on the GPU against the reference's own modules run on float64 logits."""
    from pointcept.models.losses import LovaszLoss, FocalLoss
    logits, labels = torch.from_numpy(golden[f"{name}_logits"]), torch.from_numpy(golden[f"{name}_labels"])
    c = logits.shape[1]
    for module, key in ((LovaszLoss(mode="multiclass", loss_weight=1.0, ignore_index=-1), "lovasz"),
                        (FocalLoss(gamma=2.0, alpha=[0.1, 0.9] if c == 2 else 0.25, loss_weight=1.0, ignore_index=-1),
                         "focal")):
        x = logits.to(dev).requires_grad_(True)
        loss = module(x, labels.to(dev))
        assert loss.dim() == 0 and loss.dtype == torch.float32 and "Backward" in type(loss.grad_fn).__name__
        assert type(loss.grad_fn).__name__.startswith(("LovaszSoftmaxFn", "FocalLossFn"))   # the HIP path, not torch
        loss.backward()
        ref_loss, ref_grad = float(golden[f"{name}_{key}_loss"]), torch.from_numpy(golden[f"{name}_{key}_grad"])
        top = ref_grad.abs().max().item()
        diff = (x.grad.cpu() - ref_grad).abs().max().item()
        print(f"{name} {key}: loss {loss.item():.9f} ref {ref_loss:.9f}; grad diff {diff:.2e}, max|ref| {top:.2e}")
        assert abs(loss.item() - ref_loss) <= (2e-6 if key == "lovasz" else 1e-5 * abs(ref_loss))
        assert diff <= 1e-5 * top
        # the torch composition (use_hip = False) on the same device tensor agrees as well
        module.use_hip = False
        x2 = logits.to(dev).requires_grad_(True)
        loss2 = module(x2, labels.to(dev))
        loss2.backward()
        assert abs(loss2.item() - ref_loss) <= 2e-6 and (x2.grad.cpu() - ref_grad).abs().max().item() <= 1e-5 * top


def test_modules_cast_other_float_dtypes(dev):
    from pointcept.models.losses import LovaszLoss, FocalLoss
    logits, labels = _inputs(500, 4, 4, 0.1)
    y = labels.to(dev)
    for module in (LovaszLoss(mode="multiclass", ignore_index=-1), FocalLoss(alpha=0.25)):
        base = module(logits.to(dev), y)
        assert torch.equal(module(logits.to(dev).double(), y), base)
        half = module(logits.to(dev).bfloat16(), y)
        assert half.dtype == torch.float32 and torch.equal(half, module(logits.bfloat16().float().to(dev), y))


FOCAL_N = [1, 2, T - 1, T, T + 1, 3 * T + 5, 4097]


@pytest.mark.parametrize("gamma", [2.0, 0.5])
@pytest.mark.parametrize("alpha_kind", ["list", "scalar"])
@pytest.mark.parametrize("c", [2, 13])
def test_focal_c_abi_vs_float64(dev, c, alpha_kind, gamma):
    from ptv3_hip import ops
    g = torch.Generator().manual_seed(c)
    alpha = (torch.rand(c, generator=g) * 0.8 + 0.1).tolist() if alpha_kind == "list" else 0.25
    alpha_dev = torch.tensor(alpha if alpha_kind == "list" else [alpha] * c, dtype=torch.float32, device=dev)
    for n in FOCAL_N:
        for reduction in ("mean", "sum") if n == T + 1 else ("mean",):
            logits, labels = _inputs(n, c, c, 0.2 if n > 2 else 0.0, seed=1, scale=3.0)
            if n > 8:
                labels[3], labels[n - 2] = c + 4, -3                     # out of range: treated as ignored
            valid = R.valid_rows(labels, c, -1)
            ref_loss, ref_grad = R.focal64(logits, labels, alpha, gamma, -1, 1.5, reduction)
            x, y = logits.to(dev), labels.to(dev)
            out, nvalid = ops.focal_loss(x, y, alpha_dev, gamma, -1, 1.5, reduction)
            grad = ops.focal_loss_bwd(torch.ones(1, device=dev), x, y, alpha_dev, nvalid, gamma, -1, 1.5, reduction)
            out2, _ = ops.focal_loss(x, y, alpha_dev, gamma, -1, 1.5, reduction)
            top = ref_grad.abs().max().item()
            diff = (grad.cpu().double() - ref_grad).abs().max().item()
            print(f"focal n={n} c={c} {alpha_kind} gamma={gamma} {reduction}: loss {out.item():.9f} ref {ref_loss:.9f}; "
                  f"grad diff {diff:.2e}, max|ref| {top:.2e}")
            assert int(nvalid) == int(valid.sum())
            assert abs(out.item() - ref_loss) <= 1e-5 * abs(ref_loss)
            assert diff <= 1e-5 * top
            assert (grad.cpu()[~valid] == 0).all()
            assert torch.equal(out, out2)


def test_focal_all_ignored_and_saturated(dev):
    from ptv3_hip import ops
    alpha = torch.tensor([0.1, 0.9], device=dev)
    x = torch.randn(64, 2, generator=torch.Generator().manual_seed(0)).to(dev)
    y = torch.full((64,), -1, dtype=torch.int64, device=dev)
    out, nvalid = ops.focal_loss(x, y, alpha, 2.0, -1, 1.0, "mean")
    grad = ops.focal_loss_bwd(torch.ones(1, device=dev), x, y, alpha, nvalid, 2.0, -1, 1.0, "mean")
    assert out.item() == 0.0 and int(nvalid) == 0 and not grad.any()
    # |x| = 200: sigmoid underflows to exactly 0 / 1 in fp32; gamma < 1 must not produce inf * 0
    logits, labels = _saturated(300, 2)
    logits = logits * 5.0
    for gamma in (0.5, 2.0):
        ref_loss, ref_grad = R.focal64(logits, labels, [0.1, 0.9], gamma, -1, 1.0, "mean")
        out, nvalid = ops.focal_loss(logits.to(dev), labels.to(dev), alpha, gamma, -1, 1.0, "mean")
        grad = ops.focal_loss_bwd(torch.ones(1, device=dev), logits.to(dev), labels.to(dev), alpha, nvalid, gamma, -1,
                                  1.0, "mean")
        assert torch.isfinite(grad).all()
        assert abs(out.item() - ref_loss) <= 1e-5 * abs(ref_loss)
        assert (grad.cpu().double() - ref_grad).abs().max().item() <= 1e-5 * ref_grad.abs().max().item()


def test_pigseg_criteria_under_default_segmentor_v2(dev):
    """A two-stage tiny PT-v3m1 under DefaultSegmentorV2 with PIGSEG_CRITERIA: one training forward + backward, and the
    loss against the two modules applied to the eval seg_logits of the same weights.  The BatchNorm layers are kept in
    eval mode for the training call (frozen statistics), so both calls normalise with the same numbers; drop_path is 0
    and the orders are not shuffled."""
    import torch.nn as nn
    import ptv3_scenes as S
    from pointcept.models import build_model
    from pointcept.models.losses import build_criteria
    from ptv3_hip.configs import ORDERS, PIGSEG_CRITERIA
    backbone = dict(type="PT-v3m1", in_channels=4, order=ORDERS, stride=(2,), enc_depths=(1, 1), enc_channels=(16, 32),
                    enc_num_head=(1, 2), enc_patch_size=(64, 64), dec_depths=(1,), dec_channels=(16,), dec_num_head=(1,),
                    dec_patch_size=(64,), mlp_ratio=4, qkv_bias=True, drop_path=0.0, shuffle_orders=False, pre_norm=True,
                    enable_rpe=False, enable_flash=False, upcast_attention=False, upcast_softmax=False)
    torch.manual_seed(7)
    model = build_model(dict(type="DefaultSegmentorV2", num_classes=2, backbone_out_channels=16, backbone=backbone,
                             criteria=PIGSEG_CRITERIA)).to(dev)
    data = S.make_batch([350, 250], in_channels=4, extent=48, seed=5)
    n = data["coord"].shape[0]
    g = torch.Generator().manual_seed(9)
    segment = torch.randint(0, 2, (n,), generator=g)
    segment[torch.rand(n, generator=g) < 0.15] = -1
    data = {k: v.to(dev) for k, v in data.items()}
    data["segment"] = segment.to(dev)
    model.train()
    for m in model.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            m.eval()
    res = model(dict(data))
    assert set(res) == {"loss"} and torch.isfinite(res["loss"]).item()
    res["loss"].backward()
    gw = model.seg_head.weight.grad
    assert gw is not None and torch.isfinite(gw).all() and gw.abs().max().item() > 0
    model.eval()
    with torch.no_grad():
        ev = model(dict(data))
    assert set(ev) == {"loss", "seg_logits"} and ev["seg_logits"].shape == (n, 2)
    focal, lovasz = build_criteria(PIGSEG_CRITERIA).criteria
    parts = focal(ev["seg_logits"], data["segment"]) + lovasz(ev["seg_logits"], data["segment"])
    print(f"train loss {res['loss'].item():.7f}, eval loss {ev['loss'].item():.7f}, modules on eval logits "
          f"{parts.item():.7f}")
    assert abs(ev["loss"].item() - parts.item()) <= 1e-5
    assert abs(res["loss"].item() - parts.item()) <= 1e-5
