"""The voting keypoint head on the GPU: the per-scene median kernel against CPU torch.median (exact), the fused vote loss
and its backward against a float64 torch-autograd restatement written here, KeypointSwin3DVote against the reference's
own outputs on a stand-in backbone (tests/golden/keypoint_vote_tiny.npz, which also pins the restatement), the fork
config on the Swin3D backbone (backbone parity UNPINNED, as every Swin3D test), and the KeypointEvaluator hook."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
MARGIN = 1e-4      # no (point, keypoint) distance this close to the radius: the mask is the same in any fp32 arithmetic


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _offset(sizes, dev, dtype=torch.int64):
    return torch.tensor(np.cumsum(sizes), dtype=dtype, device=dev)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------
# 1. scene_median
# ------------------------------------------------------------------------------------------------
SCENE_SETS = [[1, 2, 700, 0, 2501, 37], [100000] * 8, [5, 0, 0, 64, 65, 129]]
SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), 1e-40, -1e-40, 1.4e-45, -1.4e-45]


def _family(name, n, c, g):
    if name == "normal":
        return torch.randn(n, c, generator=g)
    if name == "column_constant":          # every value of a column equal
        return (torch.randn(1, c, generator=g) * 3).expand(n, c).contiguous()
    if name == "low_mantissa":             # the values of a column differ in the low 8 mantissa bits only
        base = (torch.randn(1, c, generator=g) * 3).view(torch.int32) & ~0xFF
        return (base | torch.randint(0, 256, (n, c), generator=g, dtype=torch.int32)).view(torch.float32)
    if name == "duplicates":               # 16 levels
        return (torch.randint(0, 16, (n, c), generator=g).float() - 8.0) * 0.25
    if name == "specials":                 # mixed signs with +-0, +-inf and denormals
        x = torch.randn(n, c, generator=g)
        pick = torch.randint(0, 3 * len(SPECIALS), (n, c), generator=g)
        sp = torch.tensor(SPECIALS)
        return torch.where(pick < len(SPECIALS), sp[pick.clamp(max=len(SPECIALS) - 1)], x)
    raise KeyError(name)


def _ref_median(x, sizes):
    """CPU torch.median(dim=0).values per scene, zeros for an empty scene (keypoint_swin3d_plus.py:172-187)."""
    out, s = [], 0
    for n in sizes:
        out.append(x[s:s + n].median(dim=0).values if n else torch.zeros(x.shape[1]))
        s += n
    return torch.stack(out)


@pytest.mark.parametrize("family", ["normal", "column_constant", "low_mantissa", "duplicates", "specials"])
@pytest.mark.parametrize("c", [3, 18, 32])
@pytest.mark.parametrize("sizes", SCENE_SETS, ids=["ragged", "8x100k", "tiny"])
def test_scene_median_equals_torch_median(dev, sizes, c, family):
    """A selection, so no tolerance: torch.equal against CPU torch.median per scene (lower middle for even sizes), zeros
    for empty scenes, int32 and int64 offsets alike, two runs bitwise equal."""
    from ptv3_hip import ops
    g = torch.Generator().manual_seed(1000 * len(sizes) + c)
    x = _family(family, sum(sizes), c, g)
    ref = _ref_median(x, sizes)
    xd = x.to(dev)
    got = ops.scene_median(xd, None, _offset(sizes, dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(sizes), c)
    assert torch.equal(got.cpu(), ref)
    for b, n in enumerate(sizes):
        if n == 0:
            assert torch.count_nonzero(got[b]).item() == 0
    again = ops.scene_median(xd, None, _offset(sizes, dev, torch.int32))
    assert torch.equal(_bits(got), _bits(again))


@pytest.mark.parametrize("family", ["normal", "column_constant", "low_mantissa", "duplicates"])
@pytest.mark.parametrize("c", [3, 18])
@pytest.mark.parametrize("sizes", SCENE_SETS, ids=["ragged", "8x100k", "tiny"])
def test_scene_median_with_coord_equals_torch(dev, sizes, c, family):
    """With coord the kernel adds coord[i, j % 3] in fp32 before selecting: the median of coord.repeat(1, C / 3) + x
    computed in fp32 torch (the same single rounding)."""
    from ptv3_hip import ops
    g = torch.Generator().manual_seed(2000 * len(sizes) + c)
    n = sum(sizes)
    x, coord = _family(family, n, c, g), torch.rand(n, 3, generator=g)
    ref = _ref_median(coord.repeat(1, c // 3) + x, sizes)
    got = ops.scene_median(x.to(dev), coord.to(dev), _offset(sizes, dev))
    assert torch.equal(got.cpu(), ref)
    again = ops.scene_median(x.to(dev), coord.to(dev), _offset(sizes, dev, torch.int32))
    assert torch.equal(_bits(got), _bits(again))


@pytest.mark.parametrize("c", [3, 18, 32])
@pytest.mark.parametrize("sizes", SCENE_SETS, ids=["ragged", "8x100k", "tiny"])
def test_scene_median_nan_poisons_one_entry_only(dev, sizes, c):
    """torch.median: a NaN in a column gives NaN for that (scene, column); every other entry is untouched."""
    from ptv3_hip import ops
    g = torch.Generator().manual_seed(3000 * len(sizes) + c)
    x = torch.randn(sum(sizes), c, generator=g)
    clean = _ref_median(x, sizes)
    scene = max(range(len(sizes)), key=lambda b: sizes[b])
    start = int(np.cumsum([0] + sizes)[scene])
    col = c // 2
    x[start + sizes[scene] // 3, col] = float("nan")
    x[start, col] = -float("nan")
    ref = _ref_median(x, sizes)
    assert torch.isnan(ref[scene, col]) and torch.isnan(ref).sum() == 1
    got = ops.scene_median(x.to(dev), None, _offset(sizes, dev)).cpu()
    assert torch.isnan(got[scene, col]) and torch.isnan(got).sum() == 1
    keep = ~torch.isnan(ref)
    assert torch.equal(got[keep], ref[keep]) and torch.equal(got[keep], clean[keep])


def test_scene_median_rejects_unsupported_widths(dev):
    from ptv3_hip import ops
    with pytest.raises(RuntimeError, match="c=33 unsupported"):
        ops.scene_median(torch.zeros(10, 33, device=dev), None, _offset([10], dev))
    with pytest.raises(RuntimeError, match="multiple of 3"):
        ops.scene_median(torch.zeros(10, 32, device=dev), torch.zeros(10, 3, device=dev), _offset([10], dev))


# ------------------------------------------------------------------------------------------------
# 2. vote_loss forward and backward
# ------------------------------------------------------------------------------------------------
def _restated_vote_loss(votes, coord, target_pp, scale_pp, radius):
    """keypoint_swin3d_plus.py:84-164 in float64 torch.  votes (N, 3K) fp32 leaf, coord (N, 3) fp32, target_pp (N, K, 3)
    per point, scale_pp (N,) or None.  The predicted position is the reference's fp32 `coord + offset` (:84, one
    rounding, the same one the kernel makes); everything after it is float64.
    -> (loss, [masked_dist_err, kp0.., kpK-1], [mask total, per keypoint])"""
    n, k = target_pp.shape[:2]
    pred = (coord.unsqueeze(1) + votes.view(n, k, 3)).double()
    t, c = target_pp.double(), coord.double()
    dist = torch.norm(c.unsqueeze(1) - t, p=2, dim=-1)
    mask = dist < radius
    loss_all = F.smooth_l1_loss(pred, t, reduction="none").mean(dim=-1)
    m = mask.double()
    loss = (loss_all * m).sum() / m.sum().clamp(min=1.0)
    real = dist if scale_pp is None else dist * scale_pp.double().view(-1, 1)
    curves = [(real * m).sum() / m.sum() if m.sum() > 0 else torch.zeros(())]
    for j in range(k):
        cj = m[:, j].sum()
        curves.append((real[:, j] * m[:, j]).sum() / cj if cj > 0 else torch.zeros(()))
    counts = [int(mask.sum())] + [int(mask[:, j].sum()) for j in range(k)]
    return loss, torch.stack([torch.as_tensor(v, dtype=torch.float64) for v in curves]).detach(), counts, dist


def _vote_case(sizes, k, layout, radius, start_seed):
    """Seeded inputs whose (point, keypoint) distances all keep MARGIN from the radius (the first such seed)."""
    n, b = sum(sizes), len(sizes)
    batch = torch.repeat_interleave(torch.arange(b), torch.tensor(sizes))
    for seed in range(start_seed, start_seed + 100000):
        g = torch.Generator().manual_seed(seed)
        coord = torch.rand(n, 3, generator=g)
        target = torch.rand(b * k, 3, generator=g) * 0.7 + 0.15
        tpp = target.view(b, k, 3)[batch]
        if layout == "point":
            tpp = (tpp + torch.randn(n, k, 3, generator=g) * 0.02).contiguous()
        dist = torch.norm(coord.double().unsqueeze(1) - tpp.double(), dim=-1)
        if (dist - radius).abs().min().item() >= MARGIN:
            votes = torch.randn(n, 3 * k, generator=g) * 0.9       # residuals on both sides of |d| = 1
            scale = {"scene": torch.rand(b, generator=g) + 0.5, "point": torch.rand(n, generator=g) + 0.5}
            return coord, votes, (tpp if layout == "point" else target), tpp, scale, batch
    raise AssertionError("no seed keeps the margin")


VOTE_SIZES = [700, 0, 1300, 257]


@pytest.mark.parametrize("scale_kind", [None, "scene", "point", "scene_column"])
@pytest.mark.parametrize("layout", ["scene", "scene_3d", "point"])
def test_vote_loss_forward_backward_vs_float64_restatement(dev, layout, scale_kind):
    """Loss and curves within 1e-5 relative, dvotes within 1e-6 relative elementwise (the tolerances of
    test_hip_keypoint_regression.py), the mask count exact, two runs bitwise equal; an empty scene in the batch."""
    from ptv3_hip import autograd as A
    k, radius = 6, 0.4
    coord, votes, target, tpp, scales, batch = _vote_case(VOTE_SIZES, k, "point" if layout == "point" else "scene",
                                                          radius, 100)
    if layout == "scene_3d":
        target = target.view(len(VOTE_SIZES), k, 3)
    scale = None if scale_kind is None else scales[scale_kind.split("_")[0]]
    scale_pp = None if scale is None else (scale if scale_kind == "point" else scale[batch])
    if scale_kind == "scene_column":
        scale = scale.view(-1, 1)
    vr = votes.clone().requires_grad_(True)
    loss_r, curves_r, counts_r, dist = _restated_vote_loss(vr, coord, tpp, scale_pp, radius)
    assert (dist - radius).abs().min().item() >= MARGIN
    (loss_r * 1.7).backward()
    resid = (coord.unsqueeze(1) + votes.view(-1, k, 3) - tpp)[dist < radius].abs()
    assert (resid < 1).any() and (resid > 1).any()
    off = _offset(VOTE_SIZES, dev)
    runs = []
    for _ in range(2):
        vh = votes.to(dev).requires_grad_(True)
        loss, curves, count = A.vote_loss(vh, coord.to(dev), target.to(dev), off, radius,
                                          None if scale is None else scale.to(dev))
        (loss * 1.7).backward()
        runs.append((loss.detach(), curves, count, vh.grad))
    loss, curves, count, grad = runs[0]
    assert loss.dim() == 0 and not curves.requires_grad and not count.requires_grad
    assert count.cpu().tolist() == counts_r
    print("loss", loss.item(), loss_r.item(), "curves", curves.cpu().tolist(), curves_r.tolist())
    assert abs(loss.item() - loss_r.item()) <= 1e-5 * abs(loss_r.item())
    assert ((curves.double().cpu() - curves_r).abs() <= 1e-5 * curves_r.abs()).all()
    ref = vr.grad.double()
    err = (grad.double().cpu() - ref).abs()
    print("dvotes worst relative error", (err / ref.abs().clamp(min=1e-30)).max().item())
    assert (err <= 1e-6 * ref.abs()).all()
    assert (ref != 0).any() and (grad.cpu()[ref == 0] == 0).all()
    for first, second in zip(runs[0], runs[1]):      # int32 views of the float results: bitwise
        assert torch.equal(first.view(torch.int32), second.view(torch.int32))


def test_vote_loss_with_nothing_inside_the_radius(dev):
    """A radius so small that no pair is masked: loss 0, gradient 0, curves 0, count 0 (div = max(count, 1))."""
    from ptv3_hip import autograd as A
    k = 6
    coord, votes, target, tpp, scales, _ = _vote_case(VOTE_SIZES, k, "scene", 1e-6, 7)
    vh = votes.to(dev).requires_grad_(True)
    loss, curves, count = A.vote_loss(vh, coord.to(dev), target.to(dev), _offset(VOTE_SIZES, dev), 1e-6,
                                      scales["scene"].to(dev))
    loss.backward()
    assert loss.item() == 0.0 and torch.count_nonzero(curves).item() == 0 and torch.count_nonzero(count).item() == 0
    assert torch.count_nonzero(vh.grad).item() == 0


def test_vote_loss_bad_target_shape_raises(dev):
    from ptv3_hip import ops
    n, k = 50, 6
    votes, coord = torch.zeros(n, 3 * k, device=dev), torch.zeros(n, 3, device=dev)
    with pytest.raises(ValueError, match="Target shape mismatch"):
        ops.vote_loss(votes, coord, torch.zeros(2 * k + 1, 3, device=dev), _offset([20, 30], dev), 0.4)


# ------------------------------------------------------------------------------------------------
# 3. the model against the reference's own outputs
# ------------------------------------------------------------------------------------------------
def _register_stand_in():
    from pointcept.models import MODELS
    from pointcept.models.utils.hip_layers import Linear
    if MODELS.get("VoteStandInBackbone") is None:
        @MODELS.register_module("VoteStandInBackbone")
        class VoteStandInBackbone(nn.Module):
            """The generator's stand-in backbone: Linear(4, channels[0]) on data_dict["feat"]."""

            def __init__(self, channels):
                super().__init__()
                self.lin = Linear(4, channels[0])

            def forward(self, data_dict):
                return self.lin(data_dict["feat"].contiguous())


def _golden(golden_dir, dev):
    from pointcept.models import build_model
    _register_stand_in()
    g = np.load(os.path.join(golden_dir, "keypoint_vote_tiny.npz"))
    model = build_model(dict(type="KeypointSwin3DVote", num_keypoints=6, hidden_dim=32, vote_radius=float(g["vote_radius"]),
                             backbone_conf=dict(type="VoteStandInBackbone", channels=[16])))
    model.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd_")}, strict=True)
    data = {k[3:]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("in_")}
    return g, model.to(dev), data


def test_vote_model_eval_vs_reference_golden(dev, golden_dir):
    """Eval `pred` within FP32_TOL absolute of the reference's: the median is 1-Lipschitz in the sup norm, so its error is
    bounded by the error of the votes.  Nothing but `pred` is returned; int32 offsets give the same result."""
    g, model, data = _golden(golden_dir, dev)
    model.eval()
    keep = {k: v.clone() for k, v in data.items()}
    with torch.no_grad():
        out = model(data)
    assert sorted(out.keys()) == ["pred"]
    assert set(data.keys()) == set(keep.keys())      # a backbone that is not the Swin3D UNet gets the dict untouched
    assert tuple(out["pred"].shape) == (3, 6, 3) and out["pred"].dtype == torch.float32
    err = np.abs(out["pred"].cpu().numpy() - g["eval_pred"]).max()
    print("eval pred max abs error", err)
    assert err < FP32_TOL
    with torch.no_grad():
        out32 = model(dict(data, offset=data["offset"].int()))
    assert torch.equal(_bits(out32["pred"]), _bits(out["pred"]))


def test_vote_model_train_step_vs_reference_golden(dev, golden_dir):
    """One training step (Dropout at p = 0): loss and curves within FP32_TOL relative, the mask count exact, every
    parameter gradient as test_keypoint_ptv3_train_step_vs_reference_golden compares its golden, the BatchNorm running
    statistics within FP32_TOL.  The float64 restatement of test 2 on the model's own votes is held to the reference's
    loss and curves here as well, which pins it."""
    from ptv3_hip import ops
    g, model, data = _golden(golden_dir, dev)
    model.train()
    model.vote_head[3].p = 0.0
    cap = {}
    model.vote_head[7].register_forward_hook(lambda m, i, o: cap.__setitem__("votes", o.detach().float()))
    out = model(dict(data))
    out["loss"].backward()
    keys = ["loss", "train/masked_dist_err"] + [f"train/kp{i}_dist_err" for i in range(6)]
    assert sorted(out.keys()) == sorted(keys)
    assert all(isinstance(out[k], torch.Tensor) and out[k].dim() == 0 and out[k].is_cuda for k in keys)
    assert not any(out[k].requires_grad for k in keys[1:])
    want = np.concatenate([[float(g["loss"]), float(g["masked_dist_err"])], g["kp_dist_err"]]).astype(np.float64)
    got = np.array([out[k].item() for k in keys])
    print("loss and curves", got.tolist(), want.tolist())
    assert (np.abs(got - want) <= FP32_TOL * np.abs(want)).all()
    radius = float(g["vote_radius"])
    _, count = ops.vote_loss(cap["votes"].contiguous(), data["coord"], data["target"], data["offset"], radius,
                             data["scale"])
    assert count.cpu().tolist() == g["mask_count"].tolist()
    # the restatement against the reference's numbers
    sizes = np.diff(np.concatenate([[0], g["in_offset"]]))
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.from_numpy(sizes))
    tpp = data["target"].cpu().view(len(sizes), 6, 3)[batch]
    loss_r, curves_r, counts_r, dist = _restated_vote_loss(cap["votes"].cpu(), data["coord"].cpu(), tpp,
                                                           data["scale"].cpu()[batch], radius)
    assert (dist - radius).abs().min().item() >= MARGIN and counts_r == g["mask_count"].tolist()
    restated = np.concatenate([[loss_r.item()], curves_r.numpy()])
    assert (np.abs(restated - want) <= FP32_TOL * np.abs(want)).all()
    # gradients
    grads = {k[5:]: torch.from_numpy(g[k].astype(np.float32) * g["gmax_" + k[5:]]) for k in g.files
             if k.startswith("grad_")}
    gmax = max(float(g[k]) for k in g.files if k.startswith("gmax_"))
    # a Linear bias in front of a batch-statistic BatchNorm has an exact gradient of zero (the batch mean removes any
    # shift): both sides hold rounding noise, so it is held to noise level against that layer's weight
    noise = ("vote_head.0.bias", "vote_head.4.bias")
    for name in noise:
        lin = model.vote_head[int(name.split(".")[1])]
        assert lin.bias.grad.abs().max().item() <= 1e-4 * grads[name.replace("bias", "weight")].abs().max().item(), name
    assert set(grads) == {n for n, _ in model.named_parameters()}
    worst = max(((n, (p.grad.float().cpu() - grads[n]).abs().max().item()
                  / max(grads[n].abs().max().item(), 1e-3 * gmax)) for n, p in model.named_parameters()
                 if n not in noise), key=lambda t: t[1])
    print("worst gradient", worst)
    assert worst[1] < 2e-3, worst
    for n, b in model.named_buffers():
        if "running" in n:
            ref = torch.from_numpy(g["buf_" + n])
            assert (b.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6) < FP32_TOL, n


# ------------------------------------------------------------------------------------------------
# 4. the fork config on the Swin3D backbone (backbone parity UNPINNED)
# ------------------------------------------------------------------------------------------------
def test_fork_vote_config_on_swin3d_backbone_unpinned(dev):
    """configs/my_dataset/keypoint_swin3d_plus.py with the "Swin3D-v1m1" backbone on a two-scene batch.  The backbone's
    parity is UNPINNED, as in every Swin3D test (MinkowskiEngine is restated, not run), so the check is on what this
    model adds: in eval `pred` equals EXACTLY the per-scene torch.median of coord + the model's own votes (captured
    behind vote_head[7]); two evals are bitwise equal; one training step is finite and returns exactly the reference's
    key set."""
    from test_hip_swin3d import _swin_batch, _randomise, _to_dev
    from pointcept.models import build_model
    from ptv3_hip import configs
    batch = _swin_batch([11000, 9000], seed=16, sig_dim=4, feat_dim=4, dup=0.0)
    batch["feat"] = np.clip(batch.pop("coord_feat"), -1, 1)
    model = build_model(dict(configs.KEYPOINT_SWIN3D_VOTE_CFG))
    _randomise(model, 23)
    model = model.to(dev).eval()
    cap = {}
    hook = model.vote_head[7].register_forward_hook(lambda m, i, o: cap.__setitem__("votes", o.detach().float()))
    data = _to_dev(batch, dev)
    with torch.no_grad():
        pred = model(dict(data))["pred"]
        votes = cap["votes"].cpu()
        again = model(dict(data))["pred"]
    assert tuple(pred.shape) == (2, 6, 3) and torch.isfinite(pred).all()
    coord = data["coord"].cpu()
    per_point = coord.unsqueeze(1) + votes.view(-1, 6, 3)
    sizes = np.diff(np.concatenate([[0], batch["offset"]])).tolist()
    ref = torch.stack([seg.median(dim=0).values for seg in torch.split(per_point, sizes)])
    assert torch.equal(pred.cpu(), ref)
    assert torch.equal(_bits(pred), _bits(again))
    hook.remove()
    model.train()
    g = torch.Generator().manual_seed(4)
    starts = np.concatenate([[0], batch["offset"][:-1]])
    pick = torch.cat([torch.randint(int(s), int(s) + int(n), (6,), generator=g) for s, n in zip(starts, sizes)])
    data["target"] = data["coord"][pick.to(dev)] + 0.01
    data["scale"] = torch.tensor([1.5, 0.7], device=dev)
    out = model(dict(data))
    out["loss"].backward()
    assert sorted(out.keys()) == sorted(["loss", "train/masked_dist_err"] + [f"train/kp{i}_dist_err" for i in range(6)])
    assert all(torch.isfinite(v).item() for v in out.values())
    assert out["loss"].item() > 0 and out["train/masked_dist_err"].item() > 0
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all() for gr in grads)
    assert model.vote_head[7].weight.grad.abs().max().item() > 0


# ------------------------------------------------------------------------------------------------
# 5. KeypointEvaluator
# ------------------------------------------------------------------------------------------------
def test_keypoint_evaluator_over_vote_model(dev, golden_dir):
    """The hook over two batches of KeypointSwin3DVote: the totals evaluate_batch gives on the model's `pred`."""
    from pointcept.engines.hooks.builder import HOOKS
    from pointcept.engines.hooks.keypoint_evaluator import evaluate_batch
    import pointcept.engines.hooks  # noqa: F401
    g, model, data = _golden(golden_dir, dev)
    second = dict(data, feat=data["feat"].flip(0).contiguous(), coord=data["coord"].flip(0).contiguous())
    del second["scale"]
    model.eval()
    totals = torch.zeros(2, device=dev)
    with torch.no_grad():
        for d in (data, second):
            totals += evaluate_batch(model(dict(d))["pred"], d["target"], d.get("scale"))
    total, count = totals.tolist()
    assert count == 6.0
    logs = []
    trainer = types.SimpleNamespace(val_loader=[dict(data), dict(second)], model=model.train(),
                                    logger=types.SimpleNamespace(info=logs.append), comm_info={})
    hook = HOOKS.build(dict(type="KeypointEvaluator"))
    hook.trainer = trainer
    hook.after_epoch()
    mean = total / (count + 1e-6)
    assert not model.training
    assert abs(trainer.comm_info["current_metric_value"] + mean) < 1e-6
    assert trainer.comm_info["current_metric_name"] == "mean_dist"
    assert f"Eval Result: Mean Distance = {mean:.4f}" in logs
