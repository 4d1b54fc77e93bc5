"""KeypointPTv2 on the GPU: the fused grouped vector attention against the same formula in float64 torch (shapes, masked
slots, determinism, canary), the grid-pool plan against numpy, the model against the reference's own outputs
(tests/golden/keypoint_ptv2_tiny.npz: eval, per-level partitions and taps, one training step), the fused eval forward
against the torch composition, and the fork config end to end."""
import os

import numpy as np
import pytest
import torch

from make_golden_keypoint_ptv2 import (seeded_state_dict, TINY_KW, TINY_SHAPES, TAP_STRIDE, MARGIN, FP16_STEP,  # noqa: E402
                                       cell_margin, unpack_grads, _zero_bias)

pytestmark = pytest.mark.gpu

# fp32 torch (CPU) against float64 on the fixture's batch, as tests/golden/make_golden_keypoint_ptv2.py printed them
# (stored in the fixture as gap_*; test_fixture_gaps_are_the_stated_ones pins the two together).  Every tolerance below is
# four times its gap: the rule of DESIGN.md sections 13 and 14.
GAPS = {
    "enc0": 2.249e-07, "dec0": 2.861e-07, "enc1": 2.457e-07, "dec1": 3.456e-07, "enc2": 2.380e-07, "dec2": 4.308e-07,
    "enc3": 2.951e-07, "dec3": 4.254e-07,      # stage features, relative to max(1, max|feature|)
    "pred": 4.731e-07, "eval_loss": 6.866e-08,
    "loss": 3.409e-06, "mean_dist": 2.769e-06, "kp_dist": 1.397e-05,
    "grad_head": 2.009e-04, "grad_backbone": 2.370e-02,     # relative to max(max|grad|, 1e-3 * the largest gradient)
    "buf": 4.245e-07,                                       # running statistics, relative to the buffer's maximum
}
MARGIN4 = 4.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------
# grouped vector attention
# ------------------------------------------------------------------------------------------------
def _gva_formula(layer, p, q, k, v, idx, dtype, renormalise=False):
    """GroupedVectorAttention.forward after the input projections (point_transformer_v2m2_base.py:116-136) with
    running-statistic BatchNorm, written out in `dtype` torch.  A neighbour is missing where idx lies outside [0, n).
    renormalise = True is NOT the reference: the softmax runs over the present neighbours only."""
    def lin(m, t):
        return t @ m.weight.to(dtype).T + m.bias.to(dtype)

    def bn(m, t):
        m = m.norm
        return (t - m.running_mean.to(dtype)) / torch.sqrt(m.running_var.to(dtype) + m.eps) * m.weight.to(dtype) \
            + m.bias.to(dtype)
    p, q, k, v = (t.to(dtype) for t in (p, q, k, v))
    n, ns = idx.shape
    c, g = q.shape[1], layer.groups
    present = (idx >= 0) & (idx < n)
    have = present.to(dtype).unsqueeze(-1)
    j = idx.long().clamp(0, n - 1)
    pos = (p[j] - p.unsqueeze(1)) * have
    lp, lw = layer.linear_p_bias, layer.weight_encoding
    peb = lin(lp[3], torch.relu(bn(lp[1], lin(lp[0], pos))))
    r = k[j] * have - q.unsqueeze(1) + peb
    w = lin(lw[3], torch.relu(bn(lw[1], lin(lw[0], r))))
    if renormalise:
        w = torch.softmax(w.masked_fill(~present.unsqueeze(-1), float("-inf")), dim=1)
        w = torch.nan_to_num(w)
    else:
        w = torch.softmax(w, dim=1) * have
    return ((v[j] * have + peb).view(n, ns, g, c // g) * w.unsqueeze(-1)).sum(1).reshape(n, c)


def _layer(c, g, dev, seed):
    from pointcept.models.point_transformer_v2.point_transformer_v2m2_base import GroupedVectorAttention
    torch.manual_seed(seed)
    layer = GroupedVectorAttention(c, g)
    for m in layer.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.normal_(1.0, 0.1)
            m.bias.data.normal_(0, 0.1)
    return layer.to(dev).eval()


def _kernel_args(layer, q, k, v, p, idx):
    from ptv3_hip import ops
    lp, lw = layer.linear_p_bias, layer.weight_encoding
    f = lambda t: t.detach().float().contiguous()   # noqa: E731
    return (q, k, v, p, idx, layer.groups, f(lp[0].weight), *ops.fold_batchnorm(lp[1].norm, lp[0].bias),
            f(lp[3].weight), f(lp[3].bias), f(lw[0].weight), *ops.fold_batchnorm(lw[1].norm, lw[0].bias),
            f(lw[3].weight), f(lw[3].bias))


# the tiny model's five shapes on 709 rows (scenes of 1, 7 and 701 points: rows of -1, and no multiple of any tile), then
#   (24, 3, 5, 37)    C no multiple of 16: a half-empty last column tile and K chunk; 37 rows: a ragged last workgroup
#   (64, 4, 16, 130)  I = 16 channels per group
#   (32, 32, 3, 65)   I = 1: one weight per channel
#   (512, 64, 16, 70) the widest layer: W_p2 (1 MB) streams, four group-column tiles, few points per workgroup
#   (48, 6, 1, 100)   ns = 1: the softmax of one slot
#   (64, 8, 32, 45)   ns = 32: the most slots
GVA_SHAPES = [(c, g, ns, 709) for c, g, ns in TINY_SHAPES] + [
    (24, 3, 5, 37), (64, 4, 16, 130), (32, 32, 3, 65), (512, 64, 16, 70), (48, 6, 1, 100), (64, 8, 32, 45)]


@pytest.mark.parametrize("c,g,ns,n", GVA_SHAPES)
def test_gva_vs_float64(dev, c, g, ns, n):
    """Yardstick E = the same formula in fp32 torch against float64: the kernel stays within 4 E (a different summation
    order); two runs are bitwise equal."""
    import pointops
    from ptv3_hip import ops
    layer = _layer(c, g, dev, c + g + ns)
    sizes = [1, 7, n - 8]
    p = torch.rand(n, 3, device=dev)
    off = torch.tensor(np.cumsum(sizes), dtype=torch.int32, device=dev)
    idx, _ = pointops.knn_query(ns, p, off)
    if ns > 1:
        assert (idx[:8] < 0).any()
    assert (idx[8:] >= 0).all()
    q, k, v = (torch.randn(n, c, device=dev) for _ in range(3))
    args = _kernel_args(layer, q, k, v, p, idx)
    got = ops.grouped_vector_attention(*args)
    assert torch.equal(got, ops.grouped_vector_attention(*args))
    with torch.no_grad():
        ref = _gva_formula(layer, p, q, k, v, idx, torch.float64)
        e32 = (_gva_formula(layer, p, q, k, v, idx, torch.float32).double() - ref).abs().max().item()
    err = (got.double() - ref).abs().max().item()
    print(f"gva c={c} g={g} ns={ns} n={n}: err {err:.3e}, fp32 torch E {e32:.3e}, max|ref| {ref.abs().max().item():.3f}")
    assert err <= MARGIN4 * e32, (err, e32)


def test_gva_masked_slots_and_canary(dev):
    """Row r has r mod 8 missing neighbours (0 to ns - 1 of them, in scattered slots), written as -1 in the first half of
    the rows and as out-of-range values (n, n + 5, 2^31 - 1, -7) in the second.  The float64 statement (softmax over all
    slots, then the mask) differs from a softmax renormalised over the present slots by more than the tolerance, so
    the masking order is what is tested.  The output row behind the last one stays untouched."""
    from ptv3_hip import ops
    from ptv3_hip.lib import lib
    c, g, ns, n = 48, 6, 8, 83
    layer = _layer(c, g, dev, 11)
    gen = torch.Generator().manual_seed(3)
    p = torch.rand(n, 3, generator=gen).to(dev)
    idx = torch.randint(0, n, (n, ns), generator=gen, dtype=torch.int32)
    bad = [n, n + 5, 2 ** 31 - 1, -7]
    for r in range(n):
        slots = torch.randperm(ns, generator=gen)[:r % ns]
        for t, s in enumerate(slots.tolist()):
            idx[r, s] = -1 if r < n // 2 else bad[(r + t) % 4]
    idx = idx.to(dev)
    missing = ((idx < 0) | (idx >= n)).sum(1)
    assert missing.min().item() == 0 and missing.max().item() == ns - 1
    q, k, v = (torch.randn(n, c, generator=gen).to(dev) for _ in range(3))
    args = _kernel_args(layer, q, k, v, p, idx)
    got = ops.grouped_vector_attention(*args)
    with torch.no_grad():
        ref = _gva_formula(layer, p, q, k, v, idx, torch.float64)
        e32 = (_gva_formula(layer, p, q, k, v, idx, torch.float32).double() - ref).abs().max().item()
        renorm = _gva_formula(layer, p, q, k, v, idx, torch.float64, renormalise=True)
    tol = MARGIN4 * e32
    err = (got.double() - ref).abs().max().item()
    apart = (renorm - ref).abs().max().item()
    print(f"gva masked: err {err:.3e}, fp32 torch E {e32:.3e}, renormalised softmax differs by {apart:.3e}")
    assert apart > tol
    assert err <= tol, (err, e32)
    # -1 and out-of-range indices are one and the same
    same = ops.grouped_vector_attention(*args[:4], torch.where((idx < 0) | (idx >= n), -1, idx).int(), *args[5:])
    assert torch.equal(got, same)
    # canary: the kernel writes n rows and nothing behind them
    big = torch.full((n + 1, c), -7.0, device=dev)
    a = args
    lib.check(lib.ptv3_gva_fwd(*[t.data_ptr() for t in a[:5]], n, c, g, ns, *[t.data_ptr() for t in a[6:]],
                               big.data_ptr(), torch.cuda.current_stream().cuda_stream), "ptv3_gva_fwd")
    torch.cuda.synchronize()
    assert torch.equal(big[:n], got) and (big[n] == -7.0).all()


def test_gva_refuses_unsupported_shapes(dev):
    from ptv3_hip import ops
    n = 10
    p = torch.rand(n, 3, device=dev)
    w = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731
    for c, g, ns, msg in ((12, 1, 8, "c=12 unsupported"), (64, 5, 8, "groups=5 unsupported"), (64, 8, 33, "ns=33 unsupported")):
        x = w(n, c)
        idx = torch.zeros(n, ns, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match=msg):
            ops.grouped_vector_attention(x, x, x, p, idx, g, w(c, 3), w(c), w(c), w(c, c), w(c), w(g, c), w(g), w(g),
                                         w(g, g), w(g))
    assert ops.grouped_vector_attention(w(0, 64), w(0, 64), w(0, 64), w(0, 3),
                                        torch.zeros(0, 16, dtype=torch.int32, device=dev), 8, w(64, 3), w(64), w(64),
                                        w(64, 64), w(64), w(8, 64), w(8), w(8), w(8, 8), w(8)).shape == (0, 64)


# ------------------------------------------------------------------------------------------------
# grid pooling
# ------------------------------------------------------------------------------------------------
def test_grid_pool_plan_vs_numpy(dev):
    """Four scenes (seed searched on the CPU for the cell margin, asserted here): 500 points in a unit cube, ONE point,
    100 points that all lie in one cell, 300 points in a 0.7 cube; cell size 0.1.  cluster map, sorted order, counts,
    pooled offsets: exact.  Coordinate mean: within 4 fp32 roundings (of the largest coordinate) per summand of the float64 mean.  Feature max: exact."""
    from ptv3_hip import ops
    rs = np.random.RandomState(5)
    coord = np.concatenate([rs.rand(500, 3).astype(np.float32) * 1.0 + 3, rs.rand(1, 3).astype(np.float32),
                            (rs.rand(100, 3) * 0.05 + 1.02).astype(np.float32), rs.rand(300, 3).astype(np.float32) * 0.7 - 2])
    ends = np.array([500, 501, 601, 901])
    margin, same, cells, batch = cell_margin(coord, ends, 0.1)
    assert margin >= MARGIN and same
    assert len(np.unique(cells[501:601], axis=0)) == 1
    key = ((batch * 64 + cells[:, 2]) * 64 + cells[:, 1]) * 64 + cells[:, 0]
    _, cluster, counts = np.unique(key, return_inverse=True, return_counts=True)
    order = np.argsort(cluster, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(counts)])
    feat = rs.randn(901, 8).astype(np.float32)
    for off_dtype in (torch.int32, torch.int64):
        plan = ops.grid_pool_plan(torch.from_numpy(coord).to(dev), torch.from_numpy(ends).to(dev).to(off_dtype), 0.1)
        assert plan.n_out == len(counts)
        assert np.array_equal(plan.cluster.cpu().numpy(), cluster)
        assert np.array_equal(plan.order.cpu().numpy(), order)
        assert np.array_equal(plan.seg_start.cpu().numpy(), ptr)
        pooled_ends = np.cumsum(np.bincount(batch[order[ptr[:-1]]], minlength=4))
        assert plan.offset_host == pooled_ends.tolist() and np.array_equal(plan.offset.cpu().numpy(), pooled_ends)
        assert pooled_ends[1] - pooled_ends[0] == 1 and pooled_ends[2] - pooled_ends[1] == 1
        starts = np.stack([coord[batch == b].min(0) for b in range(4)])
        assert np.array_equal(plan.start.cpu().numpy(), starts)
    mean = ops.segment_mean3(torch.from_numpy(coord).to(dev), plan.order, plan.seg_start, plan.n_out).cpu().numpy()
    want = np.stack([coord[order[a:b]].astype(np.float64).mean(0) for a, b in zip(ptr[:-1], ptr[1:])])
    bound = 4 * 2.0 ** -24 * np.abs(coord).max() * counts[:, None]
    assert (np.abs(mean - want) <= bound).all()
    assert np.array_equal(mean[pooled_ends[0]], coord[500])        # the one-point scene is its own mean
    mx = ops.pool_max(torch.from_numpy(feat).to(dev), plan.order, plan.seg_start, plan.n_out).cpu().numpy()
    assert np.array_equal(mx, np.stack([feat[order[a:b]].max(0) for a, b in zip(ptr[:-1], ptr[1:])]))


def test_grid_pool_plan_refuses_what_the_key_cannot_hold(dev):
    from ptv3_hip import ops
    coord = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]], device=dev)
    with pytest.raises(ValueError, match="more than 131072 cells"):
        ops.grid_pool_plan(coord, torch.tensor([2], device=dev), 1e-6)
    with pytest.raises(ValueError, match="a scene without points"):
        ops.grid_pool_plan(coord, torch.tensor([2, 2], device=dev), 0.5)


# ------------------------------------------------------------------------------------------------
# the model against the reference's own outputs
# ------------------------------------------------------------------------------------------------
def _tiny(golden_dir, dev):
    from pointcept.models import build_model
    g = np.load(os.path.join(golden_dir, "keypoint_ptv2_tiny.npz"))
    model = build_model(dict(type="KeypointPTv2", **TINY_KW))
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    data = {k[3:]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("in_")}
    return g, model.to(dev), data


def _tapped_eval(model, data):
    """Eval output and, per stage, the output features (enc{i} / dec{i}), pooled coordinates, offsets and cluster maps."""
    taps, hooks = {}, []
    bb = model.backbone
    for i in range(bb.num_stages):
        hooks.append(bb.enc_stages[i].register_forward_hook(
            lambda m, inp, out, i=i: taps.update({f"enc{i}": out[0][1].detach(), f"coord{i + 1}": out[0][0].detach(),
                                                  f"offset{i + 1}": out[0][2].detach(), f"cluster{i}": out[1].detach()})))
        hooks.append(bb.dec_stages[i].register_forward_hook(
            lambda m, inp, out, i=i: taps.__setitem__(f"dec{i}", out[1].detach())))
    with torch.no_grad():
        out = model.eval()(dict(data))
    for h in hooks:
        h.remove()
    return out, taps


def test_fixture_gaps_are_the_stated_ones(golden_dir):
    g = np.load(os.path.join(golden_dir, "keypoint_ptv2_tiny.npz"))
    for k, v in GAPS.items():
        assert abs(float(g["gap_" + k]) - v) <= 1e-3 * v, k


def test_keypoint_ptv2_eval_vs_reference_golden(dev, golden_dir):
    """Pooled row counts, cluster maps and offsets of every level: exact.  Pooled coordinates: within 2 fp32 roundings
    (of the largest coordinate) per summand.  Every stage's features, `pred` and `loss`: within four times the reference's own fp32-vs-float64 gap
    (GAPS)."""
    g, model, data = _tiny(golden_dir, dev)
    out, taps = _tapped_eval(model, data)
    for i in range(4):
        assert taps[f"coord{i + 1}"].shape[0] == int(g[f"count{i + 1}"])
        assert np.array_equal(taps[f"cluster{i}"].cpu().numpy(), g[f"cluster{i}"]), i
        assert np.array_equal(taps[f"offset{i + 1}"].cpu().numpy(), g[f"offset{i + 1}"]), i
        ref = g[f"coord{i + 1}"]
        counts = np.bincount(g[f"cluster{i}"])[:, None]
        bound = 2 * 2.0 ** -24 * np.abs(g["in_coord"]).max() * counts
        assert (np.abs(taps[f"coord{i + 1}"].cpu().numpy() - ref) <= bound).all(), i
    for i in range(4):
        for kind, level in (("enc", i + 1), ("dec", i)):
            ref = g[f"tap_{kind}{i}"]
            got = taps[f"{kind}{i}"].cpu().numpy()[::TAP_STRIDE[level]]
            err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
            print(f"{kind}{i}: err {err:.3e}, tolerance {MARGIN4 * GAPS[f'{kind}{i}']:.3e}")
            assert err <= MARGIN4 * GAPS[f"{kind}{i}"], (kind, i, err)
    assert tuple(out["pred"].shape) == (3, 6, 3) and out["pred"].dtype == torch.float32
    err = np.abs(out["pred"].cpu().numpy() - g["eval_pred"]).max()
    tol_pred = MARGIN4 * GAPS["pred"]
    print(f"pred: err {err:.3e}, tolerance {tol_pred:.3e}")
    assert err <= tol_pred
    tol_loss = MARGIN4 * GAPS["eval_loss"]
    err = abs(out["loss"].item() - float(g["eval_loss"]))
    print(f"eval loss: err {err:.3e}, tolerance {tol_loss:.3e}")
    assert err <= tol_loss
    with torch.no_grad():
        out64 = model(dict(data, offset=data["offset"].long()))
    assert torch.equal(out64["pred"], out["pred"])


def test_keypoint_ptv2_train_step_vs_reference_golden(dev, golden_dir):
    """Loss, curves, every parameter gradient and the running statistics of one training step (the head's Dropout at
    p = 0) within four times the reference's own fp32-vs-float64 gap; a gradient is held to the gap of its own tensor
    (gap_grads in the fixture: median 1.3e-3, nine in ten under 4.0e-3, the largest 2.4e-2 where batch-statistic BatchNorm over the few rows of
    the deepest level makes the reference itself that sensitive) and also carries its float16 step (2^-11 of the
    tensor's maximum)."""
    g, model, data = _tiny(golden_dir, dev)
    model.train()
    model.reg_head[3].p = 0.0
    out = model(dict(data))
    out["loss"].backward()
    assert abs(out["loss"].item() - float(g["loss"])) <= MARGIN4 * GAPS["loss"]
    assert abs(out["train/mean_dist"].item() - float(g["mean_dist"])) <= MARGIN4 * GAPS["mean_dist"]
    kp = np.array([out[f"train/kp{i}_dist"].item() for i in range(6)])
    assert np.abs(kp - g["kp_dist"]).max() <= MARGIN4 * GAPS["kp_dist"]
    params = dict(model.named_parameters())
    grads = unpack_grads(g["grads"], g["gmax"], {k: tuple(v.shape) for k, v in params.items()})
    gmax = float(g["gmax"].max())
    gaps = dict(zip(params, g["gap_grads"].tolist()))     # the reference's own fp32-vs-float64 gap of every tensor
    zero = [n for n in params if _zero_bias(n)]
    assert len(zero) == 1 + 4 * 10 + 2 * 4     # the head, four per block, two per unpooling
    for n in zero:
        weight = params[n[:-4] + "weight"].grad.abs().max().item()
        assert params[n].grad.abs().max().item() <= 1e-4 * weight, n
    worst = {"grad_head": 0.0, "grad_backbone": 0.0}
    for n, p in params.items():
        if n in zero:
            continue
        ref = torch.from_numpy(grads[n])
        err = (p.grad.float().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3 * gmax)
        kind = "grad_head" if n.startswith("reg_head.") else "grad_backbone"
        worst[kind] = max(worst[kind], err)
        assert err <= MARGIN4 * gaps[n] + FP16_STEP, (n, err, gaps[n])
    print("worst gradient errors", worst)
    bufs = [(n, b) for n, b in model.named_buffers() if "running" in n]
    flat, at = g["bufs"], 0
    for n, b in bufs:
        ref = torch.from_numpy(flat[at:at + b.numel()].reshape(tuple(b.shape)))
        at += b.numel()
        assert (b.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6) <= MARGIN4 * GAPS["buf"], n
    assert at == len(flat)


def test_eval_equals_torch_composition(dev, golden_dir):
    """The fused eval forward against the torch composition run in eval mode on the same weights, on every row of every
    stage: the partitions are identical, and the features lie within eight gaps of each other (each side within four of
    the float64 value)."""
    g, model, data = _tiny(golden_dir, dev)
    fused, taps = _tapped_eval(model, data)
    plain, ref_taps = _tapped_eval(model.set_fused(False), data)
    for i in range(4):
        assert torch.equal(taps[f"cluster{i}"], ref_taps[f"cluster{i}"])
        for kind in ("enc", "dec"):
            a, b = taps[f"{kind}{i}"], ref_taps[f"{kind}{i}"]
            err = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
            assert err <= 2 * MARGIN4 * GAPS[f"{kind}{i}"], (kind, i, err)
    assert (fused["pred"] - plain["pred"]).abs().max().item() <= 2 * MARGIN4 * GAPS["pred"]


def test_fork_config_eval(dev):
    """KeypointPTv2 from configs/my_dataset/keypoint_ptv2.py's model dict on two scenes of 3000 random points."""
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_PTV2_CFG
    torch.manual_seed(7)
    model = build_model(KEYPOINT_PTV2_CFG).to(dev)
    data = dict(coord=torch.rand(6000, 3, device=dev), feat=torch.randn(6000, 4, device=dev),
                offset=torch.tensor([3000, 6000], dtype=torch.int32, device=dev))
    with torch.no_grad():
        pred = model.eval()(dict(data))["pred"]
    assert tuple(pred.shape) == (2, 6, 3) and torch.isfinite(pred).all()
