"""KeypointPTv1 on the GPU: farthest point sampling against a float64 numpy restatement (exact rows), the fused vector
attention against the same formula in float64 torch, the model against the reference's own outputs
(tests/golden/keypoint_ptv1_tiny.npz: eval, per-stage taps, one training step), the fused eval forward against the torch
composition, and the fork config end to end."""
import os

import numpy as np
import pytest
import torch

from make_golden_keypoint_ptv1 import seeded_state_dict, TINY_KW, TAP_STRIDE  # noqa: E402

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
MARGIN = 2e-6     # relative gap winner / runner-up demanded of every test scene: 8x the fp32 rounding of a distance
# where ptv3_farthest_point_sampling moves a scene's state: registers -> + LDS -> + global memory (csrc/fps.hip)
REG_POINTS, LDS_POINTS = 16384, 8192
# past both, a thread walks its points in global memory three at a time (one every 1024) and then one at a time
FPS_THREADS = 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------
# farthest point sampling
# ------------------------------------------------------------------------------------------------
def _fps64(xyz, count):
    """One scene in float64: rows, final running distances, smallest relative gap winner / runner-up."""
    x = np.asarray(xyz, dtype=np.float64)
    d = np.full(len(x), 1e10)
    rows, gap, old = [0], np.inf, 0
    for _ in range(1, count):
        d = np.minimum(d, ((x - x[old]) ** 2).sum(1))
        old = int(np.argmax(d))
        if len(d) > 1:
            top2 = np.partition(d, -2)[-2:]
            gap = min(gap, (top2[1] - top2[0]) / top2[1]) if top2[1] > 0 else 0.0
        rows.append(old)
    return np.asarray(rows[:count], dtype=np.int64), d, gap


# seeds for which every selection of the scene clears MARGIN (searched on the CPU; _scene asserts it)
SEEDS = {(4100, 1025): 163}


def _scene(n, count):
    """n random points in the unit cube with its float64 sampling; hard-asserts the selection margin."""
    xyz = np.random.RandomState(SEEDS.get((n, count), 0)).rand(n, 3).astype(np.float32)
    rows, d, gap = _fps64(xyz, count)
    assert gap >= MARGIN, (n, count, gap)
    return xyz, rows, d


_BATCHES = {}


def _batch(key):
    """(xyz, offset, new_offset, rows, tmp) of a list of (n, count) scenes, built once."""
    if key not in _BATCHES:
        parts = [_scene(n, c) for n, c in key]
        ends = np.cumsum([n for n, _ in key])
        starts = np.concatenate([[0], ends[:-1]])
        rows = np.concatenate([r + s for (_, r, _), s in zip(parts, starts)]) if key else np.zeros(0, np.int64)
        _BATCHES[key] = (np.concatenate([p[0] for p in parts]), ends, np.cumsum([c for _, c in key]), rows,
                         np.concatenate([p[2] for p in parts]))
    return _BATCHES[key]


FPS_BATCHES = {
    # the small sizes around a wave and a workgroup; counts n // 4: zero samples for the first two scenes
    "ragged": tuple((n, n // 4) for n in (1, 3, 4, 5, 63, 64, 65, 1025, 4100)),
    "t256": ((200, 50), (256, 37)),                     # 256-thread variant
    "t1024": ((257, 64), (1024, 100)),                  # 1024 threads, one point each
    "p4": ((1025, 100), (4096, 200)),                   # four points per thread
    "lds": ((REG_POINTS + 616, 200), (300, 75)),        # past the registers: the tail sits in LDS
    "global": ((REG_POINTS + LDS_POINTS + 1424, 200),),  # past LDS too: the tail stays in global memory
    # 5 * 1024 + 333 points in global memory: threads below 333 own six of them (the three-deep loop twice), the
    # others five (the three-deep loop once, then the one-at-a-time loop twice)
    "global3": ((REG_POINTS + LDS_POINTS + 5 * FPS_THREADS + 333, 200),),
}


@pytest.mark.parametrize("name", list(FPS_BATCHES))
def test_fps_vs_float64(dev, name):
    """Exact rows against the float64 restatement; int32 and int64 offsets; final running distances within 1e-6
    relative, through pointops.farthest_point_sampling and through pointops._C; two runs bitwise equal."""
    import pointops
    from pointops import _C
    xyz, ends, new_ends, rows, d = _batch(FPS_BATCHES[name])
    x = torch.from_numpy(xyz).to(dev)
    off64, noff64 = torch.from_numpy(ends).to(dev), torch.from_numpy(new_ends).to(dev)
    got = pointops.farthest_point_sampling(x, off64, noff64)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), rows)
    again = pointops.farthest_point_sampling(x, off64.int(), noff64.int())
    assert torch.equal(got, again)
    sizes = np.diff(np.concatenate([[0], ends]))
    idx = torch.full((int(new_ends[-1]) + 1,), -7, dtype=torch.int32, device=dev)
    tmp = torch.full((len(xyz),), 1e10, dtype=torch.float32, device=dev)
    _C.farthest_point_sampling_cuda(len(ends), int(sizes.max()), x, off64.int(), noff64.int(), tmp, idx)
    assert torch.equal(idx[:-1], got) and idx[-1].item() == -7
    t = tmp.double().cpu().numpy()
    # a scene sampled once never updates its distances: both sides keep 1e10 there
    assert (np.abs(t - d) <= 1e-6 * np.abs(d)).all()


def test_fps_ties_and_zero_samples(dev):
    """A scene of identical points returns its first index repeated (ties go to the lowest index), also past the
    register tier; a last scene asked for zero samples leaves the slot behind the output untouched."""
    from pointops import _C
    xyz, _, _ = _scene(100, 25)
    same = np.tile(np.float32([[0.25, 0.5, 0.75]]), (300, 1))
    tail = np.random.RandomState(1).rand(3, 3).astype(np.float32)
    x = torch.from_numpy(np.concatenate([xyz, same, tail])).to(dev)
    off = torch.tensor([100, 400, 403], dtype=torch.int32, device=dev)
    noff = torch.tensor([25, 45, 45], dtype=torch.int32, device=dev)
    idx = torch.full((46,), -7, dtype=torch.int32, device=dev)
    tmp = torch.full((403,), 1e10, dtype=torch.float32, device=dev)
    _C.farthest_point_sampling_cuda(3, 300, x, off, noff, tmp, idx)
    got = idx.cpu().numpy()
    assert np.array_equal(got[:25], _fps64(xyz, 25)[0])
    assert (got[25:45] == 100).all() and got[45] == -7
    import pointops
    # identical points in every tier: registers, LDS, and in global memory both the three-deep and the single loop
    for n in (REG_POINTS + LDS_POINTS + 100, REG_POINTS + LDS_POINTS + 5 * FPS_THREADS + 333):
        big = torch.from_numpy(np.tile(np.float32([[1.0, 2.0, 3.0]]), (n, 1))).to(dev)
        rows = pointops.farthest_point_sampling(big, torch.tensor([n], device=dev), torch.tensor([9], device=dev))
        assert rows.shape == (9,) and (rows == 0).all(), n


def test_fps_of_no_scene_is_empty(dev):
    import pointops
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    rows = pointops.farthest_point_sampling(torch.zeros(0, 3, device=dev), none, none)
    assert rows.dtype == torch.int32 and rows.shape == (0,)


# ------------------------------------------------------------------------------------------------
# vector attention
# ------------------------------------------------------------------------------------------------
def _attention_formula(layer, p, x_q, x_k, x_v, idx, dtype):
    """PointTransformerLayer.forward after the input projections (point_transformer_seg.py:90-120) with running-statistic
    BatchNorm, written out in `dtype` torch."""
    def lin(m, t):
        return t @ m.weight.to(dtype).T + (0 if m.bias is None else m.bias.to(dtype))

    def bn(m, t):
        return (t - m.running_mean.to(dtype)) / torch.sqrt(m.running_var.to(dtype) + m.eps) * m.weight.to(dtype) \
            + m.bias.to(dtype)
    p, x_q, x_k, x_v = (t.to(dtype) for t in (p, x_q, x_k, x_v))
    n, ns = idx.shape
    c = x_q.shape[1]
    have = (idx >= 0).to(dtype).unsqueeze(-1)
    j = idx.long().clamp(min=0)
    rel = (p[j] - p.unsqueeze(1)) * have
    lp, lw = layer.linear_p, layer.linear_w
    p_r = lin(lp[3], torch.relu(bn(lp[1], lin(lp[0], rel))))
    r = x_k[j] * have - x_q.unsqueeze(1) + p_r
    w = lin(lw[5], torch.relu(bn(lw[3], lin(lw[2], torch.relu(bn(lw[0], r))))))
    w = torch.softmax(w, dim=1)
    return (((x_v[j] * have + p_r).view(n, ns, 8, c // 8)) * w.unsqueeze(2)).sum(1).reshape(n, c)


# the model's five shapes, then shapes that take the kernel's other paths:
#   (24, 5)   3 channels per share group: the K padding of the second product
#   (88, 3)   31 points = 93 rows per workgroup (no multiple of the 4-row register tile), 11 channels per group, a last
#             W_w1 tile of 24 columns, and 264 register tiles: threads 0..7 hold a second one
#   (512, 32) the largest accepted shape: one point per workgroup, every thread holds two register tiles
@pytest.mark.parametrize("c,ns", [(32, 8), (64, 16), (128, 16), (256, 16), (512, 16), (24, 5), (88, 3), (512, 32)])
def test_vector_attention_vs_float64(dev, c, ns):
    """Scenes of 1, 7 and 701 points (709 rows: no multiple of a tile; the first gives a row of -1, the second too where
    ns > 7), random running statistics.  Yardstick E = the same composition in fp32 torch against float64: the kernel
    stays within 4 E
    (a different summation order) and within FP32_TOL of max(1, max|ref|); two runs bitwise equal."""
    import pointops
    from ptv3_hip import ops
    from pointcept.models.point_transformer.point_transformer_seg import PointTransformerLayer
    torch.manual_seed(c + ns)
    layer = PointTransformerLayer(c, c, 8, ns)
    for m in layer.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.normal_(1.0, 0.1)
            m.bias.data.normal_(0, 0.1)
    layer = layer.to(dev).eval()
    sizes = [1, 7, 701]
    n = sum(sizes)
    p = torch.rand(n, 3, device=dev)
    off = torch.tensor(np.cumsum(sizes), dtype=torch.int32, device=dev)
    idx, _ = pointops.knn_query(ns, p, off)
    assert (idx[:8] < 0).any() and (idx[8:] >= 0).all()
    x_q, x_k, x_v = (torch.randn(n, c, device=dev) for _ in range(3))
    lp, lw = layer.linear_p, layer.linear_w
    f = lambda t: t.detach().float().contiguous()   # noqa: E731
    args = (x_q, x_k, x_v, p, idx, f(lp[0].weight), *ops.fold_batchnorm(lp[1], lp[0].bias), f(lp[3].weight),
            f(lp[3].bias), *ops.fold_batchnorm(lw[0]), f(lw[2].weight), *ops.fold_batchnorm(lw[3], lw[2].bias),
            f(lw[5].weight), f(lw[5].bias))
    got = ops.vector_attention(*args)
    assert torch.equal(got, ops.vector_attention(*args))
    with torch.no_grad():
        ref = _attention_formula(layer, p, x_q, x_k, x_v, idx, torch.float64)
        e32 = (_attention_formula(layer, p, x_q, x_k, x_v, idx, torch.float32).double() - ref).abs().max().item()
    err = (got.double() - ref).abs().max().item()
    print(f"vector_attention c={c} ns={ns}: err {err:.3e}, fp32 torch E {e32:.3e}, max|ref| {ref.abs().max().item():.3f}")
    assert err <= 4 * e32, (err, e32)
    assert err <= FP32_TOL * max(1.0, ref.abs().max().item())


def test_vector_attention_refuses_unsupported_shapes(dev):
    from ptv3_hip import ops
    n = 10
    p = torch.rand(n, 3, device=dev)
    w = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731
    for c, ns, msg in ((12, 8, "c=12 unsupported"), (64, 33, "ns=33 unsupported")):
        cs = c // 8
        x = w(n, c)
        idx = torch.zeros(n, ns, dtype=torch.int32, device=dev)
        with pytest.raises(RuntimeError, match=msg):
            ops.vector_attention(x, x, x, p, idx, w(3, 3), w(3), w(3), w(c, 3), w(c), w(c), w(c), w(cs, c), w(cs), w(cs),
                                 w(cs, cs), w(cs))


# ------------------------------------------------------------------------------------------------
# the model against the reference's own outputs
# ------------------------------------------------------------------------------------------------
def _tiny(golden_dir, dev):
    from pointcept.models import build_model
    g = np.load(os.path.join(golden_dir, "keypoint_ptv1_tiny.npz"))
    model = build_model(dict(type="KeypointPTv1", **TINY_KW))
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    data = {k[3:]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("in_")}
    return g, model.to(dev), data


def _tapped_eval(model, data, monkeypatch=None):
    """Eval output and every stage's output features; with `monkeypatch` also the rows of every farthest point
    sampling, in call order."""
    taps = {}
    if monkeypatch is not None:
        from ptv3_hip import ops
        sample, taps["rows"] = ops.farthest_point_sampling, []

        def recording(*a, **k):
            taps["rows"].append(sample(*a, **k))
            return taps["rows"][-1]
        monkeypatch.setattr(ops, "farthest_point_sampling", recording)
    hooks = [getattr(model, f"enc{i + 1}").register_forward_hook(
        lambda m, inp, out, i=i: taps.__setitem__(i, out[1].detach())) for i in range(5)]
    with torch.no_grad():
        out = model.eval()(dict(data))
    for h in hooks:
        h.remove()
    if monkeypatch is not None:
        monkeypatch.undo()
    return out, taps


def test_keypoint_ptv1_eval_vs_reference_golden(dev, golden_dir, monkeypatch):
    """Every stage's sampled rows exactly, every stage's features, `pred` and `loss` within FP32_TOL of the reference's
    own.  After the single read of `offset` the eval forward only queues work (sample counts follow on the host; kNN
    and sampling are called without their offset read-back); the suite has no mechanism that asserts the absence of
    synchronisation, so that property is stated here and not asserted."""
    g, model, data = _tiny(golden_dir, dev)
    out, taps = _tapped_eval(model, data, monkeypatch)
    assert len(taps["rows"]) == 4
    for i, rows in enumerate(taps["rows"], start=2):
        assert np.array_equal(rows.cpu().numpy(), g[f"tap_idx{i}"]), i
    for i in range(5):
        ref = g[f"tap_x{i + 1}"]
        err = np.abs(taps[i].cpu().numpy()[::TAP_STRIDE[i]] - ref).max()
        assert err < FP32_TOL * max(1.0, np.abs(ref).max()), (i, err)
    assert tuple(out["pred"].shape) == (3, 6, 3) and out["pred"].dtype == torch.float32
    assert np.abs(out["pred"].cpu().numpy() - g["eval_pred"]).max() < FP32_TOL
    assert abs(out["loss"].item() - float(g["eval_loss"])) < FP32_TOL
    with torch.no_grad():
        out32 = model(dict(data, offset=data["offset"].int()))
    assert torch.equal(out32["pred"], out["pred"])


def test_keypoint_ptv1_train_step_vs_reference_golden(dev, golden_dir):
    """Loss, curves, every parameter gradient and the running statistics of one training step (the head's Dropout at
    p = 0), with the tolerances of test_keypoint_ptv3_train_step_vs_reference_golden."""
    g, model, data = _tiny(golden_dir, dev)
    model.train()
    model.reg_head[3].p = 0.0
    out = model(dict(data))
    out["loss"].backward()
    assert abs(out["loss"].item() - float(g["loss"])) < 1e-4
    assert abs(out["train/mean_dist"].item() - float(g["mean_dist"])) < 1e-4
    assert np.abs(np.array([out[f"train/kp{i}_dist"].item() for i in range(6)]) - g["kp_dist"]).max() < 1e-4
    grads = {k[5:]: torch.from_numpy(g[k].astype(np.float32) * g["gmax_" + k[5:]]) for k in g.files
             if k.startswith("grad_")}
    gmax = max(float(g[k]) for k in g.files if k.startswith("gmax_"))
    params = dict(model.named_parameters())
    assert set(params) == set(grads)
    # the bias of a Linear straight in front of a batch-statistic BatchNorm has an exact gradient of zero (the batch
    # mean removes any shift): both sides hold rounding noise, so it is held to noise level against its layer's weight
    zero = [n for n in params if n == "reg_head.0.bias" or n.endswith("linear_p.0.bias") or n.endswith("linear_w.2.bias")]
    assert len(zero) == 1 + 2 * 3
    for n in zero:
        weight = params[n[:-4] + "weight"].grad.abs().max().item()
        assert params[n].grad.abs().max().item() <= 1e-4 * weight, n
    for n, p in params.items():
        if n not in zero:
            err = (p.grad.float().cpu() - grads[n]).abs().max().item() / max(grads[n].abs().max().item(), 1e-3 * gmax)
            assert err < (2e-3 if n.startswith("reg_head.") else 1e-2), (n, err)
    for n, b in model.named_buffers():
        if "running" in n:
            ref = torch.from_numpy(g["buf_" + n])
            assert (b.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6) < 1e-4, n


def test_eval_equals_torch_composition(dev, golden_dir):
    """The fused eval forward against the training path's torch composition run in eval mode on the same weights:
    features of every stage and `pred` within FP32_TOL."""
    g, model, data = _tiny(golden_dir, dev)
    fused, taps = _tapped_eval(model, data)
    plain, ref_taps = _tapped_eval(model.set_fused(False), data)
    for i in range(5):
        scale = max(1.0, ref_taps[i].abs().max().item())
        assert (taps[i] - ref_taps[i]).abs().max().item() < FP32_TOL * scale, i
    assert (fused["pred"] - plain["pred"]).abs().max().item() < FP32_TOL
    assert abs(fused["loss"].item() - plain["loss"].item()) < FP32_TOL


def test_fork_config_eval_and_train_step(dev):
    """KeypointPTv1-50 from configs/my_dataset/keypoint_ptv1.py's model dict on two scenes of about 4000 points."""
    import ptv3_scenes as S
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_PTV1_CFG
    torch.manual_seed(7)
    model = build_model(KEYPOINT_PTV1_CFG).to(dev)
    data = {k: v.to(dev) for k, v in S.make_batch([4100, 3900], in_channels=4, extent=64, seed=3).items()}
    data["target"] = torch.randn(12, 3, device=dev) * 0.5
    with torch.no_grad():
        pred = model.eval()(dict(data))["pred"]
    assert tuple(pred.shape) == (2, 6, 3) and torch.isfinite(pred).all()
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=0.05)
    out = model.train()(dict(data))
    out["loss"].backward()
    opt.step()
    assert torch.isfinite(out["loss"]).item()
    assert all(p.grad is not None and torch.isfinite(p).all() for p in model.parameters())

