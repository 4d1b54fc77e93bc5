"""OctFormer on the GPU: ops.octree_build against tests/octree_ref.py (exact), ptv3_octree_attn_fwd and
ptv3_octree_dwconv against float64 under the 4x rule of test_hip_keypoint_strat.py (the kernel's error is at most four
times the error of the fp32 torch composition of the same formula), their integrity (canary rows, bitwise repeats,
refused arguments), and KeypointOctFormer / OffsetKeypointOctFormer against the reference's own outputs
(tests/golden/keypoint_octformer_tiny.npz: taps, pred, one training step) and on the fork configs."""
import os

import numpy as np
import pytest
import torch

import octree_ref
from make_golden_keypoint_octformer import seeded_state_dict, load_golden, TINY_KW, TAPS, TAP_STRIDE
from test_keypoint_octformer_cpu import FP32_TOL

pytestmark = pytest.mark.gpu
MARGIN4 = 4.0     # every tolerance is four times the fp32-vs-float64 error of the same formula
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# octree
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 700])
def test_octree_build_exact(dev, n):
    from ptv3_hip import ops
    rs = np.random.RandomState(n)
    depth, min_depth, scale = 6, 2, 2.5
    coord = np.clip(rs.randn(n, 3) * 0.8, -2.49, 2.49).astype(np.float32)
    if n > 1:
        coord[1] = coord[0]                                    # a leaf with two points
    feat = rs.randn(n, 4).astype(np.float32)
    ends = [n] if n == 1 else [n // 3, n]
    batch = torch.searchsorted(torch.tensor(ends), torch.arange(n), right=True)
    ref = octree_ref.Octree(depth, 2, batch_size=len(ends))
    ref.build_octree(octree_ref.Points(torch.from_numpy(coord) / scale, features=torch.from_numpy(feat),
                                       batch_id=batch.view(-1, 1), batch_size=len(ends)))
    ref.construct_all_neigh()
    args = (torch.from_numpy(coord).to(dev), torch.from_numpy(feat).to(dev), torch.tensor(ends, device=dev), scale,
            depth, min_depth)
    oct, again = ops.octree_build(*args), ops.octree_build(*args)
    assert oct.leaf.cpu().tolist() == ref.leaf.tolist()
    for d in range(min_depth, depth + 1):
        assert oct.nnum[d] == len(ref.keys[d])
        assert oct.keys[d].cpu().tolist() == ref.keys[d].tolist(), d
        assert oct.xyz[d].cpu().tolist() == torch.stack(ref.xyzb(d)[:3], 1).tolist(), d
        assert oct.batch[d].cpu().tolist() == (ref.keys[d] >> 48).tolist(), d
        assert oct.neighbors(d).cpu().tolist() == ref.neighs[d].tolist(), d
        assert torch.equal(oct.keys[d], again.keys[d]) and torch.equal(oct.neighbors(d), again.neighbors(d))
        if d > min_depth:
            assert oct.parent[d].cpu().tolist() == ref.parent[d].tolist(), d
        if d < depth:
            assert oct.children[d].cpu().tolist() == ref.children[d].tolist(), d
            pairs = {tuple(r) for r in ref.deconv_pairs(d).tolist()}
            tab = oct.deconv_table(d).cpu()
            rows, taps = torch.nonzero(tab >= 0, as_tuple=True)
            assert {(int(tab[r, t]), int(t), int(r)) for r, t in zip(rows, taps)} == pairs, d
    want = ref.features[depth]
    counts = torch.bincount(ref.leaf).float().unsqueeze(1)
    # a mean of m values: m - 1 additions and one division, each within half an ulp of the running magnitude
    tol = (counts + 1) * ULP * torch.zeros_like(want).index_add_(0, ref.leaf, torch.from_numpy(feat).abs()) / counts
    assert ((oct.features.cpu() - want).abs() <= tol).all()
    assert torch.equal(oct.features, again.features) and torch.equal(oct.leaf, again.leaf)


def test_octree_build_refuses_a_point_outside_the_domain(dev):
    from ptv3_hip import ops
    coord = torch.zeros((5, 3), device=dev)
    feat = torch.zeros((5, 4), device=dev)
    ends = torch.tensor([5], device=dev)
    ops.octree_build(coord, feat, ends, 2.5, 6, 2)
    with pytest.raises(ValueError):
        ops.octree_build(coord, feat, torch.tensor([2, 4], device=dev), 2.5, 6, 2)     # offsets that end early
    for bad in (2.5, -2.5001, float("nan")):
        c = coord.clone()
        c[3, 1] = bad
        with pytest.raises(ValueError):
            ops.octree_build(c, feat, ends, 2.5, 6, 2)


# ---------------------------------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------------------------------
def _attn_ref64(qkv, xyz, batch, table, heads, k, d, bnd, scale, pad_row):
    """The float64 formula, by row indices: token j of patch p of group g is row g k d + j d + p; padding rows carry
    pad_row, scene id -1 and coordinates 0; -1e3 where the scene ids differ."""
    n_t, c = qkv.shape[0], qkv.shape[1] // 3
    groups = -(-n_t // (k * d))
    rows = (torch.arange(groups).view(-1, 1, 1) * k * d + torch.arange(d).view(1, -1, 1)
            + torch.arange(k).view(1, 1, -1) * d).reshape(-1, k)                     # (patches, k)
    real = rows < n_t
    safe = rows.clamp(max=n_t - 1)
    x = torch.where(real.unsqueeze(-1), qkv.double()[safe], pad_row.double().view(1, 1, -1))
    pos = torch.where(real.unsqueeze(-1), xyz.long()[safe], torch.zeros(1, dtype=torch.int64))
    scene = torch.where(real, batch.long()[safe], torch.full((1,), -1))
    hd = c // heads
    q, key, v = (x[..., i * c:(i + 1) * c].reshape(-1, k, heads, hd).transpose(1, 2) for i in range(3))
    logit = scale * torch.einsum("phid,phjd->phij", q, key)
    rel = (pos.unsqueeze(2) - pos.unsqueeze(1)).clamp(-bnd, bnd) + bnd                # (patches, k, k, 3)
    t64 = table.double()
    for axis in range(3):
        logit = logit + t64[axis * (2 * bnd + 1) + rel[..., axis]].permute(0, 3, 1, 2)
    logit = logit + torch.where(scene.unsqueeze(2) != scene.unsqueeze(1), -1e3, 0.0).unsqueeze(1)
    o = torch.einsum("phij,phjd->pihd", torch.softmax(logit, -1), v).reshape(-1, k, c)
    out = torch.zeros((n_t, c), dtype=torch.float64)
    out[rows[real]] = o[real]
    return out


def _scene_ids(n_t, k, d):
    """scene boundaries inside the first patch, inside a dilated patch of the second group, exactly on a group boundary,
    and a scene of one node right behind it"""
    cuts = sorted({c for c in (k // 2, k * d, k * d + 1, k * d + k + 1, 2 * k * d + 3) if 0 < c < n_t})
    return torch.searchsorted(torch.tensor(cuts, dtype=torch.int64), torch.arange(n_t), right=True).int()


ATTN_CASES = [(k, d, hd, h) for k in (26, 8) for d in (1, 2, 4) for hd in (16, 32) for h in (1, 6)]


def _attn_case(dev, k, d, hd, heads, q_scale):
    from ptv3_hip import ops
    c, bnd, scale = hd * heads, 41, hd ** -0.5
    assert ops.octree_attn_capable(c, heads, k, d)
    for n_t in (1, k * d - 1, k * d, k * d + 1, 3 * k * d + 5):
        g = torch.Generator().manual_seed(1000 * k + 100 * d + hd + heads + n_t)
        qkv = torch.randn(n_t, 3 * c, generator=g)
        qkv[:, :c] *= q_scale
        xyz = torch.randint(0, 121, (n_t, 3), generator=g, dtype=torch.int32)
        batch = _scene_ids(n_t, k, d)
        table = 0.5 * torch.randn(3 * (2 * bnd + 1), heads, generator=g)
        pad_row = torch.randn(3 * c, generator=g)
        ref = _attn_ref64(qkv, xyz, batch, table, heads, k, d, bnd, scale, pad_row)
        on = [t.to(dev) for t in (qkv, xyz, batch, table)]
        comp = ops.octree_attention_torch(*on, heads, k, d, bnd, scale, pad_row.to(dev))
        got = ops.octree_attention(*on, heads, k, d, bnd, scale, pad_row.to(dev), fused=True)
        e32 = (comp.double().cpu() - ref).abs().max().item()
        err = (got.double().cpu() - ref).abs().max().item()
        print(f"octree attn K {k} D {d} hd {hd} H {heads} n_t {n_t} q x{q_scale}: err {err:.3e}, fp32 composition E "
              f"{e32:.3e}, max|ref| {ref.abs().max().item():.3f}")
        assert torch.isfinite(got).all()
        assert err <= MARGIN4 * e32, (n_t, err, e32)


# every shape at ordinary logits; growing logits (q x 30) at the fork's head shapes and one small one
@pytest.mark.parametrize("k, d, hd, heads, q_scale",
                         [c + (1.0,) for c in ATTN_CASES] + [(26, 4, 16, 6, 30.0), (26, 1, 16, 6, 30.0),
                                                             (26, 4, 32, 6, 30.0), (8, 2, 16, 1, 30.0)])
def test_octree_attention_vs_float64(dev, k, d, hd, heads, q_scale):
    _attn_case(dev, k, d, hd, heads, q_scale)


def test_octree_attention_integrity(dev):
    """a canary row behind the output, bitwise repeats, and every refused argument with nothing launched"""
    from ptv3_hip import ops
    from ptv3_hip.lib import lib
    k, d, heads, hd, bnd, n_t = 26, 4, 6, 16, 41, 26 * 4 * 2 + 9
    c = heads * hd
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(n_t, 3 * c, generator=g).to(dev)
    xyz = torch.randint(0, 121, (n_t, 3), generator=g, dtype=torch.int32).to(dev)
    batch = _scene_ids(n_t, k, d).to(dev)
    table = torch.randn(3 * (2 * bnd + 1), heads, generator=g).to(dev)

    def run(out, n=n_t, c_=c, heads_=heads, k_=k, d_=d, bnd_=bnd):
        return lib.ptv3_octree_attn_fwd(qkv.data_ptr(), xyz.data_ptr(), batch.data_ptr(), table.data_ptr(),
                                        out.data_ptr(), n, c_, heads_, k_, d_, bnd_, 0.25, ops._stream())
    outs = []
    for _ in range(2):
        out = torch.full((n_t + 1, c), -7.0, device=dev)
        assert run(out) == 0
        assert (out[n_t] == -7.0).all() and (out[:n_t] != -7.0).all()
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    out = torch.full((n_t + 1, c), -7.0, device=dev)
    UNSUPPORTED, ARG = 3, 1
    assert run(out, c_=8 * heads) == UNSUPPORTED            # head dimension 8
    assert run(out, c_=64 * heads) == UNSUPPORTED           # head dimension 64
    assert run(out, k_=33) == UNSUPPORTED                   # a patch the wave does not hold
    assert run(out, bnd_=128) == UNSUPPORTED                # a table beyond the LDS image
    assert run(out, heads_=5) == ARG                        # channels do not divide
    assert run(out, n=0) == ARG
    assert run(out, d_=0) == ARG
    assert run(out, bnd_=-1) == ARG
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert not ops.octree_attn_capable(8 * heads, heads, k, d) and not ops.octree_attn_capable(c, heads, 33, d)
    # ops falls back to the composition where the kernel refuses
    wide = torch.randn(n_t, 3 * 64, generator=g).to(dev)
    t1 = torch.randn(3 * (2 * bnd + 1), 1, generator=g).to(dev)
    a = ops.octree_attention(wide, xyz, batch, t1, 1, k, d, bnd, 0.125, fused=True)
    b = ops.octree_attention_torch(wide, xyz, batch, t1, 1, k, d, bnd, 0.125)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# depthwise conv
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [16, 96, 384])
def test_octree_dwconv_vs_float64(dev, c):
    from ptv3_hip import ops
    for n in (1, 63, 64, 65):
        g = torch.Generator().manual_seed(c + n)
        x = torch.randn(n, c, generator=g)
        w = torch.randn(27, 1, c, generator=g) / 5
        scale, shift = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
        nbr = torch.randint(0, n, (n, 27), generator=g, dtype=torch.int32)
        nbr[torch.rand(n, 27, generator=g) < 0.3] = -1
        nbr[0] = -1                                            # a row with its own tap only
        nbr[:, 13] = torch.arange(n, dtype=torch.int32)
        if n > 1:
            nbr[n - 1] = torch.randint(0, n, (27,), generator=g, dtype=torch.int32)   # a row with all 27
        xp = torch.cat([x.double(), torch.zeros(1, c, dtype=torch.float64)])
        idx = torch.where(nbr >= 0, nbr, n).long()
        ref = x.double() + (xp[idx] * w.double()[:, 0]).sum(1) * scale.double() + shift.double()
        on = [t.to(dev) for t in (x, w, nbr, scale, shift)]
        got = ops.octree_dwconv(*on)
        comp = ops.octree_dwconv_torch(on[0], on[1][:, 0], *on[2:])
        e32 = (comp.double().cpu() - ref).abs().max().item()
        err = (got.double().cpu() - ref).abs().max().item()
        print(f"octree dwconv C {c} n {n}: err {err:.3e}, fp32 composition E {e32:.3e}")
        assert err <= MARGIN4 * e32, (n, err, e32)
        assert torch.equal(got, ops.octree_dwconv(*on))
    with pytest.raises(RuntimeError):
        ops.octree_dwconv(torch.zeros(4, 6, device=dev), torch.zeros(27, 6, device=dev),
                          torch.zeros(4, 27, dtype=torch.int32, device=dev), torch.ones(6, device=dev),
                          torch.zeros(6, device=dev))


# ---------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------
_GOLDEN = {}


def _tiny(golden_dir, dev, kind="KeypointOctFormer"):
    from pointcept.models import build_model
    if not _GOLDEN:
        _GOLDEN.update(load_golden(golden_dir))
    g = _GOLDEN
    model = build_model(dict(type=kind, **TINY_KW))
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    data = {k[3:]: torch.from_numpy(v).to(dev) for k, v in g.items() if k.startswith("in_")}
    return g, model.to(dev), data


def _tol(g, name, ref):
    """4x the reference's own fp32-vs-float64 gap of the quantity, floored at one fp32 ulp of its scale (the taps'
    errors and gaps are already relative to max(1, max|ref|))"""
    return max(MARGIN4 * float(g["gap_" + name]), ULP * (1.0 if name in TAPS else max(1.0, float(np.abs(ref).max()))))


@pytest.mark.parametrize("fused", [True, False])
def test_keypoint_octformer_eval_vs_reference_golden(dev, golden_dir, fused):
    g, model, data = _tiny(golden_dir, dev)
    model.set_fused(fused)
    taps = {}
    with torch.no_grad():
        out = model.eval()(dict(data), taps=taps)
    depth = TINY_KW["octree_depth"]
    oct = model.points2octree(data["coord"], data["feat"], data["offset"])
    for d in range(depth - TINY_KW["stem_down"] - 3, depth + 1):
        assert oct.nnum[d] == int(g[f"nnum{d}"])
        if f"keys{d}" in g:
            assert oct.keys[d].cpu().tolist() == g[f"keys{d}"].tolist()
    worst = 0.0
    for name in TAPS:
        ref = g["tap_" + name]
        err = np.abs(taps[name].cpu().numpy()[::TAP_STRIDE[name]] - ref).max() / max(1.0, np.abs(ref).max())
        print(f"fused={fused} {name}: err {err:.3e}, tolerance {_tol(g, name, ref):.3e}")
        worst = max(worst, err / _tol(g, name, ref))
    err = np.abs(out["pred"].cpu().numpy() - g["eval_pred"]).max()
    print(f"fused={fused} pred: err {err:.3e}, tolerance {_tol(g, 'pred', g['eval_pred']):.3e}")
    assert tuple(out["pred"].shape) == (3, 6, 3) and out["pred"].dtype == torch.float32
    assert err <= _tol(g, "pred", g["eval_pred"])
    assert worst <= 1.0, worst


def test_fused_eval_never_composes(dev, golden_dir, monkeypatch):
    """with autograd left on (the parameters ask for gradients) the fused eval forward still runs the kernels: the
    compositions are made to raise"""
    from ptv3_hip import ops
    g, model, data = _tiny(golden_dir, dev)

    def composed(*a, **k):
        raise AssertionError("the fused eval forward called a torch composition")
    monkeypatch.setattr(ops, "octree_attention_torch", composed)
    monkeypatch.setattr(ops, "octree_dwconv_torch", composed)
    out = model.eval()(dict(data))
    assert np.abs(out["pred"].detach().cpu().numpy() - g["eval_pred"]).max() <= _tol(g, "pred", g["eval_pred"])


@pytest.mark.parametrize("fused", [True, False])
def test_offset_keypoint_octformer_eval_vs_reference_golden(dev, golden_dir, fused):
    g, model, data = _tiny(golden_dir, dev, "OffsetKeypointOctFormer")
    model.set_fused(fused)
    data["target"] = torch.from_numpy(g["offset_target"]).to(dev)
    with torch.no_grad():
        out = model.eval()(dict(data))
    err = np.abs(out["pred"].cpu().numpy()[::16] - g["offset_pred"]).max()
    print(f"fused={fused} offset pred: err {err:.3e}, tolerance {_tol(g, 'offset_pred', g['offset_pred']):.3e}")
    assert err <= _tol(g, "offset_pred", g["offset_pred"])
    assert abs(out["loss"].item() - float(g["offset_loss"])) <= max(MARGIN4 * float(g["gap_offset_loss"]), ULP)


def test_keypoint_octformer_train_step_vs_reference_golden(dev, golden_dir):
    """Loss, curves, every parameter gradient and the running statistics of one training step (the head's Dropout at
    p = 0), with check_step's tolerances (make_golden_keypoint_oacnns.py)."""
    g, model, data = _tiny(golden_dir, dev)
    model.train()
    model.reg_head[3].p = 0.0
    out = model(dict(data))
    out["loss"].backward()
    assert abs(out["loss"].item() - float(g["loss"])) < 1e-4
    assert abs(out["train/mean_dist"].item() - float(g["mean_dist"])) < 1e-4
    assert np.abs(np.array([out[f"train/kp{i}_dist"].item() for i in range(6)]) - g["kp_dist"]).max() < 1e-4
    grads = {k[5:]: torch.from_numpy(g[k].astype(np.float32) * g["gmax_" + k[5:]]) for k in g if k.startswith("grad_")}
    gmax = max(float(g[k]) for k in g if k.startswith("gmax_"))
    params = dict(model.named_parameters())
    assert set(params) == set(grads)
    zero = "reg_head.0.bias"    # in front of a batch-statistic BatchNorm: exact gradient zero, noise on both sides
    assert params[zero].grad.abs().max().item() <= 1e-4 * params["reg_head.0.weight"].grad.abs().max().item()
    worst = ("", 0.0)
    for n, p in params.items():
        if n != zero:
            assert p.grad is not None and p.grad.abs().max().item() > 0, n
            err = (p.grad.float().cpu() - grads[n]).abs().max().item() / max(grads[n].abs().max().item(), 1e-3 * gmax)
            worst = max(worst, (n, err), key=lambda q: q[1])
            assert err < (2e-3 if n.startswith("reg_head.") else 1e-2), (n, err)
    print("worst gradient error", worst)
    for n, b in model.named_buffers():
        if "running" in n:
            ref = torch.from_numpy(g["buf_" + n])
            assert (b.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6) < 1e-4, n


@pytest.mark.parametrize("cfg_name, listing", [
    ("KEYPOINT_OCTFORMER_CFG", "state_dict_keypoint_octformer_fork.txt"),
    ("OFFSET_KEYPOINT_OCTFORMER_CFG", "state_dict_offset_keypoint_octformer_fork.txt")])
def test_fork_config_forward(dev, golden_dir, cfg_name, listing):
    """the fork config on 2 x 2000 surface points, fused against composed, and a strict load of the reference's keys"""
    from pointcept.models import build_model
    from ptv3_hip import configs
    model = build_model(dict(getattr(configs, cfg_name)))
    shapes = {}
    for line in open(os.path.join(golden_dir, listing)):
        key, rest = line.split(" ", 1)
        shapes[key] = eval(rest[:rest.rindex(")") + 1])
    sd = {k: (torch.zeros(s, dtype=torch.int64) if k.endswith("num_batches_tracked") else
              model.state_dict()[k].new_empty(s).copy_(model.state_dict()[k])) for k, s in shapes.items()}
    model.load_state_dict(sd, strict=True)
    rs = np.random.RandomState(2)
    xy = rs.rand(4000, 2) * 1.2 - 0.6
    coord = np.concatenate([xy, 0.2 * np.sin(3 * xy[:, :1]) + 0.01 * rs.randn(4000, 1)], 1).astype(np.float32)
    data = {"coord": torch.from_numpy(coord).to(dev), "feat": torch.from_numpy(rs.randn(4000, 4).astype(np.float32)).to(dev),
            "offset": torch.tensor([2000, 4000], device=dev)}
    model = model.to(dev).eval()
    with torch.no_grad():
        fused = model(dict(data))["pred"]
        plain = model.set_fused(False)(dict(data))["pred"]
    want = (2, 6, 3) if cfg_name == "KEYPOINT_OCTFORMER_CFG" else (4000, 6, 4)
    assert tuple(fused.shape) == want and torch.isfinite(fused).all()
    err = (fused - plain).abs().max().item() / max(1.0, plain.abs().max().item())
    print(f"{cfg_name}: fused against composed {err:.3e}")
    assert err < FP32_TOL * 10     # fp32 sums in another order through 24 blocks, where the 8-block tiny model has FP32_TOL
