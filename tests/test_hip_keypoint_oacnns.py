"""KeypointOACNNs on the GPU: the kernel-2 / stride-2 plan against numpy (exact), the strided convs and the cluster
kernels against float64 torch statements written here, the model against the reference's own outputs
(tests/golden/keypoint_oacnns_tiny.npz: eval taps, coarse sites, one training step), the fused eval forward against the
torch composition, and the fork config end to end.

The accuracy rule of the kernel tests: the kernel's largest error against the float64 statement
is at most 4x the largest error of the same statement evaluated by torch in fp32, both measured in the test.  The bound
never falls under one fp32 rounding of the result's magnitude (2^-23 max|ref|), which no fp32 result can beat."""
import os

import numpy as np
import pytest
import torch

from make_golden_keypoint_oacnns import seeded_state_dict, zero_bias, TINY_KW, TAPS, TAP_STRIDE, MIXED_BLOCK  # noqa: E402

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _within_4x(got, fp32, ref64, what):
    ref = ref64.double().cpu()
    err = (got.double().cpu() - ref).abs().max().item()
    base = (fp32.double().cpu() - ref).abs().max().item()
    floor = 2.0 ** -23 * ref.abs().max().item()
    print(f"{what}: kernel error {err:.3e}, fp32 torch error {base:.3e}")
    assert err <= max(4 * base, floor), (what, err, base)


# ------------------------------------------------------------------------------------------------
# plan
# ------------------------------------------------------------------------------------------------
_PLAN = {}


def _plan_case(dev):
    """2 scenes of 700 and 300 sites, minimum x = 2, at least one odd extent; numpy plan + the device plan (once)."""
    if not _PLAN:
        import ptv3_scenes as S
        from ptv3_hip import ops
        b = S.make_batch([700, 300], in_channels=4, extent=41, seed=9)
        grid = b["grid_coord"].numpy().astype(np.int64)
        grid[:, 0] += 2
        batch = np.repeat([0, 1], [700, 300])
        sites = np.concatenate([batch[:, None], grid], axis=1)
        shape = (grid.max(0) + 1).tolist()
        assert any(s % 2 for s in shape) and grid[:, 0].min() == 2
        out_shape = [(s - 2) // 2 + 1 for s in shape]
        par = np.concatenate([sites[:, :1], sites[:, 1:] >> 1], axis=1)
        ok = np.all(par[:, 1:] < np.asarray(out_shape), axis=1)
        coarse, inv = np.unique(par[ok], axis=0, return_inverse=True)
        parent = np.full(1000, -1, dtype=np.int64)
        parent[ok] = inv.reshape(-1)
        tap = (grid[:, 0] & 1) * 4 + (grid[:, 1] & 1) * 2 + (grid[:, 2] & 1)
        assert (~ok).sum() >= 1, "the case must hold sites without a parent"
        idx = torch.from_numpy(sites).int().to(dev)
        _PLAN.update(sites=sites, shape=shape, out_shape=out_shape, parent=parent, tap=tap, coarse=coarse, ok=ok,
                     plan=ops.down2_plan(idx, shape, 2))
    return _PLAN


def test_down2_plan_exact(dev):
    c = _plan_case(dev)
    plan, parent, tap, ok = c["plan"], c["parent"], c["tap"], c["ok"]
    assert plan.n == 1000 and plan.m_out == len(c["coarse"]) and plan.out_shape == c["out_shape"]
    assert np.array_equal(plan.parent.cpu().numpy(), parent)            # -1: reported as without a parent
    assert np.array_equal(plan.tap.cpu().numpy(), tap)
    assert np.array_equal(plan.coarse.cpu().numpy(), c["coarse"])
    assert plan.dropped == int((~ok).sum())
    child = np.full((plan.m_out, 8), -1, dtype=np.int64)
    child[parent[ok], tap[ok]] = np.nonzero(ok)[0]
    assert np.array_equal(plan.child.cpu().numpy(), child)
    key = np.where(ok, tap, 8)
    rows = plan.up_rows.cpu().numpy()
    assert np.array_equal(np.sort(rows), np.arange(1000)) and np.all(np.diff(key[rows]) >= 0)
    assert plan.tap_start == [0] + np.cumsum(np.bincount(key, minlength=9)).tolist()


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("cin,cout", [(4, 16), (16, 32), (64, 64), (256, 256)])
def test_down2_and_up2_conv(dev, cin, cout, epilogue):
    from ptv3_hip import ops
    c = _plan_case(dev)
    plan = c["plan"]
    gen = torch.Generator().manual_seed(cin * 1000 + cout)
    x = torch.randn(1000, cin, generator=gen)
    y = torch.randn(plan.m_out, cin, generator=gen)
    w = torch.randn(cout, 2, 2, 2, cin, generator=gen) / (8 * cin) ** 0.5
    scale, shift = torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.3
    parent, tap = torch.from_numpy(c["parent"]), torch.from_numpy(c["tap"])

    def epi(v, s, t):
        return torch.relu(v * s + t) if epilogue else v

    def down(x, w, s, t):
        out = x.new_zeros(plan.m_out, cout)
        wt = w.reshape(cout, 8, cin)
        for k in range(8):
            rows = torch.nonzero((parent >= 0) & (tap == k)).flatten().to(x.device)
            out = out.index_add(0, parent.to(x.device)[rows], x[rows] @ wt[:, k].T)
        return epi(out, s, t)

    def up(y, w, s, t):
        out = y.new_zeros(1000, cout)
        wt = w.reshape(cout, 8, cin)
        for k in range(8):
            rows = torch.nonzero((parent >= 0) & (tap == k)).flatten().to(y.device)
            out[rows] = y[parent.to(y.device)[rows]] @ wt[:, k].T
        return epi(out, s, t)

    kw = dict(bn_scale=scale.to(dev), bn_shift=shift.to(dev), act=ops.ACT_RELU) if epilogue else {}
    got = ops.down2_conv(x.to(dev), w.to(dev), plan, **kw)
    _within_4x(got, down(x.to(dev), w.to(dev), scale.to(dev), shift.to(dev)),
               down(x.double(), w.double(), scale.double(), shift.double()), f"down {cin}->{cout}")
    got = ops.up2_conv(y.to(dev), w.to(dev), plan, **kw)
    _within_4x(got, up(y.to(dev), w.to(dev), scale.to(dev), shift.to(dev)),
               up(y.double(), w.double(), scale.double(), shift.double()), f"up {cin}->{cout}")
    lost = torch.from_numpy(~c["ok"])
    if epilogue:
        assert torch.equal(got.cpu()[lost], torch.relu(shift).expand(int(lost.sum()), cout))
    else:
        assert lost.any() and (got.cpu()[lost] == 0).all()


# ------------------------------------------------------------------------------------------------
# cluster kernels
# ------------------------------------------------------------------------------------------------
_CLUSTER = {}
LOW = (5, 7, 3)     # the batch minimum: no multiple of 2, 3 or 64


def _cluster_case(dev, g):
    """1500 rows: scene 0 = 1300 sites of a 12^3 box at the batch minimum (one cluster at g = 64, 1-8 rows per cluster at
    g = 2), scene 1 = 200 sites 64 cells apart along x (single-row clusters at every g)."""
    if "idx" not in _CLUSTER:
        rs = np.random.RandomState(3)
        cells = rs.permutation(12 ** 3)[:1300]
        box = np.stack([cells // 144, cells // 12 % 12, cells % 12], axis=1) + np.asarray(LOW)
        line = np.stack([LOW[0] + 3 + 64 * np.arange(200), np.full(200, LOW[1] + 1), np.full(200, LOW[2] + 9)], axis=1)
        sites = np.concatenate([np.repeat([0, 1], [1300, 200])[:, None], np.concatenate([box, line])], axis=1)
        sites = sites[rs.permutation(1500)]
        assert tuple(sites[:, 1:].min(0)) == LOW
        _CLUSTER["sites"] = sites
        _CLUSTER["idx"] = torch.from_numpy(sites).int().to(dev)
    if g not in _CLUSTER:
        from ptv3_hip import ops
        sites = _CLUSTER["sites"]
        cell = np.concatenate([sites[:, :1], (sites[:, 1:] - np.asarray(LOW)) // g], axis=1)
        _, ids, sizes = np.unique(cell, axis=0, return_inverse=True, return_counts=True)
        low = _CLUSTER["idx"][:, 1:].amin(0).contiguous()
        _CLUSTER[g] = (ops.cluster_plan(_CLUSTER["idx"], low, g), torch.from_numpy(ids.reshape(-1)), sizes)
    return _CLUSTER[g]


def test_cluster_plan_partitions(dev):
    for g, biggest in ((2, (8, 8)), (3, (9, 27)), (64, (1300, 1300))):
        plan, ids, sizes = _cluster_case(dev, g)
        assert plan.count() == len(sizes) and np.array_equal(plan.cluster.cpu().numpy(), ids.numpy()), g
        assert sizes.min() == 1 and biggest[0] <= sizes.max() <= biggest[1], (g, sizes.max())
        seg = plan.seg_start[:plan.count() + 1].cpu().numpy()
        assert np.array_equal(np.diff(seg), sizes)
        assert np.array_equal(ids.numpy()[plan.order.cpu().numpy()], np.repeat(np.arange(len(sizes)), sizes))


def _segsum(v, ids, k):
    return v.new_zeros(k, v.shape[1]).index_add(0, ids.to(v.device), v)


@pytest.mark.parametrize("g", [2, 64])
@pytest.mark.parametrize("c", [16, 64, 256])
def test_cluster_center_and_softmax_sum(dev, c, g):
    from ptv3_hip import ops
    plan, ids, sizes = _cluster_case(dev, g)
    k = len(sizes)
    gen = torch.Generator().manual_seed(c + g)
    wide = torch.randn(1500, 3 * c, generator=gen)       # the kernels read column slices of a wider matrix
    x, p, v = wide[:, :c], wide[:, c:2 * c] * 2.0, wide[:, 2 * c:]
    count = torch.from_numpy(sizes)

    def center(x):
        mean = _segsum(x, ids, k) / count.to(x.device, x.dtype).unsqueeze(1)
        return x - mean[ids.to(x.device)]

    def ssum(p, v):
        e = torch.exp(p - p.max())
        s = _segsum(e, ids, k)
        return _segsum(v * (e / (s[ids.to(p.device)] + 1e-6)), ids, k)

    wd = wide.to(dev)
    xd, pd, vd = wd[:, :c], (wd[:, c:2 * c] * 2.0).contiguous(), wd[:, 2 * c:]
    _within_4x(ops.cluster_center(xd, plan), center(xd), center(x.double()), f"center C={c} g={g}")
    m_dev = torch.amax(pd)
    got = ops.cluster_softmax_sum(pd, vd, m_dev, plan)
    _within_4x(got[:k], ssum(pd, vd), ssum(p.double(), v.double()), f"softmax_sum C={c} g={g}")
    again = ops.cluster_softmax_sum(pd, vd, m_dev, plan)
    assert torch.equal(got[:k], again[:k])               # fixed order: bitwise reproducible
    assert torch.equal(ops.cluster_center(xd, plan), ops.cluster_center(xd, plan))


def test_softmax_sum_cluster_far_below_the_maximum_is_exactly_zero(dev):
    """exp(-120) is zero in fp32: such a cluster's S and weighted sum vanish and 0 / (0 + 1e-6) is an exact zero."""
    from ptv3_hip import ops
    for g in (2, 64):
        plan, ids, sizes = _cluster_case(dev, g)
        gen = torch.Generator().manual_seed(g)
        p, v = torch.randn(1500, 32, generator=gen), torch.randn(1500, 32, generator=gen)
        far = [int(np.argmax(sizes)), int(np.argmin(sizes))]          # the largest cluster and a single-row one
        rows = (ids == far[0]) | (ids == far[1])
        p[rows] = p[~rows].max() - 120.0
        got = ops.cluster_softmax_sum(p.to(dev), v.to(dev), torch.amax(p.to(dev)), plan)[:len(sizes)].cpu()
        assert torch.isfinite(got).all() and (got[far] == 0).all()
        rest = torch.ones(len(sizes), dtype=torch.bool)
        rest[far] = False
        assert (got[rest].abs().amax(1) > 0).all()


@pytest.mark.parametrize("grids", [(2, 3, 64), (2, 3, 64, 64)])
@pytest.mark.parametrize("c", [16, 64, 256])
def test_cluster_mix(dev, c, grids):
    from ptv3_hip import ops
    cases = [_cluster_case(dev, g) for g in grids]
    plans = [q[0] for q in cases]
    assert len(grids) == 3 or plans[2] is plans[3]        # equal grid sizes share one plan
    gen = torch.Generator().manual_seed(c + len(grids))
    logits = torch.randn(1500, len(grids), generator=gen) * 2.0
    aggs = [torch.randn(1500, c, generator=gen) for _ in grids]      # rows past a plan's cluster count are never read
    head = torch.randn(1500, c, generator=gen)

    def mix(logits, aggs):
        adp = torch.softmax(logits, dim=1)
        return sum(adp[:, l:l + 1] * aggs[l][cases[l][1].to(logits.device)] for l in range(len(grids)))

    ld, ad = logits.to(dev), [a.to(dev) for a in aggs]
    ref = mix(logits.double(), [a.double() for a in aggs])
    _within_4x(ops.cluster_mix(ld, ad, plans), mix(ld, ad), ref, f"mix C={c} L={len(grids)}")
    both = ops.cluster_mix(ld, ad, plans, head=head.to(dev))
    assert tuple(both.shape) == (1500, 2 * c) and torch.equal(both[:, :c].cpu(), head)
    assert torch.equal(both[:, c:], ops.cluster_mix(ld, ad, plans))


# ------------------------------------------------------------------------------------------------
# the model against the reference's own outputs
# ------------------------------------------------------------------------------------------------
def _tiny(golden_dir, dev):
    from pointcept.models import build_model
    g = np.load(os.path.join(golden_dir, "keypoint_oacnns_tiny.npz"))
    model = build_model(dict(type="KeypointOACNNs", **TINY_KW))
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    data = {k[3:]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("in_")}
    return g, model.to(dev), data


def _tapped_eval(model, data):
    """Eval output, the nine feature taps in the golden's order (SparseConvTensors) and `mixed` of MIXED_BLOCK."""
    block = dict(model.named_modules())[MIXED_BLOCK]
    block.tap, taps = {}, []
    with torch.no_grad():
        out = model.eval()(dict(data), taps=taps)
    mixed, block.tap = block.tap["mixed"].clone(), None
    return out, dict(zip(TAPS, taps)), mixed


def _stored(name, feat, n_in):
    return feat[::TAP_STRIDE] if feat.shape[0] == n_in else feat


def test_eval_vs_reference_golden(dev, golden_dir):
    """Coarse site lists exactly; the nine taps, `mixed`, `pred` and the loss within FP32_TOL of the tap's scale."""
    g, model, data = _tiny(golden_dir, dev)
    out, taps, mixed = _tapped_eval(model, data)
    n_in = data["feat"].shape[0]
    for i in range(4):
        assert np.array_equal(taps[f"enc.{i}"].indices.cpu().numpy(), g[f"sites{i + 1}"]), i
    for name in TAPS:
        ref = g["tap_" + name]
        err = np.abs(_stored(name, taps[name].features, n_in).cpu().numpy() - ref).max()
        print(f"tap {name}: error {err:.3e}, scale {np.abs(ref).max():.3e}")
        assert err < FP32_TOL * np.abs(ref).max(), (name, err)
    ref = g["tap_mixed"]
    assert np.abs(mixed.cpu().numpy() - ref).max() < FP32_TOL * np.abs(ref).max()
    assert tuple(out["pred"].shape) == (2, 6, 3) and out["pred"].dtype == torch.float32
    assert np.abs(out["pred"].cpu().numpy() - g["eval_pred"]).max() < FP32_TOL
    assert abs(out["loss"].item() - float(g["eval_loss"])) < FP32_TOL


def test_eval_reads_the_device_five_times(dev, golden_dir, monkeypatch):
    """One read at entry (spatial shape and offsets) and one per stage (the plan's counters).  Counted: every
    `.tolist()`, `.item()`, `.cpu()` and `.numpy()` on a GPU tensor during the fused eval forward (the ways this package
    reads the device); implicit synchronisation inside torch ops is not visible to this count."""
    g, model, data = _tiny(golden_dir, dev)
    model.eval()
    with torch.no_grad():
        model(dict(data))            # parameter caches filled
    reads = []
    for name in ("tolist", "item", "cpu", "numpy"):
        inner = getattr(torch.Tensor, name)

        def counting(self, *a, _inner=inner, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _inner(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counting)
    with torch.no_grad():
        out = model(dict(data))
    monkeypatch.undo()
    assert reads == ["tolist"] * 5, reads
    assert np.abs(out["pred"].cpu().numpy() - g["eval_pred"]).max() < FP32_TOL


def test_fused_eval_vs_composition(dev, golden_dir):
    """The fused eval forward against set_fused(False) on every row of every tap.  Both are fp32 evaluations of one
    formula, so the yardstick is the composition's own fp32 error: its distance from the reference's fp32 run on the
    rows the golden stores.  Fused and composed differ by at most 4x that (and never need to beat one rounding)."""
    g, model, data = _tiny(golden_dir, dev)
    fused, taps, mixed = _tapped_eval(model, data)
    plain, ref_taps, ref_mixed = _tapped_eval(model.set_fused(False), data)
    n_in = data["feat"].shape[0]
    pairs = [(n, taps[n].features, ref_taps[n].features, g["tap_" + n]) for n in TAPS]
    pairs.append(("mixed", mixed, ref_mixed, g["tap_mixed"]))
    for name, a, b, ref in pairs:
        err = (a - b).abs().max().item()
        base = np.abs(_stored(name, b, n_in).cpu().numpy() - ref).max()
        print(f"tap {name}: fused - composed {err:.3e}, composed - reference {base:.3e}")
        assert err <= max(4 * base, 2.0 ** -23 * np.abs(ref).max()), (name, err, base)
    assert (fused["pred"] - plain["pred"]).abs().max().item() < FP32_TOL
    assert abs(fused["loss"].item() - plain["loss"].item()) < FP32_TOL


def test_train_step_vs_reference_golden(dev, golden_dir):
    """Loss, curves, every parameter gradient and the running statistics of one training step (the head's Dropout at
    p = 0), with the tolerances of test_keypoint_ptv1_train_step_vs_reference_golden."""
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
    zero = [n for n in params if zero_bias(n)]
    assert len(zero) == 1 + 2 * 4
    for n in zero:
        weight = params[n[:-4] + "weight"].grad.abs().max().item()
        assert params[n].grad.abs().max().item() <= 1e-4 * weight, n
    worst = ("", 0.0)
    for n, p in params.items():
        if n not in zero:
            assert p.grad is not None and p.grad.abs().max().item() > 0, n
            err = (p.grad.float().cpu() - grads[n]).abs().max().item() / max(grads[n].abs().max().item(), 1e-3 * gmax)
            worst = max(worst, (n, err), key=lambda q: q[1])
            assert err < (2e-3 if n.startswith("reg_head.") else 1e-2), (n, err)
    print("worst gradient error", worst)
    for n, b in model.named_buffers():
        if "running" in n:
            ref = torch.from_numpy(g["buf_" + n])
            assert (b.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6) < 1e-4, n


def test_oacnns_segmentor_fused_vs_composition(dev, golden_dir):
    """"OACNNs" itself (with its `final` 1x1x1 conv) on the golden's batch: fused eval against the composition."""
    from pointcept.models import build_model
    g = np.load(os.path.join(golden_dir, "keypoint_oacnns_tiny.npz"))
    kw = {k: v for k, v in TINY_KW.items() if k not in ("num_keypoints", "hidden_dim")}
    model = build_model(dict(type="OACNNs", num_classes=13, **kw))
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    model = model.to(dev).eval()
    data = {k[3:]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("in_")}
    with torch.no_grad():
        fused = model(dict(data))
        plain = model.set_fused(False)(dict(data))
    assert tuple(fused.shape) == (data["feat"].shape[0], 13) and torch.isfinite(fused).all()
    assert (fused - plain).abs().max().item() < FP32_TOL * max(1.0, plain.abs().max().item())


def test_fork_config_eval_and_train_step(dev):
    """configs/my_dataset/keypoint_oa_cnns.py's model dict (23 blocks of 4 grids) on two scenes of 3000 sites."""
    import ptv3_scenes as S
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_OACNNS_CFG
    torch.manual_seed(7)
    model = build_model(KEYPOINT_OACNNS_CFG).to(dev)
    data = {k: v.to(dev) for k, v in S.make_batch([3000, 3000], in_channels=4, extent=64, seed=3).items()}
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
