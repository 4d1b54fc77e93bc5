"""GPU tests of the Sonata self-distillation loss: the kernels of csrc/sonata_loss.hip against tests/sonata_ref.py in
float64, and the model "Sonata-v1m1" against the reference's fixture (tests/golden/sonata_tiny.npz).

Kernel tolerances follow the project's rule (DESIGN.md sections 13 - 15, the check() of test_hip_cac.py): the kernel's
largest error against the float64 yardstick may be at most four times that of the reference's LITERAL formulation
(sonata_ref: exp, total, three row / column rounds, * n, -sum target log_softmax, scene means) evaluated by torch in float32
on the device, with a floor of 8 float32 ulps of the tensor's largest entry.  With bf16 logits both sides start from the
same rounded logits; the gradient, which the kernel writes in the dtype of the student logits, is then compared with the
float32 run's gradient rounded to bf16 once as well (otherwise the bound would ask a bf16 tensor for float32 digits).
Model tolerances are four times the fixture's stored fp32-vs-float64 gap of the same tensor with the floor of one fp32
rounding at the tensor's scale; a gradient, stored as float16 of grad / max|grad|, is also allowed the float16 step of its
stored value.

Shapes: M in {1, 63, 65, 700} pairs (below, across and above the 64 pairs of a workgroup; one wavefront per pair) times K
in {2, 100, 130, 4096} (every entries-per-lane variant: K <= 128, <= 1024, <= 4096, and K that are no multiple of 64), and
(2500, 100): 40 chunks, the last one ragged.  idx_t repeats rows, idx_s skips rows, three scenes of which the middle one
has no pair when M is 1 or 63; T = 0.04 with entries of |x| = 1.  Two fixed cases beside them: every pair in the first two of
three scenes (the trailing scene does not count), and logits, u and gradient in views that start on an odd element of their
storage (an even K otherwise reads pairs of columns, which needs the alignment such a view lacks)."""
import functools

import numpy as np
import pytest
import torch

import sonata_ref as R

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
DEV = "cuda:0"
T, TAU = 0.04, 0.1
MS, KS = [1, 63, 65, 700], [2, 100, 130, 4096]
CASES = [(m, k) for m in MS for k in KS] + [(2500, 100)]
DTYPES = [torch.float32, torch.bfloat16]


def check(name, got, ref64, ref32):
    ref64 = ref64.detach().cpu().double()
    err_k = (got.detach().cpu().double() - ref64).abs().max().item()
    err_t = (ref32.detach().cpu().double() - ref64).abs().max().item()
    top = ref64.abs().max().item()
    bound = max(4.0 * err_t, 8.0 * ULP * top)
    print(f"{name}: kernel {err_k:.3e} torch-fp32 {err_t:.3e} max|ref| {top:.3e} bound {bound:.3e}")
    assert err_k <= bound, (name, err_k, err_t, top)


@functools.lru_cache(maxsize=None)
def inputs(m, k, dtype):
    """teacher logits x (Nt, K) and student logits s (Ns, K): cosines, rounded to `dtype`; idx_t with repeats, idx_s
    strictly increasing with gaps, offsets of three student scenes (the middle one without a pair for m in (1, 63))"""
    g = torch.Generator().manual_seed(7919 * m + k)
    nt, ns, c = m + 7, 2 * m + 11, 24
    unit = lambda rows: torch.nn.functional.normalize(torch.randn(rows, c, generator=g, dtype=torch.float64), dim=1)  # noqa: E731
    proto = unit(k)
    x, s = unit(nt) @ proto.t(), unit(ns) @ unit(k).t()
    x[0, 0], x[nt - 1, k - 1], x[nt // 2, k // 2] = 1.0, -1.0, 1.0
    idx_t = torch.randint(0, nt, (m,), generator=g)
    idx_t[m // 2] = idx_t[0]
    idx_t[-1] = 0
    cut = [ns // 3, 2 * ns // 3, ns]
    rows = torch.randperm(ns, generator=g)
    if m in (1, 63):
        rows = rows[(rows < cut[0]) | (rows >= cut[1])]
    idx_s = rows[:m].sort()[0]
    assert idx_s.shape[0] == m and (m == 1 or (idx_s[1:] > idx_s[:-1]).all())
    x, s = x.to(dtype).double(), s.to(dtype).double()
    return x, idx_t, s, idx_s, torch.tensor(cut)


@functools.lru_cache(maxsize=None)
def refs(m, k, dtype):
    """[float64 on the CPU, float32 on the device] of (sweeps, d, lse, loss, ds) by the literal formulation"""
    x, idx_t, s, idx_s, off = inputs(m, k, dtype)
    out = []
    for dt, dev in ((torch.float64, "cpu"), (torch.float32, DEV)):
        xx, ss, it, is_ = x.to(dev, dt), s.to(dev, dt), idx_t.to(dev), idx_s.to(dev)
        sw, d = R.sweeps(xx, it, T)
        _, lse = R.pair_stats(xx, it, ss, is_, T, TAU)
        loss, _, _ = R.loss(xx, it, ss, is_, off, T, TAU)
        ds = R.dstudent(xx, it, ss, is_, off, T, TAU, dloss=0.75)
        out.append(dict(sweeps=sw, d=d, lse=lse, loss=loss.reshape(1), ds=ds))
    return out


def device_inputs(m, k, dtype, index_dtype=torch.int64):
    x, idx_t, s, idx_s, off = inputs(m, k, dtype)
    return (x.to(DEV, dtype), idx_t.to(DEV, index_dtype), s.to(DEV, dtype), idx_s.to(DEV, index_dtype), off.to(DEV))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("m,k", CASES)
def test_sk_pass(m, k, dtype):
    from ptv3_hip import ops
    assert ops.sonata_capable(k)
    x, idx_t, _, _, _ = device_inputs(m, k, dtype)
    r64, r32 = refs(m, k, dtype)
    u = None
    for i in range(3):
        a, u_next = ops.sonata_sk_pass(x, idx_t, 1.0 / T, u, m)
        again, u_again = ops.sonata_sk_pass(x, idx_t, 1.0 / T, u, m)
        assert torch.equal(a, again) and torch.equal(u_next, u_again)
        check(f"A{i + 1}", a, r64["sweeps"][i][0], r32["sweeps"][i][0])
        check(f"u{i + 1}", u_next, r64["sweeps"][i][1], r32["sweeps"][i][1])
        only_a, none = ops.sonata_sk_pass(x, idx_t, 1.0 / T, u, m, with_u=False)
        assert none is None and torch.equal(only_a, a)
        u = u_next
    # the pairs of all ranks: n_total = 2 M halves every weight
    half, _ = ops.sonata_sk_pass(x, idx_t, 1.0 / T, u, 2 * m)
    full, _ = ops.sonata_sk_pass(x, idx_t, 1.0 / T, u, m)
    assert torch.allclose(half * 2, full, rtol=4 * ULP, atol=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("m,k", CASES)
def test_ce_forward_backward(m, k, dtype):
    from ptv3_hip import ops
    x, idx_t, s, idx_s, off = device_inputs(m, k, dtype)
    r64, r32 = refs(m, k, dtype)
    u = None
    for _ in range(3):
        _, u = ops.sonata_sk_pass(x, idx_t, 1.0 / T, u, m)
    loss, d, lse, gscale = ops.sonata_ce(x, idx_t, 1.0 / T, u, s, idx_s, 1.0 / TAU, off)
    check("loss", loss, r64["loss"], r32["loss"])
    check("d", d, r64["d"], r32["d"])
    check("lse", lse, r64["lse"], r32["lse"])
    scene = R.scene_of(idx_s.cpu().long(), off.cpu())
    count = torch.bincount(scene, minlength=3).double()
    want = torch.where(count > 0, 1.0 / (count * (int(scene.max()) + 1)).clamp(min=1), torch.zeros(3, dtype=torch.float64))
    assert torch.allclose(gscale.cpu().double(), want, rtol=2 * ULP, atol=0)
    if m in (1, 63):
        assert count[1] == 0 and gscale[1] == 0
    dloss = torch.tensor([0.75], device=DEV)
    ds = ops.sonata_ce_bwd(dloss, x, idx_t, 1.0 / T, u, s, idx_s, 1.0 / TAU, off, d, lse, gscale)
    assert ds.dtype == dtype and ds.shape == s.shape
    check("ds", ds, r64["ds"], r32["ds"].to(dtype))
    rest = torch.ones(s.shape[0], dtype=torch.bool, device=DEV)
    rest[idx_s.long()] = False
    assert rest.any() and torch.equal(ds[rest], torch.zeros_like(ds[rest]))
    again = ops.sonata_ce(x, idx_t, 1.0 / T, u, s, idx_s, 1.0 / TAU, off)
    assert all(torch.equal(p, q) for p, q in zip(again, (loss, d, lse, gscale)))
    assert torch.equal(ops.sonata_ce_bwd(dloss, x, idx_t, 1.0 / T, u, s, idx_s, 1.0 / TAU, off, d, lse, gscale), ds)


def test_int32_indices_and_mixed_dtypes():
    from ptv3_hip import ops
    m, k = 65, 130
    x, idx_t, s, idx_s, off = device_inputs(m, k, torch.float32)
    x32, t32, s32, i32, _ = device_inputs(m, k, torch.float32, torch.int32)
    u = u32 = None
    for _ in range(3):
        _, u = ops.sonata_sk_pass(x, idx_t, 1.0 / T, u, m)
        _, u32 = ops.sonata_sk_pass(x32, t32, 1.0 / T, u32, m)
    assert torch.equal(u, u32)
    a = ops.sonata_ce(x, idx_t, 1.0 / T, u, s, idx_s, 1.0 / TAU, off)
    b = ops.sonata_ce(x32, t32, 1.0 / T, u, s32, i32, 1.0 / TAU, off.int())
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    # a bf16 student against an fp32 teacher: the student's rounded logits, upcast, give the same loss bit for bit
    sb = s.bfloat16()
    c = ops.sonata_ce(x, idx_t, 1.0 / T, u, sb, idx_s, 1.0 / TAU, off)
    e = ops.sonata_ce(x, idx_t, 1.0 / T, u, sb.float(), idx_s, 1.0 / TAU, off)
    assert all(torch.equal(p, q) for p, q in zip(c, e))


def test_autograd_function_and_no_pairs():
    from ptv3_hip import autograd as A
    m, k = 65, 100
    x, idx_t, s, idx_s, off = device_inputs(m, k, torch.float32)
    r64, r32 = refs(m, k, torch.float32)
    sv = s.clone().requires_grad_(True)
    loss = A.sonata_loss(sv, x, idx_t, idx_s, off, T, TAU)
    (loss * 0.75).backward()
    check("loss", loss.reshape(1), r64["loss"], r32["loss"])
    check("ds", sv.grad, r64["ds"], r32["ds"])
    # a fake second rank that holds the same pairs: every A doubles, n_total doubles, the target is unchanged
    twice = A.sonata_loss(s, x, idx_t, idx_s, off, T, TAU, n_total=2 * m, all_reduce=lambda a: a.mul_(2))
    assert abs(twice.item() - loss.item()) <= 8 * ULP * abs(loss.item())
    sv.grad = None
    none = idx_t[:0]
    zero = A.sonata_loss(sv, x, none, none, off, T, TAU)
    zero.backward()
    assert zero.item() == 0.0 and torch.equal(sv.grad, torch.zeros_like(sv))


def test_refusals():
    from ptv3_hip import ops
    x, idx_t, s, idx_s, off = device_inputs(65, 100, torch.float32)
    assert not ops.sonata_capable(1) and not ops.sonata_capable(4097) and ops.sonata_capable(2)
    with pytest.raises(RuntimeError, match="finite"):
        ops.sonata_sk_pass(x, idx_t, float("inf"))
    with pytest.raises(RuntimeError, match="finite"):
        ops.sonata_sk_pass(x, idx_t, float("nan"))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.sonata_sk_pass(x.cpu(), idx_t, 25.0)
    wide = torch.zeros(4, 4100, device=DEV)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.sonata_sk_pass(wide, idx_t[:2].clamp(max=3), 25.0)


# ---- the model against the reference's fixture ----------------------------------------------------------------------
from make_golden_sonata import load_golden, sonata_state_dict, TINY_KW, LOSSES, SEED, MOMENTUM  # noqa: E402

_G = {}


def golden(golden_dir):
    if not _G:
        _G.update(load_golden(golden_dir))
    return _G


def _close(name, got, want, gap, extra=0.0):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    floor = ULP * np.abs(want).max()             # one fp32 rounding at the tensor's scale: a stored gap can be less
    print(f"{name}: err {err.max():.3e} gap {gap:.3e} floor {floor:.3e}")
    assert (err <= np.maximum(4 * gap, floor) + extra).all(), (name, err.max(), gap)


def _grad_bound(g, name):
    stored = g["grad_" + name].astype(np.float64) * float(g["gmax_" + name])
    return stored, 2.0 ** -11 * np.abs(stored) + 2.0 ** -24 * float(g["gmax_" + name])


def _model(g, fused, monkeypatch=None, **kw):
    """the tiny model on the device, replaying the fixture's patch permutation; fused: every loss through the kernels,
    whatever `wired` lists (the wiring is a measurement, not a capability)"""
    import copy
    from pointcept.models import build_model
    from pointcept.models.sonata import sonata_v1m1_base as M
    model = build_model(dict(type="Sonata-v1m1", **dict(copy.deepcopy(TINY_KW), **kw)))
    if not kw:
        sonata_state_dict(model)
    model = model.to(DEV).set_fused(fused).train()
    real, perm = model.generate_mask, torch.from_numpy(g["patch_index"]).to(DEV)
    model.generate_mask = lambda coord, offset: real(coord, offset, patch_index=perm)
    if monkeypatch is not None:
        monkeypatch.setattr(M, "wired", lambda kernel, k, m: True)
    return model


def _data(g):
    return {k[3:]: torch.from_numpy(g[k]).to(DEV) for k in g if k.startswith("in_")}


_STEP = {}


def _train_step(g, fused, monkeypatch):
    if fused not in _STEP:
        from ptv3_hip import autograd as A
        calls = []
        real = A.sonata_loss
        monkeypatch.setattr(A, "sonata_loss", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
        model = _model(g, fused, monkeypatch)
        torch.manual_seed(SEED)
        out = model(_data(g))
        out["loss"].backward()
        torch.cuda.synchronize()
        assert len(calls) == (3 if fused else 0)
        _STEP[fused] = ({k: out[k].item() for k in out},
                        {k: (None if p.grad is None else p.grad.detach().cpu().numpy()) for k, p in model.named_parameters()},
                        model)
    return _STEP[fused]


@pytest.mark.parametrize("fused", [True, False])
def test_model_training_step_matches_reference(golden_dir, fused, monkeypatch):
    g = golden(golden_dir)
    losses, grads, model = _train_step(g, fused, monkeypatch)
    assert sorted(losses) == sorted(LOSSES)
    for k in LOSSES:
        _close(k, losses[k], g[k], float(g["gap_" + k]))
    nograd = set(g["nograd"].tolist())
    assert {k for k, v in grads.items() if v is None} == nograd
    assert all(not p.requires_grad for p in model.teacher.parameters())
    assert len(grads) - len(nograd) == sum(1 for k in g if k.startswith("gmax_"))
    for name, got in grads.items():
        if got is not None:
            stored, step = _grad_bound(g, name)
            _close("grad " + name, got, stored, float(g["gap_grad_" + name]), step)


def test_model_views_match_reference(golden_dir):
    g = golden(golden_dir)
    model = _model(g, False)
    data = _data(g)
    mask, cluster = model.generate_mask(data["global_coord"], data["global_offset"])
    assert torch.equal(mask.cpu(), torch.from_numpy(g["point_mask"]))
    assert torch.equal(cluster.cpu(), torch.from_numpy(g["point_cluster"]))
    free, _ = type(model).generate_mask(model, data["global_coord"], data["global_offset"])
    assert free.shape == mask.shape and 0.2 < free.float().mean().item() < 0.8
    origin, offset = data["global_origin_coord"], data["global_offset"]
    match = model.match_neighbour(origin, offset, origin, offset)
    assert torch.equal(match[:, 0], match[:, 1]) and match.shape[0] == origin.shape[0]
    from pointcept.models.utils.structure import Point
    rolled = model.roll_point(Point(feat=data["global_feat"], coord=data["global_coord"], origin_coord=origin,
                                    offset=offset))
    perm = torch.from_numpy(g["roll_perm"]).to(DEV)
    assert torch.equal(rolled.origin_coord, origin[perm]) and torch.equal(rolled.feat, data["global_feat"][perm])
    match = model.match_neighbour(origin, offset, rolled.origin_coord, rolled.offset)
    want = torch.from_numpy(g["match_roll_mask"]).to(DEV)
    assert torch.equal(match[:, 0], want[:, 0]) and torch.equal(perm[match[:, 1]], want[:, 1])


def test_model_fused_and_composed_agree(golden_dir, monkeypatch):
    g = golden(golden_dir)
    (l1, g1, _), (l0, g0, _) = _train_step(g, True, monkeypatch), _train_step(g, False, monkeypatch)
    for k in LOSSES:
        _close(k, l1[k], l0[k], float(g["gap_" + k]))
    for name in g1:
        if g1[name] is not None:
            _close("grad " + name, g1[name], g0[name], float(g["gap_grad_" + name]))


def test_model_after_step_and_return_point(golden_dir, monkeypatch):
    g = golden(golden_dir)
    _, _, model = _train_step(g, True, monkeypatch)
    model.momentum = MOMENTUM
    model.after_step()
    torch.cuda.synchronize()
    for k, p in model.teacher.named_parameters():
        _close("ema " + k, p.detach().cpu().numpy(), g["ema_" + k], float(g["gap_ema_" + k]))
    data = _data(g)
    with torch.no_grad():
        torch.manual_seed(SEED)
        out = model.eval()(dict(feat=data["global_feat"], coord=data["global_coord"], offset=data["global_offset"],
                                grid_size=data["grid_size"][0]), return_point=True)
    point = out["point"]
    assert tuple(point.feat.shape) == (data["global_feat"].shape[0], 64) and torch.isfinite(point.feat).all()
    assert "pooling_parent" not in point.keys()


def test_model_composes_outside_the_kernels_range(golden_dir, monkeypatch):
    """5000 prototypes lie outside ptv3_sonata_capable: the model asked for the fused path composes without a word, and
    gives what set_fused(False) gives"""
    from ptv3_hip import ops, autograd as A
    g = golden(golden_dir)
    assert not ops.sonata_capable(5000)
    monkeypatch.setattr(A, "sonata_loss", lambda *a, **k: pytest.fail("the kernels were called at K = 5000"))
    torch.manual_seed(11)
    model = _model(g, True, monkeypatch, head_num_prototypes=5000)
    outs = []
    for fused in (True, False):
        model.set_fused(fused).zero_grad()
        torch.manual_seed(SEED)
        out = model(_data(g))
        out["loss"].backward()
        outs.append(({k: out[k].item() for k in LOSSES}, model.student.mask_head.mlp[0].weight.grad.clone()))
    for k in LOSSES:
        assert np.isfinite(outs[0][0][k]) and abs(outs[0][0][k] - outs[1][0][k]) <= 16 * ULP * abs(outs[1][0][k])
    assert torch.allclose(outs[0][1], outs[1][1], rtol=1e-4, atol=1e-7 * outs[1][1].abs().max().item())


def test_trailing_scene_without_a_pair_does_not_count():
    """three student scenes, every pair in the first two: B = 2, the third scene's factor is 0 and its rows get zeros"""
    from ptv3_hip import ops
    m, k = 65, 100
    x, idx_t, s, _, off = inputs(m, k, torch.float32)
    idx_s = torch.arange(0, 2 * m, 2)[:m]
    idx_s = idx_s[idx_s < off[1]]
    m = idx_s.shape[0]
    idx_t = idx_t[:m]
    assert m > 40 and R.scene_of(idx_s, off).unique().tolist() == [0, 1]
    want, _, _ = R.loss(x, idx_t, s, idx_s, off, T, TAU)
    fp32, _, _ = R.loss(x.float().to(DEV), idx_t.to(DEV), s.float().to(DEV), idx_s.to(DEV), off, T, TAU)
    grad = R.dstudent(x, idx_t, s, idx_s, off, T, TAU)
    grad32 = R.dstudent(x.float().to(DEV), idx_t.to(DEV), s.float().to(DEV), idx_s.to(DEV), off, T, TAU)
    xd, sd, td, sid, od = x.float().to(DEV), s.float().to(DEV), idx_t.to(DEV), idx_s.to(DEV), off.to(DEV)
    u = None
    for _ in range(3):
        _, u = ops.sonata_sk_pass(xd, td, 1.0 / T, u, m)
    loss, d, lse, gscale = ops.sonata_ce(xd, td, 1.0 / T, u, sd, sid, 1.0 / TAU, od)
    check("loss", loss, want.reshape(1), fp32.reshape(1))
    count = torch.bincount(R.scene_of(idx_s, off), minlength=3)
    assert gscale[2].item() == 0.0 and count[2] == 0
    assert torch.allclose(gscale[:2].cpu().double(), 1.0 / (2.0 * count[:2].double()), rtol=2 * ULP, atol=0)
    ds = ops.sonata_ce_bwd(torch.ones(1, device=DEV), xd, td, 1.0 / T, u, sd, sid, 1.0 / TAU, od, d, lse, gscale)
    check("ds", ds, grad, grad32)
    assert torch.equal(ds[int(off[1]):], torch.zeros_like(ds[int(off[1]):]))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_views_that_start_on_an_odd_element(dtype):
    """an even K reads pairs of columns, which needs 8-byte (fp32) or 4-byte (bf16) aligned rows; a contiguous view that
    starts one element into its storage is not, and must give the same results through the one-column loads"""
    from ptv3_hip import ops
    m, k = 65, 130
    x, idx_t, s, idx_s, off = device_inputs(m, k, dtype)
    r64, r32 = refs(m, k, dtype)

    def shifted(t):
        store = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        view = store[1:].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % (2 * t.element_size()) != 0
        return view

    xs, ss = shifted(x), shifted(s)
    u = None
    for i in range(3):
        a, u_next = ops.sonata_sk_pass(xs, idx_t, 1.0 / T, None if u is None else shifted(u), m)
        check(f"A{i + 1}", a, r64["sweeps"][i][0], r32["sweeps"][i][0])
        u = u_next
    loss, d, lse, gscale = ops.sonata_ce(xs, idx_t, 1.0 / T, shifted(u), ss, idx_s, 1.0 / TAU, off)
    check("loss", loss, r64["loss"], r32["loss"])
    check("d", d, r64["d"], r32["d"])
    ds = ops.sonata_ce_bwd(torch.tensor([0.75], device=DEV), xs, idx_t, 1.0 / T, u, ss, idx_s, 1.0 / TAU, off, d, lse, gscale)
    check("ds", ds, r64["ds"], r32["ds"].to(dtype))
