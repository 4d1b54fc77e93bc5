"""KeypointStratifiedTransformer on the GPU: the attention plan against tests/strat_ref.py, the ball query against numpy,
the relative-position index against torch's CPU fp32 expression, ptv3_strat_attn_fwd against the float64 formula
(shapes, ragged tiles, key chunks, overflow, determinism, canary), and the model against the reference's own outputs
(tests/golden/keypoint_strat_tiny.npz: sampled rows, group counts, taps, eval, one training step), the fused eval forward
against the edge composition, and the fork config end to end."""
import os

import numpy as np
import pytest
import torch

import strat_ref as R
from make_golden_keypoint_strat import (seeded_state_dict, TINY_KW, TAP_STRIDE, CELL_MARGIN, FP16_STEP, cell_margins,
                                        unpack_grads, _zero_bias)
from test_keypoint_strat_cpu import GAPS, _cloud

pytestmark = pytest.mark.gpu
MARGIN4 = 4.0     # every tolerance is four times the fp32-vs-float64 error of the same formula


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _margin_cloud(sizes, window, edge=0.9):
    for seed in range(200):
        coord, ends, down = _cloud(seed, sizes, edge)
        margin, same = cell_margins(coord, window)
        if margin >= CELL_MARGIN and same:
            return coord, ends, down
    raise AssertionError("no seed holds the cell margin")


def _plan_groups(plan):
    q_ptr, k_ptr = plan.q_ptr.cpu().numpy(), plan.k_ptr.cpu().numpy()
    q_rows, k_rows = plan.q_rows.cpu().numpy(), plan.k_rows.cpu().numpy()
    return [(q_rows[q_ptr[g]:q_ptr[g + 1]], k_rows[k_ptr[g]:k_ptr[g + 1]]) for g in range(plan.n_groups)]


# ------------------------------------------------------------------------------------------------
# plan, ball query, relative-position index
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [False, True])
def test_plan_equals_reference(dev, shifted):
    """Scenes of 1, 7 and 700 points: every point is a query of exactly one group, and per query the key rows equal
    strat_ref's exactly (as sorted lists, so a key counted twice would show)."""
    from ptv3_hip import ops
    coord, ends, down = _margin_cloud([1, 7, 700], 0.2)
    plan = ops.stratified_plan(torch.from_numpy(coord).to(dev), torch.tensor(ends, dtype=torch.int32, device=dev),
                               torch.from_numpy(down).to(dev), 0.2, shifted)
    ref = R.group_plan(coord, ends, down, 0.2, shifted)
    assert plan.n_groups == len(ref) and plan.n_keys == sum(len(k) for _, k in ref)
    assert plan.q_rows.dtype == torch.int32 and plan.k_rows.shape[0] == plan.n_keys
    got = R.keys_per_query(_plan_groups(plan), len(coord))
    want = R.keys_per_query(ref, len(coord))
    for i in range(len(coord)):
        assert got[i] is not None and np.array_equal(got[i], want[i]), i
    again = ops.stratified_plan(torch.from_numpy(coord).to(dev), torch.tensor(ends, dtype=torch.int32, device=dev),
                                torch.from_numpy(down).to(dev), 0.2, shifted)
    assert torch.equal(again.k_rows, plan.k_rows) and torch.equal(again.q_rows, plan.q_rows)
    # the edge list expanded from the plan is the reference's, per query
    i0, i1 = (t.cpu().numpy() for t in plan.edges())
    r0, r1 = R.reference_edges(coord, ends, down, 0.2, shifted)
    assert np.array_equal(i0, r0)
    starts = np.searchsorted(r0, np.arange(len(coord) + 1))
    for i in range(len(coord)):
        assert np.array_equal(np.sort(i1[starts[i]:starts[i + 1]]), np.sort(r1[starts[i]:starts[i + 1]])), i


@pytest.mark.parametrize("max_neighbor", [1, 34])
def test_ball_query_exact(dev, max_neighbor):
    """Scenes of 300, 1 and 500 points with a 60-point blob (more candidates than slots), radius 0.05: exact against
    numpy.  No squared distance lies within a relative 1e-5 of r^2 (asserted), so fp32 cannot decide otherwise."""
    from ptv3_hip import ops
    for seed in range(50):
        rs = np.random.RandomState(seed)
        parts = [rs.rand(300, 3) * [0.5, 0.5, 0.05], rs.rand(1, 3), rs.rand(500, 3) * [0.6, 0.6, 0.05] + 2]
        parts[2][-60:] = parts[2][10] + 0.01 * rs.randn(60, 3)
        coord = np.concatenate(parts).astype(np.float32)
        ends = np.array([300, 301, 801])
        ref, margin = R.ball_query(0.05, max_neighbor, coord, ends)
        if margin >= 1e-5:
            break
    else:
        raise AssertionError("no seed holds the margin")
    full, _ = R.ball_query(0.05, 200, coord, ends)
    assert (full[:, 34] >= 0).any()                        # rows with more than 34 candidates
    got = ops.ball_query(0.05, max_neighbor, torch.from_numpy(coord).to(dev),
                         torch.tensor(ends, dtype=torch.int32, device=dev))
    assert got.dtype == torch.int64 and tuple(got.shape) == (801, max_neighbor)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert got[300, 0].item() == 300 and (got[300, 1:] == -1).all()      # the one-point scene holds itself
    if max_neighbor == 34:
        assert (ref[:, -1] >= 0).any() and (ref[:, 1] < 0).any()


def test_rel_index_equals_torch_cpu_fp32(dev):
    """10^5 random pairs plus pairs whose difference times 1e5 is an exact .5 tie, three (window, quant) settings:
    bit-for-bit torch's CPU fp32 value (round-half-even, IEEE division, no contraction)."""
    from ptv3_hip import ops
    ties = (np.arange(-4000, 4000, dtype=np.float64) + 0.5) / 1e5
    xi = np.float32(0.25) + np.zeros(len(ties), dtype=np.float32)
    xj = (xi.astype(np.float64) - ties).astype(np.float32)
    prod = (xi - xj) * np.float32(100000.0)
    assert (np.abs(prod - np.rint(prod)) == 0.5).sum() > 100
    rs = np.random.RandomState(0)
    n = len(ties) + 100000
    a = np.concatenate([np.stack([xi, xi, xi], 1), rs.rand(100000, 3).astype(np.float32) * 0.39])
    b = np.concatenate([np.stack([xj, xj, xj], 1), rs.rand(100000, 3).astype(np.float32) * 0.39])
    coord = torch.from_numpy(np.concatenate([a, b]))
    i0, i1 = torch.arange(n), torch.arange(n) + n
    for w, quant in ((0.2, 0.01), (0.4, 0.05), (1.6, 0.08)):
        rows = 2 * int((2 * w + 1e-4) // quant)
        want = R.rel_index(coord, i0, i1, w, quant).int()
        assert want.min() >= 0 and want.max() <= rows - 1
        got = ops.strat_rel_index(coord.to(dev), i0.to(dev), i1.to(dev), w, quant, rows)
        assert torch.equal(got.cpu(), want), (w, quant)


# ------------------------------------------------------------------------------------------------
# the fused attention
# ------------------------------------------------------------------------------------------------
def _hand_plan(groups, dev):
    from ptv3_hip.ops import StratPlan
    q_ptr = np.cumsum([0] + [len(q) for q, _ in groups])
    k_ptr = np.cumsum([0] + [len(k) for _, k in groups])
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device=dev)   # noqa: E731
    return StratPlan(t(q_ptr), t(np.concatenate([q for q, _ in groups])), t(k_ptr),
                     t(np.concatenate([k for _, k in groups])), len(groups), int(k_ptr[-1]), 0)


def _real_groups(sizes, window, shifted):
    coord, ends, down = _margin_cloud(sizes, window)
    return coord, R.group_plan(coord, ends, down, window, shifted)


def _box_groups(layout, seed, edge=0.19):
    """Hand-made groups inside one box of `edge` (so every |difference| < 2 window): layout = [(queries, extra keys)];
    a group's keys are its queries and then `extra` rows that are nobody's query.  The last row stays outside the plan."""
    rs = np.random.RandomState(seed)
    groups, at = [], 0
    for nq, extra in layout:
        q = np.arange(at, at + nq)
        k = np.arange(at, at + nq + extra)
        at += nq + extra
        groups.append((q, rs.permutation(k)))
    coord = (rs.rand(at + 1, 3) * edge).astype(np.float32)
    return coord, groups


CASES = {
    "tiny_level0": lambda: (2, 0.2, 0.01) + _real_groups([1, 7, 400], 0.2, False),
    "tiny_level0_shifted": lambda: (2, 0.2, 0.01) + _real_groups([1, 7, 400], 0.2, True),
    "tiny_level1": lambda: (4, 0.4, 0.05) + _real_groups([3, 95, 164], 0.4, True),
    "one_pair": lambda: (1, 0.2, 0.1) + _box_groups([(1, 0)], 1),
    "ragged_17x33": lambda: (6, 0.2, 0.01) + _box_groups([(17, 16)] * 3, 2),
    "chunks_40x700": lambda: (24, 0.2, 0.01) + _box_groups([(40, 660)], 3),
    "dense_only_24_rows": lambda: (4, 0.3, 0.05) + _box_groups([(1, 0), (5, 0), (16, 0), (31, 0), (50, 0)], 4, edge=0.29),
}
TABLE_ROWS = {"tiny_level0": 80, "tiny_level0_shifted": 80, "tiny_level1": 32, "one_pair": 8, "ragged_17x33": 80,
              "chunks_40x700": 80, "dense_only_24_rows": 24}


def _attention_case(dev, name, q_scale=1.0):
    from ptv3_hip import ops
    heads, w, quant, coord, groups = CASES[name]()
    rows = 2 * int((2 * w + 1e-4) // quant)
    assert rows == TABLE_ROWS[name]
    n, d = len(coord), 16
    g = torch.Generator().manual_seed(len(name) + heads)
    qkv = torch.randn(n, 3, heads, d, generator=g)
    qkv[:, 0] *= q_scale
    tabs = [0.2 * torch.randn(rows, heads, d, 3, generator=g) for _ in range(3)]
    c = torch.from_numpy(coord)
    i0 = np.concatenate([np.repeat(qr, len(kr)) for qr, kr in groups])
    i1 = np.concatenate([np.tile(kr, len(qr)) for qr, kr in groups])
    order = np.argsort(i0, kind="stable")
    i0, i1 = torch.from_numpy(i0[order]), torch.from_numpy(i1[order])
    rel = R.rel_index(c, i0, i1, w, quant)
    assert rel.min() >= 0 and rel.max() <= rows - 1
    scale = d ** -0.5
    args64 = [t.double() for t in (qkv[:, 0], qkv[:, 1], qkv[:, 2])]
    ref = R.edge_attention(*args64, c, i0, i1, *[t.double() for t in tabs], scale, w, quant, rel=rel)
    e32 = (R.edge_attention(qkv[:, 0], qkv[:, 1], qkv[:, 2], c, i0, i1, *tabs, scale, w, quant, rel=rel).double()
           - ref).abs().max().item()
    plan = _hand_plan(groups, dev)
    packed = [ops.strat_pack_tables(t.to(dev)) for t in tabs]
    queried = np.zeros(n, dtype=bool)
    queried[np.concatenate([q for q, _ in groups])] = True
    out = torch.full((n, heads, d), -7.0, device=dev)
    got = ops.stratified_attention(qkv.to(dev), c.to(dev), plan, *packed, scale, w, quant, out=out, check=True)
    again = ops.stratified_attention(qkv.to(dev), c.to(dev), plan, *packed, scale, w, quant,
                                     out=torch.full((n, heads, d), -7.0, device=dev), check=True)
    torch.cuda.synchronize()
    assert torch.equal(got, again)                                   # bitwise reproducible
    got = got.cpu()
    if (~queried).any():
        assert (got[~queried] == -7.0).all()                         # rows outside the plan are untouched
    err = (got[queried].double() - ref[queried]).abs().max().item()
    print(f"strat attn {name} (heads {heads}, rows {rows}, {len(groups)} groups, {len(i0)} pairs, q x{q_scale}): err "
          f"{err:.3e}, fp32 edge composition E {e32:.3e}, max|ref| {ref.abs().max().item():.3f}")
    assert torch.isfinite(got).all()
    assert err <= MARGIN4 * e32, (name, err, e32)


@pytest.mark.parametrize("name", list(CASES))
def test_strat_attention_vs_float64(dev, name):
    """Yardstick E = the reference's edge pipeline (the three pointops2 functions and scatter_softmax) in fp32 torch
    against the same in float64, both with the fp32 relative-position index: the kernel stays within 4 E."""
    _attention_case(dev, name)


def test_strat_attention_large_logits(dev):
    """q scaled by 30: exp of an un-shifted logit overflows fp32; the running maximum keeps every weight finite."""
    _attention_case(dev, "ragged_17x33", q_scale=30.0)
    _attention_case(dev, "chunks_40x700", q_scale=30.0)


def test_strat_attention_refuses_unsupported(dev):
    from ptv3_hip import ops
    coord, groups = _box_groups([(4, 0)], 0)
    plan = _hand_plan(groups, dev)
    c = torch.from_numpy(coord).to(dev)
    for heads, d, rows in ((2, 8, 80), (2, 32, 80), (2, 16, 96)):
        qkv = torch.zeros(len(coord), 3, heads, d, device=dev)
        tab = torch.zeros(3, rows, heads, d, device=dev)
        assert not ops.strat_attn_capable(heads, d, rows)
        with pytest.raises(NotImplementedError, match="not served"):
            ops.stratified_attention(qkv, c, plan, tab, tab, tab, 0.25, 0.2, 0.01)
    bad = _hand_plan([(np.array([0, 1]), np.array([0, len(coord)]))], dev)
    qkv = torch.zeros(len(coord), 3, 2, 16, device=dev)
    tab = torch.zeros(3, 80, 2, 16, device=dev)
    with pytest.raises(ValueError, match="out of range"):
        ops.stratified_attention(qkv, c, bad, tab, tab, tab, 0.25, 0.2, 0.01, check=True)


# ------------------------------------------------------------------------------------------------
# the model against the reference's own outputs
# ------------------------------------------------------------------------------------------------
def _tiny(golden_dir, dev):
    from pointcept.models import build_model
    g = np.load(os.path.join(golden_dir, "keypoint_strat_tiny.npz"))
    model = build_model(dict(type="KeypointStratifiedTransformer", **TINY_KW))
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    data = {k[3:]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("in_")}
    return g, model.to(dev), data


def _tapped_eval(model, data):
    taps, hooks = {}, []
    hooks.append(model.point_embed[-1].register_forward_hook(lambda m, i, o: taps.__setitem__("embed", o.detach())))
    for i, layer in enumerate(model.layers):
        layer.record = {}
        hooks.append(layer.register_forward_hook(lambda m, inp, out, i=i: taps.__setitem__(f"layer{i}", out[0].detach())))
    for i, up in enumerate(model.up):
        hooks.append(up.register_forward_hook(lambda m, inp, out, i=i: taps.__setitem__(f"up{i}", out[0].detach())))
    with torch.no_grad():
        out = model.eval()(dict(data))
    for h in hooks:
        h.remove()
    for i, layer in enumerate(model.layers):
        taps[f"record{i}"], layer.record = layer.record, None
    return out, taps


def test_keypoint_strat_eval_vs_reference_golden(dev, golden_dir):
    """The rows BasicLayer sampled and each plan's group and pair counts: exact.  Every stage's features, `pred` and
    `loss`: within four times the reference's own fp32-vs-float64 gap (GAPS)."""
    g, model, data = _tiny(golden_dir, dev)
    out, taps = _tapped_eval(model, data)
    for i in range(2):
        rec = taps[f"record{i}"]
        assert np.array_equal(rec["down_idx"].cpu().numpy(), g[f"rows_layer{i}_down_idx"]), i
        for parity, plan in enumerate(rec["plans"]):
            assert plan.n_groups == int(g[f"groups_{i}_{parity}"]), (i, parity)
            nq = (plan.q_ptr[1:] - plan.q_ptr[:-1]).long()
            nk = (plan.k_ptr[1:] - plan.k_ptr[:-1]).long()
            assert int((nq * nk).sum().item()) == int(g[f"edges_{i}_{parity}"]), (i, parity)
    for name, stride in TAP_STRIDE.items():
        ref = g["tap_" + name]
        got = taps[name].cpu().numpy()[::stride]
        err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
        print(f"{name}: err {err:.3e}, tolerance {MARGIN4 * GAPS[name]:.3e}")
        assert err <= MARGIN4 * GAPS[name], (name, err)
    assert tuple(out["pred"].shape) == (3, 6, 3) and out["pred"].dtype == torch.float32
    err = np.abs(out["pred"].cpu().numpy() - g["eval_pred"]).max()
    print(f"pred: err {err:.3e}, tolerance {MARGIN4 * GAPS['pred']:.3e}")
    assert err <= MARGIN4 * GAPS["pred"]
    err = abs(out["loss"].item() - float(g["eval_loss"]))
    print(f"eval loss: err {err:.3e}, tolerance {MARGIN4 * GAPS['eval_loss']:.3e}")
    assert err <= MARGIN4 * GAPS["eval_loss"]


def test_keypoint_strat_train_step_vs_reference_golden(dev, golden_dir):
    """Loss, curves, every parameter gradient and the BatchNorm running statistics of one training step (the head's
    Dropout at p = 0) within four times the reference's own fp32-vs-float64 gap; a gradient is held to the gap of its
    own tensor (gap_grads) plus the float16 step of the stored values."""
    g, model, data = _tiny(golden_dir, dev)
    model.train()
    model.reg_head[3].p = 0.0
    out = model(dict(data))
    out["loss"].backward()
    assert abs(out["loss"].item() - float(g["loss"])) <= MARGIN4 * GAPS["loss"]
    assert abs(out["train/mean_dist"].item() - float(g["mean_dist"])) <= MARGIN4 * GAPS["mean_dist"]
    kp = np.array([out[f"train/kp{i}_dist"].item() for i in range(6)])
    assert np.abs(kp - g["kp_dist"]).max() <= MARGIN4 * GAPS["kp_dist"]
    params = {k: p for k, p in model.named_parameters() if p.grad is not None}
    absent = [k for k, p in model.named_parameters() if p.grad is None]
    # no gradient: the frozen kernel points and the residual block's unused BatchNorm, as in the reference
    assert sorted(absent) == sorted(["point_embed.0.kpconv.K_points", "point_embed.1.kpconv.K_points",
                                     "point_embed.1.bn.batch_norm.weight", "point_embed.1.bn.batch_norm.bias"])
    grads = unpack_grads(g["grads"], g["gmax"], {k: tuple(v.shape) for k, v in params.items()})
    gmax = float(g["gmax"].max())
    gaps = dict(zip(params, g["gap_grads"].tolist()))
    worst = 0.0
    assert sum(_zero_bias(n) for n in params) == 5     # the head's first bias and the last TransitionUp's four
    for n, p in params.items():
        if _zero_bias(n):
            weight = params[n[:-4] + "weight"].grad.abs().max().item()
            assert p.grad.abs().max().item() <= 1e-4 * weight, n
            continue
        ref = torch.from_numpy(grads[n])
        err = (p.grad.float().cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3 * gmax)
        worst = max(worst, err)
        assert err <= MARGIN4 * gaps[n] + FP16_STEP, (n, err, gaps[n])
    print("worst gradient error", worst)
    bufs = [(n, b) for n, b in model.named_buffers() if "running" in n]
    flat, at = g["bufs"], 0
    for n, b in bufs:
        ref = torch.from_numpy(flat[at:at + b.numel()].reshape(tuple(b.shape)))
        at += b.numel()
        assert (b.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6) <= MARGIN4 * GAPS["buf"], n
    assert at == len(flat)


def test_eval_equals_edge_composition(dev, golden_dir):
    """The fused eval forward against set_fused(False) (the pointops2 edge composition) on every row of every stage:
    within eight gaps of each other (each side within four of the float64 value)."""
    g, model, data = _tiny(golden_dir, dev)
    fused, taps = _tapped_eval(model, data)
    plain, ref_taps = _tapped_eval(model.set_fused(False), data)
    for name in TAP_STRIDE:
        a, b = taps[name], ref_taps[name]
        err = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
        assert err <= 2 * MARGIN4 * GAPS[name], (name, err)
    assert (fused["pred"] - plain["pred"]).abs().max().item() <= 2 * MARGIN4 * GAPS["pred"]


def test_fork_config_eval(dev):
    """KeypointStratifiedTransformer from configs/my_dataset/keypoint_stratified_transformer.py's model dict on two
    seeded scenes of 3000 points on a sheet: finite `pred` of the right shape."""
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_STRAT_CFG
    torch.manual_seed(7)
    model = build_model(KEYPOINT_STRAT_CFG).to(dev)
    xy = torch.rand(6000, 2) * 1.5
    coord = torch.cat([xy, 0.1 * torch.sin(3 * xy[:, :1]) + 0.01 * torch.randn(6000, 1)], 1)
    data = dict(coord=coord.to(dev), feat=torch.randn(6000, 4).to(dev),
                offset=torch.tensor([3000, 6000], dtype=torch.int32, device=dev))
    with torch.no_grad():
        pred = model.eval()(dict(data))["pred"]
    assert tuple(pred.shape) == (2, 6, 3) and torch.isfinite(pred).all()
