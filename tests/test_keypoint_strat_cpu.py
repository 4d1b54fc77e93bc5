"""CPU-side checks of KeypointStratifiedTransformer / ST-v1m2: the group plan of tests/strat_ref.py against a literal
transcription of BasicLayer.forward's masks, the group formula against the three-function edge pipeline in float64, the
relative-position index at exact .5 ties, the fixture's stated gaps and margins, the fork config's state_dict, the two
sample-count quirks, the pointops2 surface and the argument refusals of the new entry points without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import strat_ref as R
from make_golden_keypoint_strat import TINY_KW, CELL_MARGIN, cell_margins

N_TINY_PARAMS = 223268
# fp32 torch (CPU) against float64 on the fixture's batch, as tests/golden/make_golden_keypoint_strat.py printed them
GAPS = {
    "embed": 2.663e-07, "layer0": 3.260e-07, "layer1": 5.510e-07, "up0": 4.792e-07, "up1": 4.260e-07,
    "pred": 8.711e-07, "eval_loss": 7.489e-08, "loss": 3.497e-07, "mean_dist": 1.676e-07, "kp_dist": 2.234e-06,
    "buf": 1.810e-07,
}


def _cloud(seed, sizes, edge=0.9):
    rs = np.random.RandomState(seed)
    coord = np.concatenate([rs.rand(n, 3) * [edge, edge, 0.3] + rs.randn(3) for n in sizes]).astype(np.float32)
    ends = np.cumsum(sizes)
    down = np.concatenate([s + np.sort(rs.choice(e - s, (e - s) // 4 + 1, replace=False))
                           for s, e in zip([0] + ends[:-1].tolist(), ends.tolist())])
    return coord, ends, down


@pytest.mark.parametrize("shifted", [False, True])
def test_group_plan_equals_reference_masks(shifted):
    """Per query, the multiset of keys: the plan (every row of the query's small window + the sampled rows of its large
    window in another small window) against BasicLayer.forward's [windows, k, k] masks, transcribed in numpy.  The cloud
    is checked to hold the cell margin, so the reference's second shifted expression gives the same cells."""
    for seed in range(40):
        coord, ends, down = _cloud(seed, [1, 7, 500])
        if cell_margins(coord, 0.2)[0] >= CELL_MARGIN and cell_margins(coord, 0.2)[1]:
            break
    else:
        raise AssertionError("no seed holds the margin")
    groups = R.group_plan(coord, ends, down, 0.2, shifted)
    assert sum(len(q) for q, _ in groups) == len(coord)
    keys = R.keys_per_query(groups, len(coord))
    i0, i1 = R.reference_edges(coord, ends, down, 0.2, shifted)
    assert len(i0) == sum(len(k) for k in keys)
    starts = np.searchsorted(i0, np.arange(len(coord) + 1))
    for i in range(len(coord)):
        assert np.array_equal(np.sort(i1[starts[i]:starts[i + 1]]), keys[i]), i
    c = torch.from_numpy(coord)
    small = R.cells(c, c.min(0).values, 0.2, shifted, False).numpy()
    batch = np.repeat(np.arange(len(ends)), np.diff(np.concatenate([[0], ends])))
    cells = len({(b,) + tuple(s) for b, s in zip(batch, small)})
    # unshifted: small windows nest in large ones; shifted: a small window straddles large ones and splits into groups
    assert len(groups) > cells if shifted else len(groups) == cells


def test_group_formula_equals_edge_pipeline_float64():
    """softmax over a group's keys = attention_step1_v2 + dot_prod_with_idx_v3 -> scatter_softmax ->
    attention_step2_with_rel_pos_value_v2 over the expanded edge list, in float64 to rounding."""
    coord, ends, down = _cloud(3, [5, 120], edge=0.5)
    h, d, w, quant = 3, 16, 0.2, 0.01
    rows = 2 * int((2 * w + 1e-4) // quant)
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(len(coord), h, d, generator=g, dtype=torch.float64) for _ in range(3))
    tq, tk, tv = (0.3 * torch.randn(rows, h, d, 3, generator=g, dtype=torch.float64) for _ in range(3))
    c = torch.from_numpy(coord)
    for shifted in (False, True):
        groups = R.group_plan(coord, ends, down, w, shifted)
        i0 = np.concatenate([np.repeat(qr, len(kr)) for qr, kr in groups])
        i1 = np.concatenate([np.tile(kr, len(qr)) for qr, kr in groups])
        order = np.argsort(i0, kind="stable")
        i0, i1 = torch.from_numpy(i0[order]), torch.from_numpy(i1[order])
        rel = R.rel_index(c, i0, i1, w, quant)
        assert rel.min() >= 0 and rel.max() <= rows - 1
        edge = R.edge_attention(q, k, v, c, i0, i1, tq, tk, tv, d ** -0.5, w, quant, rel=rel)
        group = R.group_attention(q, k, v, c, groups, tq, tk, tv, d ** -0.5, w, quant)
        assert (edge - group).abs().max().item() <= 1e-12 * max(1.0, edge.abs().max().item())


def test_rel_index_is_round_half_even_and_ieee_division():
    """The host statement of the kernel's index (one fp32 rounding per operation) against torch's CPU expression, with
    differences whose 1e5 multiple is an exact .5 tie."""
    ties = (np.arange(-4000, 4000, dtype=np.float64) + 0.5) / 1e5
    xi = np.float32(0.25) + np.zeros(len(ties), dtype=np.float32)
    xj = (xi.astype(np.float64) - ties).astype(np.float32)
    rs = np.random.RandomState(0)
    xi = np.concatenate([xi, rs.rand(100000).astype(np.float32) * 0.4])
    xj = np.concatenate([xj, rs.rand(100000).astype(np.float32) * 0.4])
    prod = (xi - xj) * np.float32(100000.0)
    assert (np.abs(prod - np.rint(prod)) == 0.5).sum() > 100        # real ties are in the set
    for w, quant in ((0.2, 0.01), (0.4, 0.05), (1.6, 0.08)):
        host = np.trunc(((np.rint(prod) / np.float32(100000.0) + np.float32(2 * w)) - np.float32(1e-4))
                        / np.float32(quant)).astype(np.int64)
        c = torch.from_numpy(np.stack([xi, xj]).reshape(-1, 1).repeat(3, 1))
        n = len(xi)
        want = R.rel_index(c, torch.arange(n), torch.arange(n) + n, w, quant)[:, 0].long().numpy()
        assert np.array_equal(host, want)


def test_fixture_gaps_and_margins(golden_dir):
    g = np.load(os.path.join(golden_dir, "keypoint_strat_tiny.npz"))
    for k, v in GAPS.items():
        assert abs(float(g["gap_" + k]) - v) <= 1e-3 * v, k
    for i, w in enumerate(TINY_KW["window_size"]):
        margin, same = cell_margins(g[f"coord_layer{i}"], w)
        assert margin >= CELL_MARGIN and same, (i, margin)
        sizes = np.diff(np.concatenate([[0], g[f"offset_layer{i}"]]))
        assert sizes[1] == (11, 3)[i]
        for parity in (0, 1):
            groups = R.group_plan(g[f"coord_layer{i}"], g[f"offset_layer{i}"], g[f"rows_layer{i}_down_idx"], w, bool(parity))
            assert len(groups) == int(g[f"groups_{i}_{parity}"])
            assert sum(len(q) * len(k) for q, k in groups) == int(g[f"edges_{i}_{parity}"])
    idx, margin = R.ball_query(0.05, 34, g["in_coord"], g["in_offset"])
    assert margin >= 1e-5 and (idx[:, -1] >= 0).any() and (idx[:, 1] < 0).any()


def test_names_registered_and_fork_state_dict(golden_dir):
    from pointcept.models import MODELS, build_model
    from ptv3_hip.configs import KEYPOINT_STRAT_CFG
    assert MODELS.get("ST-v1m2") is not None and MODELS.get("KeypointStratifiedTransformer") is not None
    from pointcept.models.stratified_transformer.stratified_transformer_v1m2_refine import (
        StratifiedTransformer, WindowAttention, BasicLayer, TransitionDown, TransitionUp, KPConvSimpleBlock,
        KPConvResBlock)
    from pointcept.models.keypoint_stratified_transformer import KeypointStratifiedTransformer
    tiny = build_model(dict(type="KeypointStratifiedTransformer", **TINY_KW))
    assert isinstance(tiny, KeypointStratifiedTransformer) and isinstance(tiny, StratifiedTransformer)
    assert sum(p.numel() for p in tiny.parameters()) == N_TINY_PARAMS
    attn = tiny.layers[0].blocks[0].attn
    assert isinstance(attn, WindowAttention) and attn.table_rows == 80 and tiny.layers[1].blocks[0].attn.table_rows == 32
    # a fresh model: the query table drawn, the key and value tables zero (the reference draws the query table thrice)
    assert attn.relative_pos_query_table.detach().any() and not attn.relative_pos_key_table.detach().any()
    assert not attn.relative_pos_value_table.detach().any()
    assert isinstance(tiny.layers[0], BasicLayer) and isinstance(tiny.layers[0].down, TransitionDown)
    assert tiny.layers[1].down is None and isinstance(tiny.up[0], TransitionUp)
    assert isinstance(tiny.point_embed[0], KPConvSimpleBlock) and isinstance(tiny.point_embed[1], KPConvResBlock)
    assert not tiny.point_embed[0].kpconv.K_points.requires_grad
    model = build_model(KEYPOINT_STRAT_CFG)
    got = [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]
    ref = open(os.path.join(golden_dir, "state_dict_keypoint_strat_fork.txt")).read().strip().split("\n")
    assert len(ref) == 351 and got == ref
    assert sum(p.numel() for p in model.parameters()) == 18877268
    model.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}, strict=True)
    assert all(b.attn.table_rows == 80 for layer in model.layers for b in layer.blocks)
    seg = build_model(dict(type="ST-v1m2", in_channels=4, num_classes=13, channels=(16, 32, 64), num_heads=(2, 4),
                           depths=(1, 1), window_size=(0.2, 0.4), quant_size=(0.01, 0.05)))
    assert [k for k in seg.state_dict() if k.startswith("classifier.")][:2] == ["classifier.0.weight", "classifier.0.bias"]
    with pytest.raises(KeyError):
        build_model(dict(type="ST-v1m1"))


def test_sample_count_quirks():
    """BasicLayer: int(n * ratio) + 1 per scene.  TransitionDown: the running sum stays a float and IntTensor truncates
    it, so the two differ from the third scene on."""
    from pointcept.models.stratified_transformer.stratified_transformer_v1m2_refine import (
        basic_layer_counts, transition_down_counts)
    sizes = [376, 11, 651]
    assert basic_layer_counts(sizes, 0.25) == [95, 98, 261]
    assert transition_down_counts(sizes, 0.25) == [95, 98, 262]
    assert transition_down_counts([1500, 40, 2600], 0.25) == basic_layer_counts([1500, 40, 2600], 0.25) == [376, 387, 1038]


def test_pointops2_surface():
    import pointops2.pointops as P
    for name in ("furthestsampling", "knnquery", "queryandgroup", "interpolation", "attention_step1_v2",
                 "dot_prod_with_idx_v3", "attention_step2_with_rel_pos_value_v2"):
        assert callable(getattr(P, name))
    for name in ("attention_step1", "attention_step2", "dot_prod_with_idx", "dot_prod_with_idx_v2", "subtraction",
                 "aggregation", "grouping", "interpolation_v2", "Divide2Patch"):
        with pytest.raises(NotImplementedError, match=name):
            getattr(P, name)()
    # the three compositions against the CPU restatement (they are plain torch: they run without a GPU)
    g = torch.Generator().manual_seed(0)
    n, h, d, m = 9, 2, 16, 40
    q, k, v = (torch.randn(n, h, d, generator=g) for _ in range(3))
    i0 = torch.sort(torch.randint(0, n, (m,), generator=g)).values
    i1 = torch.randint(0, n, (m,), generator=g)
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(i0, minlength=n).cumsum(0)])
    tab = torch.randn(8, h, d, 3, generator=g)
    rel = torch.randint(0, 8, (m, 3), generator=g).int()
    assert torch.equal(P.attention_step1_v2(q, k, i1.int(), off.int(), 0), R.attention_step1_v2(q, k, i1, off, 0))
    assert torch.equal(P.dot_prod_with_idx_v3(q, off.int(), 0, k, i1.int(), tab, tab, rel),
                       R.dot_prod_with_idx_v3(q, off, 0, k, i1, tab, tab, rel))
    a = torch.rand(m, h, generator=g)
    assert torch.equal(P.attention_step2_with_rel_pos_value_v2(a, v, off.int(), 0, i1.int(), tab, rel),
                       R.attention_step2_with_rel_pos_value_v2(a, v, off, 0, i1, tab, rel))


def test_entries_refuse_bad_arguments_without_a_gpu():
    """Argument checks come before any pointer is touched or kernel launched: error code 1 and a message."""
    from ptv3_hip.lib import lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    assert lib.ptv3_strat_attn_capable(6, 16, 80) == 1 and lib.ptv3_strat_attn_capable(1, 16, 8) == 1
    for heads, hd, rows in ((6, 8, 80), (6, 32, 80), (6, 16, 81), (6, 16, 0), (0, 16, 80), (70000, 16, 80)):
        assert lib.ptv3_strat_attn_capable(heads, hd, rows) == 0
        rc = lib.ptv3_strat_attn_fwd(p, p, p, 3 * heads * hd, p, p, p, p, p, p, p, p, 1, heads, hd, rows, 0.25, 0.2, 0.01,
                                     p, None)
        assert rc == 1 and b"head_dim 16, 1 .. 80 table rows" in lib.ptv3_last_error()
    attn = lambda **kw: lib.ptv3_strat_attn_fwd(   # noqa: E731
        kw.get("q", p), p, p, kw.get("ld", 288), p, p, p, p, p, p, p, p, kw.get("g", 1), 6, 16, 80, 0.25,
        kw.get("w", 0.2), kw.get("quant", 0.01), p, None)
    assert attn(q=None) == 1 and b"a NULL pointer" in lib.ptv3_last_error()
    assert attn(ld=95) == 1 and b"row stride" in lib.ptv3_last_error()
    assert attn(g=-1) == 1 and b"groups" in lib.ptv3_last_error()
    assert attn(quant=0.0) == 1 and b"quant=0" in lib.ptv3_last_error()
    assert attn(g=0) == 0                                             # nothing to do: no launch
    assert lib.ptv3_ball_query(p, p, 1, 0, 0.05, 34, p, None) == 0
    assert lib.ptv3_ball_query(p, p, 1, 4, 0.05, 0, p, None) == 1 and b"max_neighbor=0" in lib.ptv3_last_error()
    assert lib.ptv3_ball_query(None, p, 1, 4, 0.05, 34, p, None) == 1 and b"a NULL pointer" in lib.ptv3_last_error()
    assert lib.ptv3_strat_cell_keys(p, 0, p, 1, p, 0.2, 0, p, p, p, None) == 1 and b"n=0 rows" in lib.ptv3_last_error()
    assert lib.ptv3_strat_cell_keys(p, 4, p, 0, p, 0.2, 0, p, p, p, None) == 1 and b"0 scenes" in lib.ptv3_last_error()
    assert lib.ptv3_strat_rel_index(p, p, p, 0, 0.2, 0.01, 80, p, None) == 0
    assert lib.ptv3_strat_rel_index(p, p, p, 4, 0.2, 0.0, 80, p, None) == 1 and b"quant=0" in lib.ptv3_last_error()


def test_model_refuses_without_device_work():
    from pointcept.models import build_model
    with pytest.raises(NotImplementedError, match="rel_query = rel_key = rel_value = True"):
        build_model(dict(type="KeypointStratifiedTransformer", **dict(TINY_KW, rel_value=False)))
    model = build_model(dict(type="KeypointStratifiedTransformer", **TINY_KW))
    data = dict(coord=torch.rand(30, 3), feat=torch.rand(30, 4), offset=torch.tensor([20, 20, 30]))
    with pytest.raises(ValueError, match="non-empty scenes"):
        model.eval()(dict(data))
