"""PointGroup's evaluation tail on the GPU (csrc/pointgroup.hip) against the numpy restatements of
tests/pointgroup_ref.py: the ball query (lists and start_len exact), the on-device clustering against the directed
breadth-first search, the proposal kernel, the fused head and bias losses against float64, and PG-v1m1 / PG-v1m2
against the reference's outputs on a stand-in backbone
(tests/golden/pointgroup_tiny.npz; pointgroup_ops parity UNPINNED: the fixture's clustering is a restatement)."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import pointgroup_ref as R

pytestmark = pytest.mark.gpu

RADIUS = 1.5
FP32_TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _quarter_grid(n, seed, lo=-6.0, hi=6.0):
    """coordinates that are multiples of 1/4: every d2 is exact in fp32 and d2 == radius^2 = 2.25 occurs"""
    g = np.random.default_rng(seed)
    return (g.integers(int(lo * 4), int(hi * 4), size=(n, 3)) / 4.0).astype(np.float32)


def _batch(sizes):
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int32), offsets


def _capped_blob():
    """4001 points: a blob of 1300 inside one ball (every blob point has more than 1000 neighbours), a probe at index
    1300 with exactly 1000 neighbours (itself and 999 copies of one position 0.25 away), a probe at 1301 with exactly
    1001, and isolated filler 4 apart."""
    g = np.random.default_rng(7)
    blob = g.uniform(-0.4, 0.4, size=(1300, 3)).astype(np.float32)
    far = np.zeros((702, 3), dtype=np.float32)
    far[:, 0] = 100.0 + 4.0 * np.arange(702)          # isolated filler, 4 apart
    # two probes far from the blob, each with a private cloud of neighbours of exact count
    far[0] = (50.0, 0.0, 0.0)
    far[1] = (50.0, 40.0, 0.0)
    a = np.tile(np.array([[50.25, 0.0, 0.0]], dtype=np.float32), (999, 1))
    b = np.tile(np.array([[50.25, 40.0, 0.0]], dtype=np.float32), (1000, 1))
    xyz = np.concatenate([blob, far[:2], a, b, far[2:]]).astype(np.float32)
    return xyz


BQ_CASES = {
    "n1": lambda: (_quarter_grid(1, 1), [1]),
    "n257": lambda: (_quarter_grid(257, 2), [257]),
    "two_scenes": lambda: (_quarter_grid(2100, 3), [1200, 900]),
    "negative": lambda: (_quarter_grid(600, 4, lo=-6.0, hi=-0.25), [600]),
    "capped": lambda: (_capped_blob(), None),
}


def _bq_case(name):
    xyz, sizes = BQ_CASES[name]()
    sizes = [xyz.shape[0]] if sizes is None else sizes
    batch, offsets = _batch(sizes)
    return xyz, batch, offsets


_REF = {}


def _bq_ref(name):
    """the reference lists of a case, computed once"""
    if name not in _REF:
        xyz, batch, offsets = _bq_case(name)
        _REF[name] = (xyz, batch, offsets) + R.ball_query(xyz, batch, offsets, RADIUS)
    return _REF[name]


# ------------------------------------------------------------------------------------------------
# 1. ball query
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BQ_CASES))
def test_ballquery_lists_exact(dev, name):
    """idx and start_len equal the brute restatement: strict d2 < r^2 (d2 == r^2 occurs on the quarter grid), no list
    crosses a scene, ascending order, the first 1000 of a longer list, start = scan of the counts by point index."""
    import pointgroup_ops
    xyz, batch, offsets, idx_ref, sl_ref = _bq_ref(name)
    if name != "capped" and xyz.shape[0] > 1:
        d = xyz[:, None, :] - xyz[None, :, :]
        assert ((d * d).sum(-1) == np.float32(RADIUS * RADIUS)).any()
    if name == "capped":
        true = R.neighbour_counts(xyz, batch, offsets, RADIUS)
        assert (true[:1300] > 1000).all() and true[1300] == 1000 and true[1301] == 1001
        assert sl_ref[1300, 1] == 1000 and sl_ref[1301, 1] == 1000
    t = [torch.from_numpy(a).to(dev) for a in (xyz, batch, offsets)]
    idx, start_len = pointgroup_ops.ballquery_batch_p(t[0], t[1], t[2], RADIUS, 300)
    assert idx.dtype == torch.int32 and start_len.dtype == torch.int32 and idx.is_cuda and start_len.is_cuda
    assert np.array_equal(start_len.cpu().numpy(), sl_ref)
    assert np.array_equal(idx.cpu().numpy(), idx_ref)
    idx2, start_len2 = pointgroup_ops.ballquery_batch_p(t[0], t[1], t[2], RADIUS, 1)
    assert torch.equal(idx, idx2) and torch.equal(start_len, start_len2)


# ------------------------------------------------------------------------------------------------
# 2. clustering
# ------------------------------------------------------------------------------------------------
def _chain():
    xyz = np.zeros((4000, 3), dtype=np.float32)
    xyz[:, 0] = 1.25 * np.arange(4000) - 2500.0
    g = np.random.default_rng(11)
    return xyz[g.permutation(4000)], np.zeros(4000, dtype=np.int32), [4000]


def _interleaved():
    ax = np.arange(12, dtype=np.float32)
    xyz = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    label = ((xyz.sum(1).astype(np.int64)) % 2 + 2).astype(np.int32)     # checkerboard: same-label lattice neighbours
    return xyz, label, [xyz.shape[0]]                                    # are sqrt(2) apart, within 1.5


def _overlaid():
    g = np.random.default_rng(12)
    a = (g.integers(-16, 16, size=(700, 3)) / 4.0).astype(np.float32)
    return np.concatenate([a, a[:500]]), (np.arange(1200) % 3).astype(np.int32), [700, 500]


def _sizes_at_threshold():
    """blobs of 49, 50, 51, 100 and 101 points, far apart (min_points = 50: the first is dropped)"""
    parts, g = [], np.random.default_rng(13)
    for k, m in enumerate([49, 50, 51, 100, 101]):
        parts.append(g.uniform(-0.3, 0.3, size=(m, 3)).astype(np.float32) + np.float32(10.0 * k))
    xyz = np.concatenate(parts)
    perm = g.permutation(xyz.shape[0])
    return xyz[perm], np.full(xyz.shape[0], 5, dtype=np.int32), [xyz.shape[0]]


def _isolated():
    xyz = np.zeros((300, 3), dtype=np.float32)
    xyz[:, 1] = 2.0 * np.arange(300)
    return xyz, np.zeros(300, dtype=np.int32), [300]


CL_CASES = {"chain": _chain, "interleaved": _interleaved, "overlaid": _overlaid, "threshold": _sizes_at_threshold,
            "isolated": _isolated}


def _cl_ref(name, min_points):
    key = ("cl", name, min_points)
    if key not in _REF:
        xyz, label, sizes = CL_CASES[name]()
        offsets = _batch(sizes)[1]
        idxs, offs = R.cluster(xyz, label, offsets, RADIUS, min_points)
        _REF[key] = xyz, label, offsets, R.sort_members(idxs, offs), offs
    return _REF[key]


@pytest.mark.parametrize("min_points", [1, 50])
@pytest.mark.parametrize("name", list(CL_CASES))
def test_cluster_equals_directed_bfs(dev, name, min_points):
    """Without truncation the lists are symmetric, so the union's components are the search's: cluster order exact (by
    smallest member), members compared as sorted sets, the >= min_points boundary at 49 / 50, labels and scenes never
    merge; two runs bitwise equal."""
    from ptv3_hip import ops
    xyz, label, offsets, idxs_ref, offs_ref = _cl_ref(name, min_points)
    if name == "threshold":
        assert sorted(np.diff(offs_ref).tolist()) == ([50, 51, 100, 101] if min_points == 50 else [49, 50, 51, 100, 101])
    if name == "chain":
        assert offs_ref.tolist() == [0, 4000]
    t = [torch.from_numpy(a).to(dev) for a in (xyz, label, offsets)]
    got = ops.pg_cluster(t[0], t[1], t[2], RADIUS, min_points, 100)
    assert got is not None
    idxs, offs, large = got
    assert idxs.dtype == torch.int32 and offs.dtype == torch.int32
    assert np.array_equal(offs.cpu().numpy(), offs_ref)
    assert np.array_equal(idxs.cpu().numpy(), idxs_ref)
    assert large == int((np.diff(offs_ref) > 100).sum())
    again = ops.pg_cluster(t[0], t[1], t[2], RADIUS, min_points, 100)
    assert torch.equal(again[0], idxs) and torch.equal(again[1], offs) and again[2] == large


def test_cluster_cap_status_and_list_path(dev):
    """More than 1000 neighbours: the fast path reports it (None from the wrapper) and the list path - ball query, copy,
    host search - equals the directed search of the restatement."""
    from ptv3_hip import ops
    import pointgroup_ops
    xyz, batch, offsets, idx_ref, sl_ref = _bq_ref("capped")
    label = np.zeros(xyz.shape[0], dtype=np.int32)
    t = [torch.from_numpy(a).to(dev) for a in (xyz, label, offsets, batch)]
    assert ops.pg_cluster(t[0], t[1], t[2], RADIUS, 50, 100) is None
    idx, start_len = pointgroup_ops.ballquery_batch_p(t[0], t[3], t[2], RADIUS, 300)
    idxs, offs = pointgroup_ops.bfs_cluster(t[1].cpu(), idx.cpu(), start_len.cpu(), 50)
    ref_idxs, ref_offs = R.bfs_cluster(label, idx_ref, sl_ref, 50)
    assert np.array_equal(offs.numpy(), ref_offs)
    assert np.array_equal(idxs.numpy(), R.sort_members(ref_idxs, ref_offs))


# ------------------------------------------------------------------------------------------------
# 3. proposals
# ------------------------------------------------------------------------------------------------
def _proposal_case(sizes, n_rows, classes, seed):
    """clusters of the given sizes over a random subset of n_rows rows (through a row map), random probabilities"""
    g = np.random.default_rng(seed)
    total = int(sum(sizes))
    row_map = np.sort(g.choice(n_rows, size=total + 17, replace=False)).astype(np.int64)
    members = g.permutation(total + 17)[:total]
    idxs, offs, at = [], [0], 0
    for c, m in enumerate(sizes):
        idxs.extend((c, int(v)) for v in np.sort(members[at:at + m]))
        at += m
        offs.append(at)
    prob = g.random((n_rows, classes), dtype=np.float32)
    prob /= prob.sum(1, keepdims=True)
    seg = prob.argmax(1).astype(np.int64)
    return (np.array(idxs, dtype=np.int32).reshape(-1, 2), np.array(offs, dtype=np.int32), prob.astype(np.float32), seg,
            row_map)


@pytest.mark.parametrize("sizes", [[100, 101, 50, 1300, 257, 102], [100, 99, 1], []], ids=["mixed", "none_kept", "empty"])
def test_proposals_against_float64(dev, sizes):
    """Classes and masks exact, > propose_points strict (100 out, 101 in), scores within 2 m 2^-24 of float64 (the
    worst case of an m-term fp32 sum of values in [0, 1], m the largest cluster), zero proposals well-formed."""
    from ptv3_hip import ops
    n_rows, classes = 4099, 20
    idxs, offs, prob, seg, row_map = _proposal_case(sizes, n_rows, classes, 21)
    cls_ref, score_ref, members = R.proposals(idxs, offs, prob, seg, 100, row_map)
    p = len(cls_ref)
    assert p == sum(1 for m in sizes if m > 100)
    t = [torch.from_numpy(a).to(dev) for a in (idxs, offs, prob, seg, row_map)]
    got_cls, got_score, got_mask = ops.pg_proposals(t[0], t[1], t[2], t[3], 100, p, row_map=t[4])
    assert got_cls.dtype == torch.int64 and got_score.dtype == torch.float32 and got_mask.dtype == torch.int32
    assert tuple(got_mask.shape) == (p, n_rows) and tuple(got_cls.shape) == (p,) and tuple(got_score.shape) == (p,)
    assert np.array_equal(got_cls.cpu().numpy(), cls_ref)
    mask_ref = np.zeros((p, n_rows), dtype=np.int32)
    for k, rows in enumerate(members):
        mask_ref[k, rows] = 1
    assert np.array_equal(got_mask.cpu().numpy(), mask_ref)
    if p:
        m = max(sizes)
        err = np.abs(got_score.cpu().numpy().astype(np.float64) - score_ref).max()
        print("score error", err, "bound", 2 * m * 2.0 ** -24)
        assert err <= 2 * m * 2.0 ** -24
        again = ops.pg_proposals(t[0], t[1], t[2], t[3], 100, p, row_map=t[4])
        assert torch.equal(again[1].view(torch.int32), got_score.view(torch.int32))


# ------------------------------------------------------------------------------------------------
# 5. the models against the reference's own outputs
# ------------------------------------------------------------------------------------------------
IGNORE = (-1, 0, 1)
EVAL_KEYS = ["bias_cosine_loss", "bias_l1_loss", "loss", "pred_classes", "pred_masks", "pred_scores", "seg_loss"]


def _register_stand_in():
    from pointcept.models import MODELS
    from pointcept.models.utils.hip_layers import Linear
    if MODELS.get("PGStandInBackbone") is None:
        @MODELS.register_module("PGStandInBackbone")
        class PGStandInBackbone(nn.Module):
            """The generator's stand-in backbone: Linear(6, 64) on data_dict["feat"]."""

            def __init__(self):
                super().__init__()
                self.lin = Linear(6, 64)

            def forward(self, data_dict):
                return self.lin(data_dict["feat"].contiguous())


def _golden(golden_dir, dev, version):
    from pointcept.models import build_model
    _register_stand_in()
    g = np.load(os.path.join(golden_dir, "pointgroup_tiny.npz"))
    extra = {} if version == "v1m1" else dict(criteria=[dict(type="CrossEntropyLoss", loss_weight=0.7, ignore_index=-1)])
    model = build_model(dict(type="PG-" + version, backbone=dict(type="PGStandInBackbone"), backbone_out_channels=64,
                             semantic_num_classes=20, semantic_ignore_index=-1, segment_ignore_index=IGNORE,
                             instance_ignore_index=-1, cluster_thresh=1.5, cluster_closed_points=300,
                             cluster_propose_points=100, cluster_min_points=50, voxel_size=0.02, **extra))
    model.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd_")}, strict=True)
    data = {k[3:]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("in_")}
    return g, model.to(dev), data


def _check_eval(out, g, n):
    assert sorted(out.keys()) == EVAL_KEYS
    for k in ("pred_classes", "pred_masks", "pred_scores"):
        assert not out[k].is_cuda
    assert out["pred_masks"].dtype == torch.int32 and out["pred_classes"].dtype == torch.int64
    assert out["pred_scores"].dtype == torch.float32
    p = g["pred_classes"].shape[0]
    assert tuple(out["pred_masks"].shape) == (p, n)
    assert np.array_equal(out["pred_classes"].numpy(), g["pred_classes"])
    masks = out["pred_masks"].numpy()
    assert set(np.unique(masks).tolist()) <= {0, 1}
    rows = [np.nonzero(m)[0] for m in masks]
    assert np.array_equal(np.concatenate(rows), g["pred_mask_rows"])
    assert np.array_equal(np.concatenate([[0], np.cumsum([len(r) for r in rows])]), g["pred_mask_offset"])
    m = max(len(r) for r in rows)
    err = np.abs(out["pred_scores"].numpy().astype(np.float64) - g["pred_scores"].astype(np.float64)).max()
    print("score error", err, "bound", 2 * m * 2.0 ** -24)
    assert err <= 2 * m * 2.0 ** -24


@pytest.mark.parametrize("version", ["v1m1", "v1m2"])
def test_model_eval_vs_reference_golden(dev, golden_dir, version):
    """Proposals (dense masks) and classes exact, scores within the bound of test 3, on the device clustering and on
    the list path; the clusters themselves against the fixture's lists; the eval losses within FP32_TOL relative."""
    g, model, data = _golden(golden_dir, dev, version)
    model.eval()
    n = data["coord"].shape[0]
    with torch.no_grad():
        out = model(dict(data))
    _check_eval(out, g, n)
    want = {k: float(g["eval_" + k]) for k in ("loss", "seg_loss", "bias_l1_loss", "bias_cosine_loss")}
    if version == "v1m2":
        want["seg_loss"] = float(g["eval_v1m2_seg_loss"])
        want["loss"] = want["seg_loss"] + want["bias_l1_loss"] + want["bias_cosine_loss"]
    for k, v in want.items():
        assert abs(out[k].item() - v) <= FP32_TOL * abs(v), (k, out[k].item(), v)
    with torch.no_grad():
        listed = model.set_fused(False)(dict(data))
    _check_eval(listed, g, n)
    assert torch.equal(listed["pred_masks"], out["pred_masks"])
    assert torch.equal(listed["pred_scores"].view(torch.int32), out["pred_scores"].view(torch.int32))
    # the cluster lists (every cluster of at least min_points, rows of the batch)
    model.set_fused(True)
    with torch.no_grad():
        feat = model.backbone(dict(data))
        center = ((data["coord"] + model.bias_head(feat)) / 0.02).contiguous()
        seg = model.seg_head(feat).argmax(1)
    keep = ~torch.isin(seg, torch.tensor(IGNORE, device=dev))
    idxs, offs, rows, large = model.cluster(center, seg, keep, data["offset"])
    idxs = idxs.cpu().numpy().copy()
    idxs[:, 1] = rows.cpu().numpy()[idxs[:, 1]]
    assert np.array_equal(offs.cpu().numpy(), g["proposals_offset"]) and np.array_equal(idxs, g["proposals_idx"])
    assert large == g["pred_classes"].shape[0]
    if version == "v1m2":
        with torch.no_grad():
            point = model(dict(data), return_point=True)
        assert sorted(point.keys()) == ["point"] and tuple(point["point"].shape) == (n, 64)


@pytest.mark.parametrize("version", ["v1m1", "v1m2"])
def test_model_train_step_vs_reference_golden(dev, golden_dir, version):
    """One training step: the four losses within FP32_TOL relative, every parameter gradient as
    test_vote_model_train_step_vs_reference_golden compares its golden, the BatchNorm running statistics within
    FP32_TOL; nothing but the four losses is returned."""
    g, model, data = _golden(golden_dir, dev, version)
    model.train()
    out = model(dict(data))
    out["loss"].backward()
    keys = ["loss", "seg_loss", "bias_l1_loss", "bias_cosine_loss"]
    assert sorted(out.keys()) == sorted(keys)
    for k in keys:
        want = float(g[f"{version}_{k}"])
        print(k, out[k].item(), want)
        assert abs(out[k].item() - want) <= FP32_TOL * abs(want), k
    pre = f"{version}_grad_"
    grads = {k[len(pre):]: torch.from_numpy(g[k].astype(np.float32) * g[f"{version}_gmax_" + k[len(pre):]])
             for k in g.files if k.startswith(pre)}
    gmax = max(float(g[k]) for k in g.files if k.startswith(f"{version}_gmax_"))
    # a Linear bias in front of a batch-statistic BatchNorm has an exact gradient of zero: rounding noise on both sides
    noise = ("bias_head.0.bias",)
    assert model.bias_head[0].bias.grad.abs().max().item() <= 1e-4 * grads["bias_head.0.weight"].abs().max().item()
    assert set(grads) == {n for n, _ in model.named_parameters()}
    worst = max(((n, (p.grad.float().cpu() - grads[n]).abs().max().item()
                  / max(grads[n].abs().max().item(), 1e-3 * gmax)) for n, p in model.named_parameters()
                 if n not in noise), key=lambda t: t[1])
    print("worst gradient", worst)
    assert worst[1] < 2e-3, worst
    for n, b in model.named_buffers():
        if "running" in n:
            ref = torch.from_numpy(g[f"{version}_buf_" + n])
            assert (b.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6) < FP32_TOL, n


def test_model_eval_with_every_point_ignored(dev, golden_dir):
    """Every point predicted as an ignored class: the empty results the reference's tail is heading for (the
    reference itself raises on this branch, point_group_v1m1_base.py:120 / :149)."""
    g, model, data = _golden(golden_dir, dev, "v1m1")
    with torch.no_grad():
        model.seg_head.weight.zero_()
        model.seg_head.bias.zero_()
        model.seg_head.bias[1] = 5.0
    model.eval()
    with torch.no_grad():
        out = model(dict(data))
    assert sorted(out.keys()) == EVAL_KEYS
    assert tuple(out["pred_masks"].shape) == (0, data["coord"].shape[0]) and out["pred_masks"].dtype == torch.int32
    assert tuple(out["pred_scores"].shape) == (0,) and tuple(out["pred_classes"].shape) == (0,)
    assert out["pred_scores"].dtype == torch.float32 and out["pred_classes"].dtype == torch.float32


def test_scannet_ptv3_config_eval_is_well_formed(dev):
    """PG_PTV3_SCANNET_CFG at a reduced depth on 2 x 3000 points: a shape check (the backbone is pinned elsewhere)."""
    from pointcept.models import build_model
    from ptv3_hip.configs import PG_PTV3_SCANNET_CFG
    import ptv3_scenes as S
    cfg = dict(PG_PTV3_SCANNET_CFG)
    cfg["backbone"] = dict(cfg["backbone"], enc_depths=(1, 1, 1, 1, 1), dec_depths=(1, 1, 1, 1),
                           enc_patch_size=(128,) * 5, dec_patch_size=(128,) * 4)
    torch.manual_seed(0)
    model = build_model(cfg).to(dev).eval()
    data = S.make_batch([3000, 3000], in_channels=6, extent=96, seed=1)
    data = {k: v.to(dev) for k, v in data.items()}
    data["instance_centroid"] = data["coord"].clone()
    n = data["coord"].shape[0]
    with torch.no_grad():
        out = model(data)
    assert sorted(out.keys()) == ["pred_classes", "pred_masks", "pred_scores"]
    p = out["pred_masks"].shape[0]
    assert tuple(out["pred_masks"].shape) == (p, n) and out["pred_masks"].dtype == torch.int32
    assert out["pred_scores"].shape[0] == p and out["pred_classes"].shape[0] == p
    if p:
        assert (out["pred_masks"].sum(1) > 100).all()
        assert ((out["pred_scores"] > 0) & (out["pred_scores"] <= 1)).all()
        assert not np.isin(out["pred_classes"].numpy(), IGNORE).any()


# ------------------------------------------------------------------------------------------------
# 1b. d2 is evaluated without contraction; 2b. the model's own cap fallback
# ------------------------------------------------------------------------------------------------
def _contraction_pairs(want=12):
    """Pairs (origin, x) whose d2 = x0*x0 + x1*x1 + x2*x2 lands on different sides of r^2 = 2.25 when every operation is
    rounded (the reference's text) and when the sums are fused multiply-adds, fma(x2, x2, fma(x1, x1, x0*x0)); both
    directions occur.  The fused form is emulated in float64, where each product of two float32 is exact."""
    g = np.random.default_rng(31)
    picked = {True: [], False: []}
    r2 = np.float32(2.25)
    while min(len(v) for v in picked.values()) < want // 2:
        x = g.uniform(0.3, 1.2, size=(200000, 3)).astype(np.float32)
        rest = 2.25 - x[:, 0].astype(np.float64) ** 2 - x[:, 1].astype(np.float64) ** 2
        x = x[rest > 0.01]
        x[:, 2] = np.sqrt(rest[rest > 0.01]).astype(np.float32)
        x[:, 2] = np.nextafter(x[:, 2], np.float32(2.0) * g.integers(0, 2, size=x.shape[0]).astype(np.float32))
        sq = x * x
        plain = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
        x64 = x.astype(np.float64)
        fused = (x64[:, 2] * x64[:, 2] + (x64[:, 1] * x64[:, 1] + sq[:, 0].astype(np.float64)).astype(np.float32)
                 .astype(np.float64)).astype(np.float32)
        for inside in (True, False):
            rows = np.nonzero(((plain < r2) == inside) & ((fused < r2) != inside))[0]
            picked[inside].extend(x[rows[:want // 2 - len(picked[inside])]])
    return np.array(picked[True] + picked[False], dtype=np.float32), want // 2


def test_ballquery_d2_has_one_rounding_per_operation(dev):
    """Scenes of two points, the origin and x: with every operation rounded half of the pairs are neighbours and half
    are not, with fused multiply-adds it is the other way round.  The lists equal the restatement's (numpy float32, no
    fma), which pins `#pragma clang fp contract(off)` in a library built with -ffp-contract=on."""
    import pointgroup_ops
    from ptv3_hip import ops
    x, half = _contraction_pairs()
    xyz = np.zeros((2 * x.shape[0], 3), dtype=np.float32)
    xyz[1::2] = x
    batch, offsets = _batch([2] * x.shape[0])
    idx_ref, sl_ref = R.ball_query(xyz, batch, offsets, RADIUS)
    assert sl_ref[:2 * half, 1].tolist() == [2] * (2 * half) and sl_ref[2 * half:, 1].tolist() == [1] * (2 * half)
    t = [torch.from_numpy(a).to(dev) for a in (xyz, batch, offsets)]
    idx, start_len = pointgroup_ops.ballquery_batch_p(t[0], t[1], t[2], RADIUS, 300)
    assert np.array_equal(start_len.cpu().numpy(), sl_ref) and np.array_equal(idx.cpu().numpy(), idx_ref)
    label = torch.zeros(xyz.shape[0], dtype=torch.int32, device=dev)
    idxs, offs, _ = ops.pg_cluster(t[0], label, t[2], RADIUS, 2, 100)     # the same d2 in the clustering walk
    assert offs.cpu().tolist() == list(range(0, 2 * half + 1, 2))
    assert idxs[:, 1].cpu().tolist() == list(range(2 * half))


def test_model_cluster_falls_back_on_the_cap(dev, golden_dir):
    """PointGroupBase.cluster on the 1300-point blob: the device clustering reports the cap, the model takes the list
    path by itself, without raising, and returns the directed search's clusters (one cluster of the blob's first 1000
    points, which no undirected clustering gives)."""
    from ptv3_hip import ops
    _, model, _ = _golden(golden_dir, dev, "v1m1")
    xyz, batch, offsets, idx_ref, sl_ref = _bq_ref("capped")
    n = xyz.shape[0]
    label = np.full(n, 2, dtype=np.int32)
    center = torch.from_numpy(xyz).to(dev)
    seg = torch.full((n,), 2, dtype=torch.int64, device=dev)
    assert ops.pg_cluster(center, seg.int(), torch.from_numpy(offsets).to(dev), RADIUS, 50, 100) is None
    idxs, offs, rows, large = model.cluster(center, seg, torch.ones(n, dtype=torch.bool, device=dev),
                                            torch.tensor([n], device=dev))
    ref_idxs, ref_offs = R.bfs_cluster(label, idx_ref, sl_ref, 50)
    assert np.array_equal(offs.cpu().numpy(), ref_offs)
    assert np.array_equal(idxs.cpu().numpy(), R.sort_members(ref_idxs, ref_offs))
    assert ref_offs[1] == 1000 and large == int((np.diff(ref_offs) > 100).sum()) and rows.shape[0] == n


# ------------------------------------------------------------------------------------------------
# 4. the fused head and the bias losses
# ------------------------------------------------------------------------------------------------
ULP = 2.0 ** -23


def _check(name, got, ref64, torch32, floor_scale=None):
    """the rule of tests/test_hip_cls_head.py: the error against float64 is at most 4x the error of the same function
    composed from torch float32 ops on the device, with a floor of 8 float32 ulps of the tensor's largest entry; prints
    each figure before it asserts"""
    ref64 = ref64.double().cpu()
    err_k = (got.double().cpu() - ref64).abs().max().item() if ref64.numel() else 0.0
    err_t = (torch32.double().cpu() - ref64).abs().max().item() if ref64.numel() else 0.0
    top = (ref64.abs().max().item() if ref64.numel() else 0.0) if floor_scale is None else floor_scale
    bound = max(4.0 * err_t, 8.0 * ULP * top)
    print(f"{name}: kernel {err_k:.3e} torch-fp32 {err_t:.3e} max|ref| {top:.3e} bound {bound:.3e}")
    assert err_k <= bound, (name, err_k, err_t, top)


def _head_params(c, k, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(w1=r(c, c) / c ** 0.5, b1=r(c) * 0.1, bn_w=torch.rand(c, generator=g) + 0.5, bn_b=r(c) * 0.1,
                bn_mean=r(c) * 0.1, bn_var=torch.rand(c, generator=g) + 0.5, w2=r(3, c) / c ** 0.5, b2=r(3) * 0.1,
                ws=r(k, c) * (4.0 / c ** 0.5), bs=r(k) * 0.1)


def _head_composed(feat, coord, p, voxel, eps=1e-3):
    h = torch.nn.functional.linear(feat, p["w1"], p["b1"])
    h = torch.relu((h - p["bn_mean"]) / torch.sqrt(p["bn_var"] + eps) * p["bn_w"] + p["bn_b"])
    bias = torch.nn.functional.linear(h, p["w2"], p["b2"])
    logit = torch.nn.functional.linear(feat, p["ws"], p["bs"])
    return bias, logit, torch.softmax(logit, 1), (coord + bias) / voxel


@pytest.mark.parametrize("k", [2, 20, 200])
@pytest.mark.parametrize("c", [64, 96])
@pytest.mark.parametrize("n", [1, 255, 4099])
def test_head_eval_against_float64(dev, n, c, k):
    """bias_pred, logit, softmax and centre under the rule of _check; argmax and keep flag exact on every row whose
    top-two logit gap exceeds 1e-3 in float64 (at least nine rows in ten)."""
    from ptv3_hip import ops
    p = _head_params(c, k, 100 * c + k)
    g = torch.Generator().manual_seed(n)
    feat, coord = torch.randn(n, c, generator=g), torch.rand(n, 3, generator=g) * 4.0
    voxel = 0.02
    ref = _head_composed(feat.double(), coord.double(), {a: b.double() for a, b in p.items()}, voxel)
    pd = {a: b.to(dev) for a, b in p.items()}
    t32 = _head_composed(feat.to(dev), coord.to(dev), pd, voxel)
    got = ops.pg_head_eval(feat.to(dev), coord.to(dev), pd["w1"], pd["b1"], pd["bn_w"], pd["bn_b"], pd["bn_mean"],
                           pd["bn_var"], 1e-3, pd["w2"], pd["b2"], pd["ws"], pd["bs"], voxel, IGNORE)
    for name, a, b, d in zip(("bias_pred", "logit", "prob", "center"), (got[0], got[1], got[2], got[4]), ref, t32):
        _check(name, a, b, d)
    top = ref[1].topk(2, dim=1).values if k > 1 else None
    sure = (top[:, 0] - top[:, 1]) > 1e-3
    assert sure.double().mean().item() >= 0.9 or n == 1
    arg = ref[1].argmax(1)
    assert got[3].dtype == torch.int64 and got[5].dtype == torch.bool
    assert torch.equal(got[3].cpu()[sure], arg[sure])
    assert torch.equal(got[5].cpu()[sure], ~torch.isin(arg, torch.tensor(IGNORE))[sure])
    again = ops.pg_head_eval(feat.to(dev), coord.to(dev), pd["w1"], pd["b1"], pd["bn_w"], pd["bn_b"], pd["bn_mean"],
                             pd["bn_var"], 1e-3, pd["w2"], pd["b2"], pd["ws"], pd["bs"], voxel, IGNORE)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def _bias_losses(bias_pred, coord, centroid, instance, ignore=-1):
    """point_group_v1m1_base.py:75-89 composed in torch"""
    mask = (instance != ignore).to(bias_pred.dtype)
    gt = centroid - coord
    l1 = torch.sum(torch.sum(torch.abs(bias_pred - gt), dim=-1) * mask) / (torch.sum(mask) + 1e-8)
    pn = bias_pred / (torch.norm(bias_pred, p=2, dim=1, keepdim=True) + 1e-8)
    gn = gt / (torch.norm(gt, p=2, dim=1, keepdim=True) + 1e-8)
    return l1, torch.sum(-(pn * gn).sum(-1) * mask) / (torch.sum(mask) + 1e-8)


@pytest.mark.parametrize("masked", ["some", "all"])
@pytest.mark.parametrize("n", [1, 255, 4099])
def test_bias_loss_forward_and_backward(dev, n, masked):
    """Both losses and d bias_pred against float64 autograd of the torch composition under the rule of _check (the
    composition in float32 on the device is the yardstick).  Row 0 has bias_pred == 0: its gradient is the 1 / eps term
    alone, as torch.norm's zero subgradient leaves it, and is compared on its own so that it does not set the floor of the
    other rows.  With every point masked both losses and the gradient are exactly 0."""
    from ptv3_hip import autograd as A
    g = torch.Generator().manual_seed(7 * n)
    bias, coord = torch.randn(n, 3, generator=g) * 0.05, torch.rand(n, 3, generator=g)
    centroid = coord + torch.randn(n, 3, generator=g) * 0.05
    bias[0] = 0.0
    instance = torch.randint(-1, 5, (n,), generator=g)
    instance[0] = 0
    if masked == "all":
        instance[:] = -1
    wl, wc = 0.7, 1.3

    def run(b, fn, *rest):
        b = b.clone().requires_grad_(True)
        l1, cs = fn(b, *rest)
        (wl * l1 + wc * cs).backward()
        return l1.detach(), cs.detach(), b.grad

    ref = run(bias.double(), _bias_losses, coord.double(), centroid.double(), instance)
    rest = (coord.to(dev), centroid.to(dev), instance.to(dev))
    t32 = run(bias.to(dev), _bias_losses, *rest)
    got = run(bias.to(dev), A.pg_bias_loss, *rest)
    if masked == "all":
        assert got[0].item() == 0.0 and got[1].item() == 0.0 and torch.count_nonzero(got[2]).item() == 0
        return
    _check("bias_l1_loss", got[0], ref[0], t32[0])
    _check("bias_cosine_loss", got[1], ref[1], t32[1])
    _check("d bias_pred, row 0 (bias_pred == 0)", got[2][:1], ref[2][:1], t32[2][:1])
    _check("d bias_pred, other rows", got[2][1:], ref[2][1:], t32[2][1:])
