"""Build-container-only: run the reference's KeypointStratifiedTransformer (pointcept/models/
keypoint_stratified_transformer.py over stratified_transformer/stratified_transformer_v1m2_refine.py, both imported in
place) on a seeded three-scene batch and store, in keypoint_strat_tiny.npz, its eval `pred` and loss, the rows every
farthest point sampling call returned, the number of attention groups of every (layer, parity), strided feature taps of
every stage and one training step (loss, curves, every parameter gradient, the updated BatchNorm statistics).  Also
lists the state_dict of the model built from configs/my_dataset/keypoint_stratified_transformer.py.

Stand-ins for what the reference imports and this machine lacks (parity with the packages is unpinned):
  pointops2.pointops                     tests/strat_ref.py (CPU restatement of libs/pointops2)
  torch_geometric.nn.pool.voxel_grid     torch_cluster.grid_cluster over [pos | batch]: ((p - start) / size).long() per
                                         column, start = the column minima unless given (the section-15 stand-in, with
                                         the start argument)
  torch_scatter.scatter_softmax, torch_geometric.utils.scatter (mean), timm.layers.trunc_normal_
  torch_points_kernels.ball_query        strat_ref.ball_query (partial_dense)
  torch_points3d KPConvLayer / FastBatchNorm1d   restated below from the published source: linear influence, sum
                                         aggregation, a shadow point at 1e6 for index -1
  torch.cuda.IntTensor, Tensor.cuda      CPU no-ops
The float64 model keeps the fp32 COORDINATES: windows, sampled rows, neighbours and the quantized relative positions
are part of the input's definition and must be the same in both runs; only the feature arithmetic is float64.

A freshly built reference model leaves the key and value tables at zero (its trunc_normal_ hits the query table three
times); the seeded ones are non-zero.

The script asserts what the tests rest on:
  * every cell expression (small and large windows, unshifted and shifted, the reference's second shifted form
    (x - min + w/2) / w included), evaluated in float64, is at least 1e-4 from an integer and equals its fp32 value;
  * every farthest point sampling winner leads the runner-up by a relative 2e-6 (the section-13 margin);
  * some ball-query row is full and some holds only itself, and no squared distance is within 1e-5 (relative) of r^2;
  * the 40-point scene has 11 and then 3 rows below, so kNN-16 pads there and interpolation has exactly 3.
fp32 against float64 gaps are printed and stored as gap_*.  If an assertion fails, change the seed, not the tolerance.
usage: python tests/golden/make_golden_keypoint_strat.py [find-seed]"""
import importlib
import os
import sys
import types
import zlib

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden_keypoint_ptv1 import seeded_state_dict as _seeded  # noqa: E402
import strat_ref  # noqa: E402

TINY_KW = dict(in_channels=4, channels=(16, 32, 64), num_heads=(2, 4), depths=(2, 2), window_size=(0.2, 0.4),
               quant_size=(0.01, 0.05), mlp_expend_ratio=4.0, down_ratio=0.25, down_num_sample=16, kp_ball_radius=0.05,
               kp_max_neighbor=34, kp_grid_size=0.02, kp_sigma=1.0, drop_path_rate=0.0, stem=True, num_keypoints=6,
               hidden_dim=64)
SIZES = [1500, 40, 2600]
EDGES = [0.9, 0.4, 1.1]
DATA_SEED = 644                 # first seed whose margins hold (searched by find_seed())
TAP_STRIDE = {"embed": 32, "layer0": 8, "layer1": 2, "up0": 8, "up1": 32}
CELL_MARGIN = 1e-4
FPS_MARGIN = 2e-6
BALL_MARGIN = 1e-5
FP16_STEP = 2.0 ** -11


def seeded_state_dict(shapes, seed=1234):
    """make_golden_keypoint_ptv1.seeded_state_dict, with the three kinds of tensor it has no rule for drawn at a scale
    that keeps them in play: K_points inside the kernel ball (first one at the centre), KPConv weights ~ N(0, 1 / (3 in)),
    relative-position tables ~ 0.2 N."""
    out = _seeded(shapes, seed)
    for key, v in shapes.items():
        shape = tuple(v.shape) if hasattr(v, "shape") else tuple(v)
        rs = np.random.RandomState((zlib.crc32(key.encode()) ^ seed ^ 0x5A5A) & 0x7FFFFFFF)
        if key.endswith("K_points"):
            d = rs.standard_normal(shape)
            a = 0.03 * d / np.linalg.norm(d, axis=1, keepdims=True) * rs.random_sample((shape[0], 1)) ** (1 / 3)
            a[0] = 0
        elif key.endswith("kpconv.weight"):
            a = rs.standard_normal(shape) / np.sqrt(3 * shape[1])
        elif "relative_pos_" in key:
            a = 0.2 * rs.standard_normal(shape)
        else:
            continue
        out[key] = torch.from_numpy(np.asarray(a, dtype=np.float32))
    return out


def make_scenes(seed):
    """Three sheets z = 0.1 sin(3 x) + 0.02 N over a square of the scene's edge, each at its own origin; in the first
    scene five rows are lifted 0.3 off the sheet (alone in their ball) and the last forty sit in a 0.015 blob (full
    balls).  coord (n, 3) fp32, feat (n, 4) fp32, offset (3) int32."""
    rs = np.random.RandomState(seed)
    coord = []
    for k, (n, e) in enumerate(zip(SIZES, EDGES)):
        xy = rs.rand(n, 2) * e
        z = 0.1 * np.sin(3 * xy[:, 0]) + 0.02 * rs.randn(n)
        c = np.concatenate([xy, z[:, None]], 1)
        if k == 0:
            c[:5, 2] += 0.3
            d = rs.randn(40, 3)
            c[-40:] = c[700] + 0.015 * d / np.linalg.norm(d, axis=1, keepdims=True) * rs.rand(40, 1) ** (1 / 3)
        coord.append(c + rs.randn(3))
    coord = np.concatenate(coord).astype(np.float32)
    feat = rs.randn(len(coord), 4).astype(np.float32)
    return coord, feat, np.cumsum(SIZES).astype(np.int32)


def cell_margins(coord, window):
    """Smallest distance from an integer over the five cell expressions of one level, in float64, and whether every fp32
    cell equals the float64 one."""
    c32 = torch.as_tensor(coord, dtype=torch.float32)
    c64 = c32.double()
    margin, same = np.inf, True
    for c in (c32, c64):
        mn = c.min(0).values
        w = torch.tensor([window] * 3, dtype=c.dtype)
        exprs = [(c - mn) / w, (c - mn) / (2 * w), ((c + w * 1 / 2) - mn) / w, (c - mn + 1 / 2 * w) / w,
                 ((c + (2 * w) * 1 / 2) - mn) / (2 * w)]
        if c is c32:
            cells32 = [e.long() for e in exprs]
        else:
            for e, c32cell in zip(exprs, cells32):
                frac = (e - torch.round(e)).abs()
                nz = e != 0
                if nz.any():
                    margin = min(margin, float(frac[nz].min()))
                same = same and bool((e.long() == c32cell).all())
    return margin, same


def transition_down_counts(sizes, ratio):
    """TransitionDown.forward :470-476 (the float running sum, truncated by IntTensor)."""
    total = int(sizes[0] * ratio) + 1
    out = [total]
    for n in sizes[1:]:
        total += (n * ratio) + 1
        out.append(total)
    return [int(v) for v in out]


def level_coords(coord, ends):
    """The coordinates of the two BasicLayers for a batch - TransitionDown's sampling applied twice (stem, layer 0) - and
    the smallest relative lead of a winner over all five sampling calls of the forward."""
    out, gap = [], np.inf
    ends = [int(v) for v in ends]

    def sample(coord, ends, new_ends):
        nonlocal gap
        rows = []
        for s, e, ms, me in zip([0] + ends[:-1], ends, [0] + new_ends[:-1], new_ends):
            r, g = strat_ref.fps_scene(coord[s:e], me - ms)
            gap = min(gap, g)
            rows.append(r + s)
        return np.concatenate(rows)

    for level in range(3):
        sizes = [int(s) for s in np.diff([0] + ends)]
        if level:
            sample(coord, ends, np.cumsum([int(n * 0.25) + 1 for n in sizes]).tolist())     # BasicLayer's down_idx
        if level < 2:
            new_ends = transition_down_counts(sizes, 0.25)
            coord, ends = coord[sample(coord, ends, new_ends)], new_ends
            out.append((coord, ends))
    return out, gap


def find_seed(limit=4000):
    for seed in range(limit):
        coord, _, ends = make_scenes(seed)
        try:
            levels, gap = level_coords(coord, ends)
        except AssertionError:
            continue
        if gap < 2 * FPS_MARGIN:
            continue
        if all(cell_margins(c, w)[0] >= 2 * CELL_MARGIN and cell_margins(c, w)[1]
               for (c, _), w in zip(levels, TINY_KW["window_size"])):
            if strat_ref.ball_query(0.05, 34, coord, ends)[1] >= 2 * BALL_MARGIN:
                return seed
    raise RuntimeError("no seed holds the margins")


class KPConvLayer(nn.Module):
    """torch_points3d.modules.KPConv.kernels.KPConvLayer (KPConv_ops with KP_influence="linear", aggregation_mode="sum"),
    K_points a frozen parameter (n_kernel_points, 3), weight (n_kernel_points, in, out)."""

    def __init__(self, num_inputs, num_outputs, point_influence, n_kernel_points=15, add_one=False, **kw):
        super().__init__()
        assert not add_one
        self.point_influence = point_influence
        self.K_points = nn.Parameter(torch.zeros(n_kernel_points, 3), requires_grad=False)
        self.weight = nn.Parameter(torch.zeros(n_kernel_points, num_inputs, num_outputs))

    def forward(self, query_points, support_points, neighbors, x):
        shadow = torch.ones_like(support_points[:1, :]) * 1e6
        support = torch.cat([support_points, shadow], dim=0)
        nb = support[neighbors] - query_points.unsqueeze(1)
        differences = nb.unsqueeze(2) - self.K_points
        sq_distances = torch.sum(differences ** 2, dim=3)
        all_weights = torch.clamp(1 - torch.sqrt(sq_distances) / self.point_influence, min=0.0).transpose(2, 1)
        features = torch.cat([x, torch.zeros_like(x[:1, :])], dim=0)
        weighted = torch.matmul(all_weights.to(features.dtype), features[neighbors]).permute(1, 0, 2)
        return torch.sum(torch.matmul(weighted, self.weight), dim=0)


class FastBatchNorm1d(nn.Module):
    def __init__(self, num_features, momentum=0.1, **kw):
        super().__init__()
        self.batch_norm = nn.BatchNorm1d(num_features, momentum=momentum, **kw)

    def forward(self, x):
        return self.batch_norm(x)


def _install_stubs():
    def voxel_grid(pos, size, batch=None, start=None, end=None):
        assert batch is not None and end is None
        pos = torch.cat([pos, batch.view(-1, 1).to(pos.dtype)], dim=-1)
        size = torch.as_tensor(size, dtype=pos.dtype)
        sizes = torch.cat([size.expand(pos.shape[1] - 1), size.new_ones(1)])
        lo = pos.min(dim=0).values if start is None else torch.cat([start.to(pos.dtype), pos.new_zeros(1)])
        hi = pos.max(dim=0).values
        extent = ((hi - lo) / sizes).long() + 1
        stride = torch.cat([extent.new_ones(1), torch.cumprod(extent, 0)[:-1]])
        return (((pos - lo) / sizes).long() * stride).sum(1)

    def scatter(src, index, dim=0, dim_size=None, reduce="mean"):
        assert dim == 0 and reduce == "mean"
        out = torch.zeros((dim_size,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, index, src)
        return out / torch.bincount(index, minlength=dim_size).clamp(min=1).to(src.dtype).unsqueeze(-1)

    def ball_query(radius, max_neighbor, x, y, mode="partial_dense", batch_x=None, batch_y=None):
        assert mode == "partial_dense" and x is y
        ends = torch.bincount(batch_x).cumsum(0).tolist()
        idx, margin = strat_ref.ball_query(radius, max_neighbor, x.detach().numpy(), ends)
        BALL["margin"], BALL["idx"] = margin, idx
        return torch.from_numpy(idx), None

    tg = types.ModuleType("torch_geometric")
    tgn, tgp, tgu = (types.ModuleType("torch_geometric." + n) for n in ("nn", "nn.pool", "utils"))
    tgp.voxel_grid, tgu.scatter = voxel_grid, scatter
    tg.nn, tgn.pool, tg.utils = tgn, tgp, tgu
    sys.modules.update({"torch_geometric": tg, "torch_geometric.nn": tgn, "torch_geometric.nn.pool": tgp,
                        "torch_geometric.utils": tgu})
    sys.modules["torch_scatter"].scatter_softmax = strat_ref.scatter_softmax
    sys.modules["timm.layers"].trunc_normal_ = torch.nn.init.trunc_normal_
    tp = types.ModuleType("torch_points_kernels")
    tp.ball_query = ball_query
    sys.modules["torch_points_kernels"] = tp
    names = ["torch_points3d", "torch_points3d.modules", "torch_points3d.modules.KPConv",
             "torch_points3d.modules.KPConv.kernels", "torch_points3d.core", "torch_points3d.core.common_modules"]
    mods = {n: types.ModuleType(n) for n in names}
    for n, m in mods.items():
        m.__path__ = []
    mods["torch_points3d.modules.KPConv.kernels"].KPConvLayer = KPConvLayer
    mods["torch_points3d.core.common_modules"].FastBatchNorm1d = FastBatchNorm1d
    sys.modules.update(mods)
    p2 = types.ModuleType("pointops2")
    p2.__path__ = []
    p2.pointops = strat_ref
    sys.modules.update({"pointops2": p2, "pointops2.pointops": strat_ref})
    torch.cuda.IntTensor = lambda v: torch.tensor([int(x) for x in v], dtype=torch.int32)
    torch.Tensor.cuda = lambda self, *a, **k: self


BALL = {}


def _load_reference():
    import ref_loader
    assert ref_loader.available()
    ref_loader.load()
    _install_stubs()
    ref_loader._bare_pkg("pointcept.models.stratified_transformer",
                         os.path.join(ref_loader.REF, "pointcept", "models", "stratified_transformer"))
    importlib.import_module("pointcept.models.stratified_transformer.stratified_transformer_v1m2_refine")
    return importlib.import_module("pointcept.models.keypoint_stratified_transformer"), ref_loader


_FLOAT = torch.Tensor.float


def _tapped(model, data, train=False):
    """Run the model with taps.  The reference casts q / k / v and the tables with .float() in front of its fp32-only
    kernels; for the float64 model that cast is switched off, or the float64 run would be an fp32 one."""
    taps, hooks = {}, []
    is64 = next(model.parameters()).dtype == torch.float64
    torch.Tensor.float = (lambda self, *a, **k: self if self.dtype == torch.float64 else _FLOAT(self, *a, **k)) \
        if is64 else _FLOAT
    hooks.append(model.point_embed[-1].register_forward_hook(lambda m, i, o: taps.__setitem__("embed", o.detach().clone())))
    for i, layer in enumerate(model.layers):
        hooks.append(layer.register_forward_hook(
            lambda m, inp, out, i=i: taps.update({f"layer{i}": out[0].detach().clone(),
                                                  f"coord{i}": out[1].detach().clone(),
                                                  f"offset{i}": out[2].detach().clone()})))
    for i, up in enumerate(model.up):
        hooks.append(up.register_forward_hook(lambda m, inp, out, i=i: taps.__setitem__(f"up{i}", out[0].detach().clone())))
    strat_ref.FPS_LOG["samples"] = []
    if train:
        model.train()
        model.reg_head[3].p = 0.0
        model.zero_grad()
        out = model(dict(data))
        out["loss"].backward()
    else:
        with torch.no_grad():
            out = model.eval()(dict(data))
    torch.Tensor.float = _FLOAT
    for h in hooks:
        h.remove()
    taps["samples"] = list(strat_ref.FPS_LOG["samples"])
    return out, taps


ZERO_BIASES = ("reg_head.0.bias", "up.1.linear1.0.bias", "up.1.linear1.1.bias", "up.1.linear2.0.bias",
               "up.1.linear2.1.bias")


def _zero_bias(name):
    """Biases of the tiny model whose gradient is exactly zero, with rounding noise on both sides: the Linear straight in
    front of the head's batch-statistic BatchNorm, and the four biases of the last TransitionUp - each shifts every
    output row by the same vector (interpolation weights sum to one), so every scene mean moves alike and the
    BatchNorm's batch mean takes it out."""
    return name in ZERO_BIASES


def unpack_grads(flat, gmax, shapes):
    out, at = {}, 0
    for i, (k, shape) in enumerate(shapes.items()):
        n = int(np.prod(shape))
        out[k] = flat[at:at + n].astype(np.float32).reshape(shape) * gmax[i]
        at += n
    assert at == len(flat)
    return out


def grad_errors(grads, ref_grads):
    """{name: max|g - ref| / max(max|ref|, 1e-3 * the largest gradient of the model)} for all but the zero biases."""
    gmax = max(float(np.abs(v).max()) for v in ref_grads.values())
    return {n: float(np.abs(g - ref_grads[n]).max() / max(np.abs(ref_grads[n]).max(), 1e-3 * gmax))
            for n, g in grads.items() if not _zero_bias(n)}


def main():
    sys.path.insert(0, ROOT)
    kp, ref_loader = _load_reference()
    model = kp.KeypointStratifiedTransformer(**TINY_KW)
    fresh = model.layers[0].blocks[0].attn
    assert not fresh.relative_pos_key_table.detach().any() and not fresh.relative_pos_value_table.detach().any()
    print("tiny parameters", sum(p.numel() for p in model.parameters()))
    sd0 = seeded_state_dict(model.state_dict())
    model.load_state_dict(sd0, strict=True)
    coord, feat, ends = make_scenes(DATA_SEED)
    data = {"coord": torch.from_numpy(coord), "feat": torch.from_numpy(feat), "offset": torch.from_numpy(ends)}
    g = torch.Generator().manual_seed(5)
    data["target"] = torch.randn(len(SIZES) * 6, 3, generator=g) * 0.5
    data["scale"] = torch.rand(len(SIZES), generator=g) + 0.5
    res = {"in_" + k: v.numpy() for k, v in data.items()}

    model64 = kp.KeypointStratifiedTransformer(**TINY_KW).double()
    model64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd0.items()}, strict=True)
    data64 = {k: (v.double() if v.is_floating_point() and k != "coord" else v) for k, v in data.items()}

    strat_ref.FPS_LOG["gap"] = np.inf
    out, taps = _tapped(model, data)
    out64, taps64 = _tapped(model64, data64)
    res["eval_pred"], res["eval_loss"] = out["pred"].numpy(), out["loss"].numpy()
    print("farthest point sampling: smallest relative lead", strat_ref.FPS_LOG["gap"])
    assert strat_ref.FPS_LOG["gap"] >= FPS_MARGIN
    # call order: stem down, then per layer BasicLayer's down_idx and (all but the last) its TransitionDown
    names = ["stem_down", "layer0_down_idx", "layer0_down", "layer1_down_idx"]
    assert len(taps["samples"]) == len(names)
    for nm, s, s64 in zip(names, taps["samples"], taps64["samples"]):
        assert np.array_equal(s, s64)
        res["rows_" + nm] = s.astype(np.int32)
    ball = BALL["idx"]
    full, alone = int((ball[:, -1] >= 0).sum()), int((ball[:, 1] < 0).sum())
    print(f"ball query: {full} full rows, {alone} rows alone, margin {BALL['margin']:.3e}")
    assert full > 0 and alone > 0 and BALL["margin"] >= BALL_MARGIN
    sizes = []
    for i, w in enumerate(TINY_KW["window_size"]):
        c, o = taps[f"coord{i}"].numpy(), taps[f"offset{i}"].numpy()
        margin, same = cell_margins(c, w)
        print(f"layer {i}: {len(c)} points, cell margin {margin:.3e}, fp32 cells equal float64 cells: {same}")
        assert margin >= CELL_MARGIN and same, (i, margin, same)
        sizes.append(np.diff(np.concatenate([[0], o])).tolist())
        res[f"coord_layer{i}"] = c
        res[f"offset_layer{i}"] = o.astype(np.int32)
        for parity in range(2):
            groups = strat_ref.group_plan(c, o, res[f"rows_layer{i}_down_idx"], w, bool(parity))
            i0, i1 = strat_ref.reference_edges(c, o, res[f"rows_layer{i}_down_idx"], w, bool(parity))
            assert sum(len(q) * len(k) for q, k in groups) == len(i0), (i, parity)
            res[f"groups_{i}_{parity}"] = np.int32(len(groups))
            res[f"edges_{i}_{parity}"] = np.int64(len(i0))
            print(f"layer {i} parity {parity}: {len(groups)} groups, {len(i0)} edges")
    print("scene sizes per layer", sizes)
    assert sizes[0][1] == 11 and sizes[1][1] == 3, sizes
    gaps = {}
    for name, stride in TAP_STRIDE.items():
        x, x64 = taps[name].numpy(), taps64[name].numpy()
        res["tap_" + name] = x[::stride].copy()
        gaps[name] = float(np.abs(x - x64).max() / max(1.0, np.abs(x64).max()))
    gaps["pred"] = float(np.abs(res["eval_pred"] - out64["pred"].numpy()).max())
    gaps["eval_loss"] = abs(float(res["eval_loss"]) - float(out64["loss"]))

    out, _ = _tapped(model, data, train=True)
    out64, _ = _tapped(model64, data64, train=True)
    res["loss"] = out["loss"].detach().numpy()
    res["mean_dist"] = out["train/mean_dist"].numpy()
    res["kp_dist"] = np.array([out[f"train/kp{i}_dist"].item() for i in range(6)], dtype=np.float32)
    grads = {k: p.grad.detach().clone().numpy() for k, p in model.named_parameters() if p.grad is not None}
    bufs = {k: b.detach().clone().numpy() for k, b in model.named_buffers() if "running" in k}
    tops = {k: max(float(np.abs(gr).max()), 1e-30) for k, gr in grads.items()}
    res["grads"] = np.concatenate([(gr / tops[k]).astype(np.float16).ravel() for k, gr in grads.items()])
    res["gmax"] = np.array([tops[k] for k in grads], dtype=np.float32)
    res["bufs"] = np.concatenate([b.ravel() for b in bufs.values()]).astype(np.float32)
    grads64 = {k: p.grad.numpy() for k, p in model64.named_parameters() if p.grad is not None}
    bufs64 = {k: b.detach().numpy() for k, b in model64.named_buffers() if "running" in k}
    gaps["loss"] = abs(float(res["loss"]) - float(out64["loss"]))
    gaps["mean_dist"] = abs(float(res["mean_dist"]) - float(out64["train/mean_dist"]))
    gaps["kp_dist"] = float(np.abs(res["kp_dist"] - np.array([out64[f"train/kp{i}_dist"].item() for i in range(6)])).max())
    errs = grad_errors(grads, grads64)
    gaps["buf"] = max(float(np.abs(b - bufs64[n]).max() / max(np.abs(bufs64[n]).max(), 1e-6)) for n, b in bufs.items())
    for k, v in gaps.items():
        print(f"fp32 vs float64 gap {k}: {v:.3e}")
        res["gap_" + k] = np.float64(v)
    stored = unpack_grads(res["grads"], res["gmax"], {k: v.shape for k, v in grads.items()})
    res["gap_grads"] = np.array([errs.get(k, 0.0) for k in grads], dtype=np.float64)
    print("per-tensor gradient gaps: median %.3e, 90%% %.3e, max %.3e" % tuple(
        np.percentile([v for v in errs.values()], [50, 90, 100])))
    for n, e in grad_errors(stored, grads64).items():
        assert e <= 4 * errs[n] + FP16_STEP, (n, e)
    for n in grads:
        if _zero_bias(n):
            assert np.abs(grads[n]).max() <= 1e-4 * np.abs(grads[n[:-4] + "weight"]).max(), n

    path = os.path.join(HERE, "keypoint_strat_tiny.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("keypoint_strat_tiny.npz", size // 1024, "KiB; eval loss", float(res["eval_loss"]))

    from make_golden_keypoint_regression import write_listing
    scope = {}
    cfg_path = os.path.join(ref_loader.REF, "configs", "my_dataset", "keypoint_stratified_transformer.py")
    exec(compile(open(cfg_path).read(), cfg_path, "exec"), scope)
    from pointcept.models.builder import MODELS
    fork = MODELS.build(scope["model"])
    print("fork parameters", sum(p.numel() for p in fork.parameters()))
    write_listing(fork, "state_dict_keypoint_strat_fork.txt")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "find-seed":
        print("seed", find_seed())
    else:
        main()
