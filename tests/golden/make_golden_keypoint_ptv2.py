"""Build-container-only: run the reference's KeypointPTv2 (pointcept/models/keypoint_ptv2.py over
point_transformer_v2/point_transformer_v2m2_base.py, both imported in place) on a seeded three-scene batch with float
coordinates and store, in keypoint_ptv2_tiny.npz, its eval `pred` and loss, every level's pooled row counts, `cluster`
maps, pooled coordinates and offsets, a strided subset of every encoder and decoder stage's output features, and one
training step (loss, curves, every parameter gradient, the updated BatchNorm running statistics).  Also lists the
state_dict of the model built from configs/my_dataset/keypoint_ptv2.py.

The reference's native dependencies here are libs/pointops (the stub of make_golden_keypoint_ptv1.py: its Python files
imported where they lie, kNN from oracle/pointops.py) and three package functions, restated below for the CPU from their
published semantics (none of the packages is installed; parity with them is unpinned):
  torch_geometric.nn.pool.voxel_grid(pos, size, batch, start=0)   torch_cluster.grid_cluster over [pos | batch] with voxel
      sizes [size, size, size, 1], start 0 and end = the column maxima: cell = ((p - start) / size).long() per column,
      id = sum_d cell_d * stride_d with stride_0 = 1 and stride_{d+1} = stride_d * (((end_d - start_d) / size_d).long() + 1)
      - x runs fastest, the batch slowest, so torch.unique ranks the ids by (batch, cz, cy, cx)
  torch_scatter.segment_csr(src, indptr, reduce)                  ref_loader's torch.segment_reduce stand-in: the
      min / mean / max of src[indptr[j] : indptr[j + 1]] per j
  timm.layers.DropPath                                            ref_loader's stand-in; the tiny config has
      drop_path_rate = 0, so the reference builds nn.Identity and the class is never called

The fixture stays under 1 MiB: weights come from seeded_state_dict() (key names -> numpy's frozen RandomState streams),
each gradient is float16 of grad / max|grad| plus that fp32 maximum (all of them in one flat array, in named_parameters()
order), and the feature taps keep every TAP_STRIDE-th row.
The head's Dropout is at p = 0 for the training step.

The script asserts what the tests rest on:
  * at every level every (coord - start) / size, computed in float64, is at least 1e-4 away from an integer and its
    fp32 cell equals the float64 one.  The one exception is an exact zero: the scene's own minimum minus itself is 0 in
    any arithmetic, so it cannot round across a cell boundary;
  * the 0.5-wide scene has fewer than 16 points at its deepest level (so -1 neighbours occur) and the 1.3-wide scene has at
    least 16 at every level;
  * the float64 eval and training step agree with the fp32 ones within the GPU test's tolerances, which are four times
    the gaps printed here (stored in the fixture as gap_*; for gradients one gap per tensor, gap_grads), plus the
    float16 step of the stored gradients.
If an assertion fails, change the seed, not the tolerance.
usage: python tests/golden/make_golden_keypoint_ptv2.py"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_golden_keypoint_ptv1 import seeded_state_dict  # noqa: E402,F401  (the tests import it from here)

TINY_BACKBONE = dict(
    type="PT-v2m2", in_channels=4, num_classes=0, patch_embed_depth=1, patch_embed_channels=16, patch_embed_groups=2,
    patch_embed_neighbours=8, enc_depths=(1, 1, 2, 1), enc_channels=(32, 48, 64, 96), enc_groups=(4, 6, 8, 12),
    enc_neighbours=(16, 16, 16, 16), dec_depths=(1, 1, 1, 1), dec_channels=(16, 32, 48, 64), dec_groups=(2, 4, 6, 8),
    dec_neighbours=(8, 16, 16, 16), grid_sizes=(0.06, 0.12, 0.24, 0.48), attn_qkv_bias=True, pe_multiplier=False,
    pe_bias=True, attn_drop_rate=0.0, drop_path_rate=0.0, enable_checkpoint=False, unpool_backend="map")
TINY_KW = dict(backbone_conf=TINY_BACKBONE, num_keypoints=6, hidden_dim=64)
# the five (C, G, ns) of the tiny model's attention layers
TINY_SHAPES = [(16, 2, 8), (32, 4, 16), (48, 6, 16), (64, 8, 16), (96, 12, 16)]
SIZES = [1500, 700, 2600]
EDGES = [1.0, 0.5, 1.3]          # cube edge of every scene
DATA_SEED = 560                  # first seed whose cell margins hold (searched by find_seed())
TAP_STRIDE = [32, 16, 8, 4, 1]  # rows kept of the features at levels 0..4
MARGIN = 1e-4
FP16_STEP = 2.0 ** -11           # float16 rounding of a value in [-1, 1]


def make_scenes(seed):
    """coord (n, 3) fp32 uniform in every scene's cube (each at its own origin), feat (n, 4), offset (3) int32."""
    rs = np.random.RandomState(seed)
    coord = [rs.rand(n, 3) * e + rs.randn(3) for n, e in zip(SIZES, EDGES)]
    coord = np.concatenate(coord).astype(np.float32)
    feat = rs.randn(len(coord), 4).astype(np.float32)
    return coord, feat, np.cumsum(SIZES).astype(np.int32)


def cell_margin(coord, ends, size):
    """-> (smallest distance of a non-zero (coord - start) / size from an integer, in float64; whether every fp32 cell
    equals the float64 one; the fp32 cells (n, 3) int64 and the scene ids).  start = the scene's per-axis minimum."""
    coord = np.asarray(coord, dtype=np.float32)
    batch = np.repeat(np.arange(len(ends)), np.diff(np.concatenate([[0], ends])))
    start = np.stack([coord[batch == b].min(0) for b in range(len(ends))])[batch]
    d32 = coord - start
    q32 = d32 / np.float32(size)
    q64 = (coord.astype(np.float64) - start.astype(np.float64)) / float(size)
    frac = np.abs(q64 - np.rint(q64))
    margin = frac[q64 != 0].min() if (q64 != 0).any() else np.inf
    cells = q32.astype(np.int64)
    return margin, bool((cells == np.floor(q64).astype(np.int64)).all()), cells, batch


def pool_level(coord, ends, size):
    """One GridPool in numpy: (cluster (n), pooled coord (m, 3) fp32 summed in sorted order, pooled ends)."""
    _, _, cells, batch = cell_margin(coord, ends, size)
    key = ((batch * (1 << 17) + cells[:, 2]) * (1 << 17) + cells[:, 1]) * (1 << 17) + cells[:, 0]
    uniq, cluster, counts = np.unique(key, return_inverse=True, return_counts=True)
    order = np.argsort(cluster, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(counts)])
    pooled = np.stack([coord[order[a:b]].astype(np.float64).mean(0) for a, b in zip(ptr[:-1], ptr[1:])])
    pooled_batch = batch[order[ptr[:-1]]]
    return cluster, pooled.astype(np.float32), np.cumsum(np.bincount(pooled_batch, minlength=len(ends)))


def find_seed(limit=2000):
    """First data seed whose four levels hold the cell margin (pooled coordinates in float64 here; main() asserts the
    margin again on the coordinates the reference model really pools)."""
    for seed in range(limit):
        coord, _, ends = make_scenes(seed)
        ok = True
        for size in TINY_BACKBONE["grid_sizes"]:
            margin, same, _, _ = cell_margin(coord, ends, size)
            if margin < 2 * MARGIN or not same:
                ok = False
                break
            _, coord, ends = pool_level(coord, ends, size)
        if ok:
            return seed
    raise RuntimeError("no seed holds the margin")


def _install_package_stubs():
    """voxel_grid as described in the module docstring (segment_csr and DropPath come from ref_loader)."""
    def voxel_grid(pos, size, batch=None, start=None, end=None):
        assert batch is not None and end is None and (start is None or start == 0)
        pos = torch.cat([pos, batch.view(-1, 1).to(pos.dtype)], dim=-1)
        sizes = torch.tensor([size] * (pos.shape[1] - 1) + [1], dtype=pos.dtype)
        lo = torch.zeros(pos.shape[1], dtype=pos.dtype)
        hi = pos.max(dim=0).values
        extent = ((hi - lo) / sizes).long() + 1
        stride = torch.cat([extent.new_ones(1), torch.cumprod(extent, 0)[:-1]])
        return (((pos - lo) / sizes).long() * stride).sum(1)

    tg = types.ModuleType("torch_geometric")
    tgn = types.ModuleType("torch_geometric.nn")
    tgp = types.ModuleType("torch_geometric.nn.pool")
    tgp.voxel_grid = voxel_grid
    tg.nn, tgn.pool = tgn, tgp
    sys.modules.update({"torch_geometric": tg, "torch_geometric.nn": tgn, "torch_geometric.nn.pool": tgp})


def _load_reference():
    import ref_loader
    import make_golden_keypoint_ptv1 as ptv1
    assert ref_loader.available()
    ptv1.REF = ref_loader.REF
    ptv1._install_pointops_stub()
    ref_loader.load()
    _install_package_stubs()
    torch.cuda.IntTensor = lambda v: torch.tensor(v, dtype=torch.int32)
    ref_loader._bare_pkg("pointcept.models.point_transformer_v2",
                         os.path.join(ref_loader.REF, "pointcept", "models", "point_transformer_v2"))
    importlib.import_module("pointcept.models.point_transformer_v2.point_transformer_v2m2_base")
    return importlib.import_module("pointcept.models.keypoint_ptv2"), ref_loader


def _tapped(model, data, train=False):
    """Run the model; returns (output dict, taps): taps["enc{i}"] / ["dec{i}"] = the stage's output [coord, feat,
    offset], taps["cluster{i}"] = the map of encoder i's pooling."""
    taps, hooks = {}, []
    bb = model.backbone
    for i in range(bb.num_stages):
        hooks.append(bb.enc_stages[i].register_forward_hook(
            lambda m, inp, out, i=i: taps.update({f"enc{i}": [t.detach().clone() for t in out[0]],
                                                  f"cluster{i}": out[1].detach().clone()})))
        hooks.append(bb.dec_stages[i].register_forward_hook(
            lambda m, inp, out, i=i: taps.__setitem__(f"dec{i}", [t.detach().clone() for t in out])))
        hooks.append(bb.enc_stages[i].down.register_forward_hook(
            lambda m, inp, out, i=i: taps.__setitem__(f"pool_in{i}", [t.detach().clone() for t in inp[0]])))
    if train:
        model.train()
        model.reg_head[3].p = 0.0
        model.zero_grad()
        out = model(dict(data))
        out["loss"].backward()
    else:
        with torch.no_grad():
            out = model.eval()(dict(data))
    for h in hooks:
        h.remove()
    return out, taps


def _zero_bias(name):
    """Biases of a Linear straight in front of a batch-statistic BatchNorm: exact gradient zero, noise on both sides."""
    return name == "reg_head.0.bias" or any(name.endswith(s) for s in (
        "linear_q.0.bias", "linear_k.0.bias", "linear_p_bias.0.bias", "weight_encoding.0.bias", "proj.0.bias",
        "proj_skip.0.bias"))


def unpack_grads(flat, gmax, shapes):
    """{name: fp32 gradient} from the fixture's flat float16 array, the per-tensor maxima and {name: shape} in
    named_parameters() order."""
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
    model = kp.KeypointPTv2(**TINY_KW)
    n_params = sum(p.numel() for p in model.parameters())
    print("tiny parameters", n_params)
    sd0 = seeded_state_dict(model.state_dict())
    model.load_state_dict(sd0, strict=True)
    coord, feat, ends = make_scenes(DATA_SEED)
    data = {"coord": torch.from_numpy(coord), "feat": torch.from_numpy(feat), "offset": torch.from_numpy(ends)}
    g = torch.Generator().manual_seed(5)
    data["target"] = torch.randn(len(SIZES) * 6, 3, generator=g) * 0.5
    data["scale"] = torch.rand(len(SIZES), generator=g) + 0.5
    res = {"in_" + k: v.numpy() for k, v in data.items()}

    model64 = kp.KeypointPTv2(**TINY_KW).double()
    model64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd0.items()}, strict=True)
    data64 = {k: (v.double() if v.is_floating_point() else v) for k, v in data.items()}

    out, taps = _tapped(model, data)
    out64, taps64 = _tapped(model64, data64)
    res["eval_pred"], res["eval_loss"] = out["pred"].numpy(), out["loss"].numpy()
    stages = model.backbone.num_stages
    sizes = []
    for i in range(stages):
        pc, _, po = taps[f"pool_in{i}"]
        margin, same, _, _ = cell_margin(pc.numpy(), po.numpy(), TINY_BACKBONE["grid_sizes"][i])
        print(f"level {i}: {len(pc)} points, cell margin {margin:.3e}, fp32 cells equal float64 cells: {same}")
        assert margin >= MARGIN and same, (i, margin, same)
        assert torch.equal(taps[f"cluster{i}"], taps64[f"cluster{i}"]), i
        c, x, o = taps[f"enc{i}"]
        res[f"cluster{i}"] = taps[f"cluster{i}"].numpy().astype(np.int32)
        res[f"coord{i + 1}"] = c.numpy()
        res[f"offset{i + 1}"] = o.numpy().astype(np.int32)
        res[f"count{i + 1}"] = np.int32(len(c))
        sizes.append(np.diff(np.concatenate([[0], o.numpy()])))
    print("scene sizes per level", [s.tolist() for s in sizes])
    assert sizes[-1][1] < 16 and all(s[2] >= 16 for s in sizes), sizes
    gaps = {}
    for i in range(stages):
        for kind, level in (("enc", i + 1), ("dec", i)):
            x, x64 = taps[f"{kind}{i}"][1].numpy(), taps64[f"{kind}{i}"][1].numpy()
            res[f"tap_{kind}{i}"] = x[::TAP_STRIDE[level]].copy()
            gaps[f"{kind}{i}"] = float(np.abs(x - x64).max() / max(1.0, np.abs(x64).max()))
    gaps["pred"] = float(np.abs(res["eval_pred"] - out64["pred"].numpy()).max())
    gaps["eval_loss"] = abs(float(res["eval_loss"]) - float(out64["loss"]))

    out, _ = _tapped(model, data, train=True)
    out64, _ = _tapped(model64, data64, train=True)
    res["loss"] = out["loss"].detach().numpy()
    res["mean_dist"] = out["train/mean_dist"].numpy()
    res["kp_dist"] = np.array([out[f"train/kp{i}_dist"].item() for i in range(6)], dtype=np.float32)
    grads = {k: p.grad.detach().clone().numpy() for k, p in model.named_parameters()}
    bufs = {k: b.detach().clone().numpy() for k, b in model.named_buffers() if "running" in k}
    # one flat array each, in named_parameters() / named_buffers() order (a zip member per tensor would cost more than
    # the small tensors themselves)
    tops = {k: max(float(np.abs(gr).max()), 1e-30) for k, gr in grads.items()}
    res["grads"] = np.concatenate([(gr / tops[k]).astype(np.float16).ravel() for k, gr in grads.items()])
    res["gmax"] = np.array([tops[k] for k in grads], dtype=np.float32)
    res["bufs"] = np.concatenate([b.ravel() for b in bufs.values()]).astype(np.float32)
    grads64 = {k: p.grad.numpy() for k, p in model64.named_parameters()}
    bufs64 = {k: b.detach().numpy() for k, b in model64.named_buffers() if "running" in k}
    gaps["loss"] = abs(float(res["loss"]) - float(out64["loss"]))
    gaps["mean_dist"] = abs(float(res["mean_dist"]) - float(out64["train/mean_dist"]))
    gaps["kp_dist"] = float(np.abs(res["kp_dist"] - np.array([out64[f"train/kp{i}_dist"].item() for i in range(6)])).max())
    errs = grad_errors(grads, grads64)
    gaps["grad_head"] = max(v for k, v in errs.items() if k.startswith("reg_head."))
    gaps["grad_backbone"] = max(v for k, v in errs.items() if not k.startswith("reg_head."))
    gaps["buf"] = max(float(np.abs(b - bufs64[n]).max() / max(np.abs(bufs64[n]).max(), 1e-6)) for n, b in bufs.items())
    for k, v in gaps.items():
        print(f"fp32 vs float64 gap {k}: {v:.3e}")
        res["gap_" + k] = np.float64(v)
    # the stored float16 gradients against float64, within the GPU test's tolerance (4 gaps + the float16 step)
    stored = unpack_grads(res["grads"], res["gmax"], {k: v.shape for k, v in grads.items()})
    # per tensor, in named_parameters() order (0 for the zero biases): the GPU test holds every tensor to its own gap,
    # so the ill-conditioned few (batch statistics over the deepest level's 36 rows) do not loosen the others
    res["gap_grads"] = np.array([errs.get(k, 0.0) for k in grads], dtype=np.float64)
    print("per-tensor gradient gaps: median %.3e, 90%% %.3e, max %.3e" % tuple(
        np.percentile([v for v in errs.values()], [50, 90, 100])))
    for n, e in grad_errors(stored, grads64).items():
        assert e <= 4 * errs[n] + FP16_STEP, (n, e)
    # a zero bias holds rounding noise only: at most 1e-4 of its layer's weight gradient on both sides
    for n in grads:
        if _zero_bias(n):
            assert np.abs(grads[n]).max() <= 1e-4 * np.abs(grads[n[:-4] + "weight"]).max(), n

    path = os.path.join(HERE, "keypoint_ptv2_tiny.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("keypoint_ptv2_tiny.npz", size // 1024, "KiB; eval loss", float(res["eval_loss"]))

    from make_golden_keypoint_regression import write_listing
    scope = {}
    cfg_path = os.path.join(ref_loader.REF, "configs", "my_dataset", "keypoint_ptv2.py")
    exec(compile(open(cfg_path).read(), cfg_path, "exec"), scope)
    from pointcept.models.builder import MODELS
    fork = MODELS.build(scope["model"])
    print("fork parameters", sum(p.numel() for p in fork.parameters()))
    write_listing(fork, "state_dict_keypoint_ptv2_fork.txt")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "find-seed":
        print("seed", find_seed())
    else:
        main()
