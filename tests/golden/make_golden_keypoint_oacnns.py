"""Build-container-only: run the reference's KeypointOACNNs (pointcept/models/keypoint_oa_cnns.py over
oacnns/oacnns_v1m1_base.py, both imported in place) on a seeded two-scene batch and store, in keypoint_oacnns_tiny.npz,
its eval `pred` and loss, feature taps (after the stem, after each of the 8 blocks, `mixed` of one BasicBlock), the
coarse site lists of every level and one training step (loss, curves, every parameter gradient, the updated BatchNorm
running statistics).  Also lists the state_dict of the model built from configs/my_dataset/keypoint_oa_cnns.py.

The reference's native dependencies are not installed; CPU stand-ins written here take their place (parity with the
real packages unpinned, their behaviour restated from their published semantics):
  spconv.pytorch      SubMConv3d -> oracle.ptv3.subm_conv3d (ref_loader); SparseConv3d(kernel 2, stride 2): parent
                      (b, x>>1, y>>1, z>>1), tap (x&1)*4 + (y&1)*2 + (z&1), output shape (S - 2) // 2 + 1, a site whose
                      parent lies outside it contributes nothing, coarse rows sorted by (b, x, y, z);
                      SparseInverseConv3d: out[i] = W[:, tap(i), :] y[parent(i)], zero without a parent
  torch_geometric     voxel_grid: cell = trunc((pos - min over all rows) / size) in fp32, batch as a fourth axis;
                      scatter(sum | mean) by index_add
  timm.layers         trunc_normal_ = torch.nn.init.trunc_normal_

Weights are not stored: seeded_state_dict() derives them from the key names with numpy's frozen RandomState streams and
the GPU test calls the same function.  Gradients are stored as float16 of grad / max|grad| plus that maximum.

The script asserts what the tests rely on: at least one site without a parent and no scene empty at any level; every
p_l has a unique maximum; every cluster's S >= 1e-3 (so the 1e-6 in the denominator does not amplify rounding); the
training step in float64 agrees with the fp32 one within the GPU test's tolerances.  If an assertion fails, change the
seed or the weight scale, not the tolerance.
usage: python tests/golden/make_golden_keypoint_oacnns.py"""
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

TINY_KW = dict(num_keypoints=6, hidden_dim=32, in_channels=4, embed_channels=16, enc_channels=[16, 16, 32, 32],
               groups=[2, 2, 4, 4], enc_depth=[1, 1, 2, 1], dec_channels=[16, 16, 32, 32],
               point_grid_size=[[4, 6, 6], [3, 4, 4], [2, 3, 3], [2, 2, 3]], dec_depth=[2, 2, 2, 2],
               enc_num_ref=[16, 16, 16, 16])
SIZES = [600, 250]
EXTENT = 51
WEIGHT_SEED = 77
LOGIT_SCALE = 0.5          # of BasicBlock.weight[l]: keeps every cluster's softmax mass S above 1e-3
MIXED_BLOCK = "enc.2.blocks.1"
TAPS = ["stem"] + [f"enc.{i}" for i in range(4)] + [f"dec.{i}" for i in (3, 2, 1, 0)]
TAP_STRIDE = 2             # rows kept of the taps on the 850 input sites


def seeded_state_dict(shapes, seed=WEIGHT_SEED):
    """{key: tensor} for a KeypointOACNNs state_dict given as {key: tensor or shape}: every entry drawn from
    numpy.random.RandomState(crc32(key) ^ seed).  Linear / conv weights ~ N(0, 1 / fan_in) (the logit Linears
    `weight.{l}` times LOGIT_SCALE), BatchNorm weights 1 + 0.1 N, biases and running means 0.1 N, running variances
    U(0.5, 1.5)."""
    out = {}
    for key, v in shapes.items():
        shape = tuple(v.shape) if hasattr(v, "shape") else tuple(v)
        rs = np.random.RandomState((zlib.crc32(key.encode()) ^ seed) & 0x7FFFFFFF)
        if key.endswith("num_batches_tracked"):
            out[key] = torch.zeros(shape, dtype=torch.int64)
            continue
        if key.endswith("running_var"):
            a = rs.random_sample(shape) + 0.5
        elif key.endswith("running_mean") or key.endswith("bias"):
            a = 0.1 * rs.standard_normal(shape)
        elif len(shape) >= 2:
            a = rs.standard_normal(shape) / np.sqrt(np.prod(shape[1:]))
            if ".weight." in key:
                a = a * LOGIT_SCALE
        else:
            a = 1.0 + 0.1 * rs.standard_normal(shape)
        out[key] = torch.from_numpy(np.asarray(a, dtype=np.float32).reshape(shape))
    return out


def down2_plan_numpy(indices, shape):
    """(parent (n) int64 with -1 = none, tap (n), coarse (m, 4), coarse shape) of a kernel-2 / stride-2 sparse conv."""
    idx = np.asarray(indices, dtype=np.int64)
    out_shape = [(int(s) - 2) // 2 + 1 for s in shape]
    par = idx[:, 1:] >> 1
    ok = np.all(par < np.asarray(out_shape), axis=1)
    tap = (idx[:, 1] & 1) * 4 + (idx[:, 2] & 1) * 2 + (idx[:, 3] & 1)
    key = ((idx[:, 0] * out_shape[0] + par[:, 0]) * out_shape[1] + par[:, 1]) * out_shape[2] + par[:, 2]
    uniq, inv = np.unique(key[ok], return_inverse=True)
    parent = np.full(len(idx), -1, dtype=np.int64)
    parent[ok] = inv
    coarse = np.stack([uniq // (out_shape[0] * out_shape[1] * out_shape[2]),
                       uniq // (out_shape[1] * out_shape[2]) % out_shape[0],
                       uniq // out_shape[2] % out_shape[1], uniq % out_shape[2]], axis=1)
    return parent, tap, coarse, out_shape


class _Rec:
    smin = np.inf
    dropped = []


def _install_standins():
    sp = sys.modules["spconv.pytorch"]
    SubM = sp.SubMConv3d

    class SparseConvTensor:
        def __init__(self, features, indices, spatial_shape, batch_size, plans=None):
            self.features, self.indices = features, indices
            self.spatial_shape, self.batch_size = spatial_shape, batch_size
            self.plans = {} if plans is None else plans

        def replace_feature(self, feat):
            return SparseConvTensor(feat, self.indices, self.spatial_shape, self.batch_size, self.plans)

    class _Strided(nn.Module):
        def __init__(self, in_channels, out_channels, kernel_size, stride=2, indice_key=None, bias=False, **kw):
            super().__init__()
            assert kernel_size == 2 and stride == 2 and not bias
            self.indice_key = indice_key
            self.weight = nn.Parameter(torch.empty(out_channels, 2, 2, 2, in_channels))
            nn.init.normal_(self.weight, std=(1.0 / (8 * in_channels)) ** 0.5)

    class SparseConv3d(_Strided):
        def forward(self, x):
            parent, tap, coarse, out_shape = down2_plan_numpy(x.indices.numpy(), x.spatial_shape)
            x.plans[self.indice_key] = (parent, tap, x)
            _Rec.dropped.append(int((parent < 0).sum()))
            w = self.weight.reshape(self.weight.shape[0], 8, -1)
            out = x.features.new_zeros(len(coarse), w.shape[0])
            for t in range(8):
                rows = torch.from_numpy(np.nonzero((parent >= 0) & (tap == t))[0])
                out = out.index_add(0, torch.from_numpy(parent)[rows], x.features[rows] @ w[:, t].T)
            y = SparseConvTensor(out, torch.from_numpy(coarse).int(), out_shape, x.batch_size, x.plans)
            return y

    class SparseInverseConv3d(_Strided):
        def forward(self, x):
            parent, tap, fine = x.plans[self.indice_key]
            w = self.weight.reshape(self.weight.shape[0], 8, -1)
            out = x.features.new_zeros(len(parent), w.shape[0])
            for t in range(8):
                rows = torch.from_numpy(np.nonzero((parent >= 0) & (tap == t))[0])
                out = out.index_put((rows,), x.features[torch.from_numpy(parent)[rows]] @ w[:, t].T)
            return SparseConvTensor(out, fine.indices, fine.spatial_shape, fine.batch_size, x.plans)

    class SparseSequential(nn.Sequential):
        def forward(self, x):
            for m in self:
                x = m(x) if isinstance(m, (SubM, _Strided)) else x.replace_feature(m(x.features))
            return x

    sp.SparseConvTensor, sp.SparseConv3d, sp.SparseInverseConv3d = SparseConvTensor, SparseConv3d, SparseInverseConv3d
    sp.SparseSequential = SparseSequential
    sys.modules["timm.layers"].trunc_normal_ = nn.init.trunc_normal_

    def voxel_grid(pos, size, batch):
        p = torch.cat([pos, batch.to(pos.dtype).unsqueeze(1)], dim=1)
        sz = torch.tensor([size, size, size, 1], dtype=pos.dtype)
        lo, hi = p.min(0).values, p.max(0).values
        cell = ((p - lo) / sz).long()
        count = ((hi - lo) / sz).long() + 1
        return ((cell[:, 3] * count[2] + cell[:, 2]) * count[1] + cell[:, 1]) * count[0] + cell[:, 0]

    def scatter(src, index, dim=0, dim_size=None, reduce="sum"):
        size = int(index.max()) + 1 if dim_size is None else dim_size
        out = src.new_zeros((size,) + tuple(src.shape[1:])).index_add(0, index, src)
        if reduce == "mean":
            cnt = torch.bincount(index, minlength=size).clamp(min=1).to(src.dtype)
            out = out / cnt.view(-1, *([1] * (src.dim() - 1)))
        return out

    def scatter_recording(src, index, **kw):
        out = scatter(src, index, **kw)
        if kw.get("reduce") == "sum" and "dim" in kw:     # oacnns_v1m1_base.py:95, the softmax mass S per cluster
            _Rec.smin = min(_Rec.smin, float(out.detach().min()))
        return out

    tg = types.ModuleType("torch_geometric")
    tgn, tgp, tgu = (types.ModuleType("torch_geometric." + n) for n in ("nn", "nn.pool", "utils"))
    tgp.voxel_grid, tgu.scatter = voxel_grid, scatter_recording
    tg.nn, tgn.pool, tg.utils = tgn, tgp, tgu
    sys.modules.update({"torch_geometric": tg, "torch_geometric.nn": tgn, "torch_geometric.nn.pool": tgp,
                        "torch_geometric.utils": tgu})


def _load_reference():
    import ref_loader
    assert ref_loader.available()
    ref_loader.load()
    _install_standins()
    pkg = ref_loader._bare_pkg("pointcept.models.oacnns", os.path.join(ref_loader.REF, "pointcept", "models", "oacnns"))
    base = importlib.import_module("pointcept.models.oacnns.oacnns_v1m1_base")
    pkg.OACNNs = base.OACNNs
    return importlib.import_module("pointcept.models.keypoint_oa_cnns")


def _train_step(model, data):
    model.train()
    model.reg_head[3].p = 0.0
    model.zero_grad()
    out = model(dict(data))
    out["loss"].backward()
    return out


def zero_bias(name):
    """Biases of a Linear straight in front of a batch-statistic BatchNorm: exact gradient zero, noise on both sides."""
    return name == "reg_head.0.bias" or (name.startswith("dec.") and name.endswith(("fuse.0.bias", "fuse.3.bias")))


# tolerances of tests/test_hip_keypoint_oacnns.py::test_train_step_vs_reference_golden
def check_step(loss, grads, bufs, ref_loss, ref_grads, ref_bufs, gmax):
    assert abs(loss - ref_loss) < 1e-4, (loss, ref_loss)
    for n, g in grads.items():
        r = ref_grads[n]
        scale = max(np.abs(r).max(), 1e-3 * gmax)
        err = np.abs(g - r).max() / scale
        assert err < (2e-3 if n.startswith("reg_head.") else 1e-2) or zero_bias(n), (n, err)
    for n, b in bufs.items():
        assert np.abs(b - ref_bufs[n]).max() / max(np.abs(ref_bufs[n]).max(), 1e-6) < 1e-4, n


def make_data():
    sys.path.insert(0, os.path.join(ROOT, "pointcept-keypointdetection_amd"))
    import ptv3_scenes as S
    batch = S.make_batch(SIZES, in_channels=4, extent=EXTENT, seed=23)
    grid = batch["grid_coord"].clone()
    grid[SIZES[0]:, 1] += 3          # the second scene does not start at the batch minimum on y
    data = {"grid_coord": grid, "feat": batch["feat"], "offset": batch["offset"], "coord": batch["coord"]}
    g = torch.Generator().manual_seed(5)
    data["target"] = torch.randn(len(SIZES) * 6, 3, generator=g) * 0.5
    data["scale"] = torch.rand(len(SIZES), generator=g) + 0.5
    return data


def main():
    sys.path.insert(0, HERE)
    kp = _load_reference()
    model = kp.KeypointOACNNs(**TINY_KW)
    print("tiny model:", sum(p.numel() for p in model.parameters()), "parameters,", len(model.state_dict()), "entries")
    sd0 = seeded_state_dict(model.state_dict())
    model.load_state_dict(sd0, strict=True)
    data = make_data()
    res = {"in_" + k: v.numpy() for k, v in data.items()}

    mods = dict(model.named_modules())
    taps, logits, hooks = {}, [], []
    for name in TAPS:
        hooks.append(mods[name].register_forward_hook(lambda m, i, o, name=name: taps.__setitem__(name, o)))
    hooks.append(mods[MIXED_BLOCK + ".fuse"].register_forward_pre_hook(
        lambda m, i: taps.__setitem__("mixed", i[0][:, i[0].shape[1] // 2:].detach().clone())))
    for name, m in mods.items():
        if ".weight." in name + ".":
            hooks.append(m.register_forward_hook(lambda m, i, o: logits.append(o.detach())))
    with torch.no_grad():
        out = model.eval()(dict(data))
    for h in hooks:
        h.remove()
    res["eval_pred"], res["eval_loss"] = out["pred"].numpy(), out["loss"].numpy()
    n_in = sum(SIZES)
    for name in TAPS:
        f = taps[name].features.detach().numpy()
        res["tap_" + name] = f[::TAP_STRIDE].copy() if len(f) == n_in else f.copy()
    res["tap_mixed"] = taps["mixed"].numpy()
    for i in range(4):
        sites = taps[f"enc.{i}"].indices.numpy().astype(np.int32)
        res[f"sites{i + 1}"] = sites
        assert set(sites[:, 0].tolist()) == set(range(len(SIZES))), f"a scene is empty at level {i + 1}"
    res["dropped"] = np.asarray(_Rec.dropped[:4], dtype=np.int32)
    print("sites without a parent per level", _Rec.dropped[:4], "rows per level", [len(res[f"sites{i + 1}"]) for i in range(4)])
    assert res["dropped"].sum() >= 1
    assert len(logits) == 5 * 3, len(logits)
    for p in logits:
        assert int((p == p.max()).sum()) == 1, "a p_l without a unique maximum"
    print(f"smallest cluster softmax mass S = {_Rec.smin:.3e}")
    assert _Rec.smin >= 1e-3, _Rec.smin

    out = _train_step(model, data)
    res["loss"] = out["loss"].detach().numpy()
    res["mean_dist"] = out["train/mean_dist"].numpy()
    res["kp_dist"] = np.array([out[f"train/kp{i}_dist"].item() for i in range(6)], dtype=np.float32)
    grads = {k: p.grad.detach().clone().numpy() for k, p in model.named_parameters()}
    assert all(np.abs(g).max() > 0 for k, g in grads.items() if not zero_bias(k))
    bufs = {k: b.detach().clone().numpy() for k, b in model.named_buffers() if "running" in k}
    for k, gr in grads.items():
        top = max(float(np.abs(gr).max()), 1e-30)
        res["grad_" + k] = (gr / top).astype(np.float16)
        res["gmax_" + k] = np.float32(top)
    res.update({"buf_" + k: b for k, b in bufs.items()})

    # the same step in float64: the fp32 step must sit within the GPU test's tolerances of it
    model64 = kp.KeypointOACNNs(**TINY_KW).double()
    model64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd0.items()}, strict=True)
    data64 = {k: (v.double() if v.is_floating_point() else v) for k, v in data.items()}
    out64 = _train_step(model64, data64)
    grads64 = {k: p.grad.numpy() for k, p in model64.named_parameters()}
    bufs64 = {k: b.detach().numpy() for k, b in model64.named_buffers() if "running" in k}
    gmax = max(float(np.abs(v).max()) for v in grads64.values())
    check_step(float(res["loss"]), grads, bufs, float(out64["loss"].detach()), grads64, bufs64, gmax)
    stored = {k: res["grad_" + k].astype(np.float32) * res["gmax_" + k] for k in grads}
    check_step(float(res["loss"]), stored, bufs, float(out64["loss"].detach()), grads64, bufs64, gmax)
    print("float64 step agrees; loss", float(res["loss"]), float(out64["loss"].detach()))

    path = os.path.join(HERE, "keypoint_oacnns_tiny.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("keypoint_oacnns_tiny.npz", size // 1024, "KiB; eval loss", float(res["eval_loss"]))

    from make_golden_keypoint_regression import write_listing
    from make_golden_swin3d import _cfg
    from pointcept.models.builder import MODELS
    fork = MODELS.build(_cfg("configs/my_dataset/keypoint_oa_cnns.py"))
    write_listing(fork, "state_dict_keypoint_oacnns_fork.txt")
    print("fork model:", sum(p.numel() for p in fork.parameters()), "parameters")


if __name__ == "__main__":
    main()
