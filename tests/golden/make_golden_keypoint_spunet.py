"""Build-container-only: run the reference's KeypointSparseUNet (pointcept/models/keypoint_sparse_unet.py over
sparse_unet/spconv_unet_v1m1_base.py, both imported in place) on the seeded two-scene batch of the OA-CNNs fixture and
store, in keypoint_spunet_tiny.npz (+ keypoint_spunet_tiny_grad{i}.npz, the gradients), its eval `pred` and loss,
feature taps (after conv_input, every enc[s], every dec[s]), the coarse site lists of every level, one training step
(loss, curves, every parameter gradient, the updated BatchNorm running statistics) and the eval `pred` and loss of the same model built with enc_mode=True.  Also lists the state_dict
of the model built from configs/my_dataset/keypoint_sparse_unet.py.

The CPU stand-ins for spconv / torch_geometric / timm are those of make_golden_keypoint_oacnns.py (parity with the real
packages unpinned); two more names the reference needs are added here: spconv.pytorch.SparseModule = nn.Module and
spconv.pytorch.Identity = nn.Identity, and SparseSequential hands the SparseConvTensor itself to the reference's own
SparseModules (BasicBlock) as spconv does.

Weights are not stored: seeded_state_dict() derives them from the key names and the GPU test calls the same function.
Gradients are stored as float16 of grad / max|grad| plus that maximum.

The script asserts what the tests rely on: no site is left without a parent (the +96 margin of sparse_shape), no scene
is empty at the deepest level, every training BatchNorm sees at least two rows, and the training step in float64 agrees
with the fp32 one within check_step's tolerances.  If an assertion fails, change the seed or the weight scale, not the
tolerance.
usage: python tests/golden/make_golden_keypoint_spunet.py"""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

from make_golden_keypoint_oacnns import (_install_standins, _Rec, seeded_state_dict, check_step, make_data,  # noqa: F401
                                         SIZES, TAP_STRIDE)

HERE = os.path.dirname(os.path.abspath(__file__))

TINY_KW = dict(num_keypoints=6, hidden_dim=32, in_channels=4, base_channels=16,
               channels=(16, 32, 32, 64, 64, 32, 16, 16), layers=(1, 2, 1, 1, 1, 1, 2, 1))
NUM_STAGES = 4
TAPS = ["conv_input"] + [f"enc.{i}" for i in range(NUM_STAGES)] + [f"dec.{i}" for i in reversed(range(NUM_STAGES))]
MARGIN = 96
GRAD_PART_BYTES = 900 * 1024     # raw float16 bytes per gradient file (compression gains little on them)


def load_golden(golden_dir):
    """{name: array} of keypoint_spunet_tiny.npz and exactly the `grad_parts` gradient files it names; a part that is
    missing, or a stale one beside them, is an error"""
    out = {}
    with np.load(os.path.join(golden_dir, "keypoint_spunet_tiny.npz")) as g:
        out.update({k: g[k] for k in g.files})
    want = [f"keypoint_spunet_tiny_grad{i}.npz" for i in range(int(out.pop("grad_parts")))]
    have = sorted(f for f in os.listdir(golden_dir) if f.startswith("keypoint_spunet_tiny_grad"))
    assert have == want, (have, want)
    for fname in want:
        with np.load(os.path.join(golden_dir, fname)) as g:
            assert not set(g.files) & set(out), fname
            out.update({k: g[k] for k in g.files})
    return out


def _load_reference():
    import ref_loader
    assert ref_loader.available()
    ref_loader.load()
    _install_standins()
    sp = sys.modules["spconv.pytorch"]
    sp.SparseModule = nn.Module
    sp.Identity = nn.Identity
    Base = sp.SparseSequential
    sparse_aware = (sp.SubMConv3d, sp.SparseConv3d, sp.SparseInverseConv3d)

    class SparseSequential(Base):
        """the reference's own SparseModules (BasicBlock) and nested SparseSequentials take the SparseConvTensor"""

        def forward(self, x):
            for m in self:
                own = type(m).__module__.startswith("pointcept.") or isinstance(m, SparseSequential)
                x = m(x) if own or isinstance(m, sparse_aware) else x.replace_feature(m(x.features))
            return x

    sp.SparseSequential = SparseSequential
    pkg = ref_loader._bare_pkg("pointcept.models.sparse_unet",
                               os.path.join(ref_loader.REF, "pointcept", "models", "sparse_unet"))
    base = importlib.import_module("pointcept.models.sparse_unet.spconv_unet_v1m1_base")
    pkg.SpUNetBase = base.SpUNetBase
    return importlib.import_module("pointcept.models.keypoint_sparse_unet")


def _train_step(model, data, rows=None):
    model.train()
    model.reg_head[3].p = 0.0
    model.zero_grad()
    hooks = []
    if rows is not None:
        for m in model.modules():
            if isinstance(m, nn.BatchNorm1d):
                hooks.append(m.register_forward_pre_hook(lambda m, i: rows.append(i[0].shape[0])))
    out = model(dict(data))
    out["loss"].backward()
    for h in hooks:
        h.remove()
    return out


def main():
    sys.path.insert(0, HERE)
    kp = _load_reference()
    model = kp.KeypointSparseUNet(**TINY_KW)
    print("tiny model:", sum(p.numel() for p in model.parameters()), "parameters,", len(model.state_dict()), "entries")
    sd0 = seeded_state_dict(model.state_dict())
    model.load_state_dict(sd0, strict=True)
    data = make_data()
    res = {"in_" + k: v.numpy() for k, v in data.items()}

    mods = dict(model.named_modules())
    taps, hooks = {}, []
    for name in TAPS:
        hooks.append(mods[name].register_forward_hook(lambda m, i, o, name=name: taps.__setitem__(name, o)))
    _Rec.dropped.clear()
    with torch.no_grad():
        out = model.eval()(dict(data))
    for h in hooks:
        h.remove()
    res["eval_pred"], res["eval_loss"] = out["pred"].numpy(), out["loss"].numpy()
    n_in = sum(SIZES)
    for name in TAPS:
        f = taps[name].features.detach().numpy()
        res["tap_" + name] = f[::TAP_STRIDE].copy() if len(f) == n_in else f.copy()
        print(f"tap {name}: {f.shape}, max|.| {np.abs(f).max():.3f}")
    for i in range(NUM_STAGES):
        sites = taps[f"enc.{i}"].indices.numpy().astype(np.int32)
        res[f"sites{i + 1}"] = sites
        assert set(sites[:, 0].tolist()) == set(range(len(SIZES))), f"a scene is empty at level {i + 1}"
    assert taps["conv_input"].spatial_shape == (data["grid_coord"].max(0).values + MARGIN).tolist()
    print("sites without a parent per level", _Rec.dropped[:NUM_STAGES], "rows per level",
          [len(res[f"sites{i + 1}"]) for i in range(NUM_STAGES)])
    assert len(_Rec.dropped) == NUM_STAGES and sum(_Rec.dropped) == 0, "the +96 margin must keep every parent"

    rows = []
    out = _train_step(model, data, rows)
    assert min(rows) >= 2, "a training BatchNorm saw fewer than two rows"
    res["loss"] = out["loss"].detach().numpy()
    res["mean_dist"] = out["train/mean_dist"].numpy()
    res["kp_dist"] = np.array([out[f"train/kp{i}_dist"].item() for i in range(6)], dtype=np.float32)
    grads = {k: p.grad.detach().clone().numpy() for k, p in model.named_parameters()}
    assert all(np.abs(g).max() > 0 for k, g in grads.items() if k != "reg_head.0.bias")
    bufs = {k: b.detach().clone().numpy() for k, b in model.named_buffers() if "running" in k}
    for k, gr in grads.items():
        top = max(float(np.abs(gr).max()), 1e-30)
        res["grad_" + k] = (gr / top).astype(np.float16)
        res["gmax_" + k] = np.float32(top)
    res.update({"buf_" + k: b for k, b in bufs.items()})

    # the same step in float64: the fp32 step must sit within the GPU test's tolerances of it
    model64 = kp.KeypointSparseUNet(**TINY_KW).double()
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

    # enc_mode=True: no decoder, the head on the per-scene mean of the deepest level; eval only
    enc = kp.KeypointSparseUNet(enc_mode=True, **TINY_KW)
    assert enc.dec is None and len(enc.up) == 0
    enc.load_state_dict(seeded_state_dict(enc.state_dict()), strict=True)
    with torch.no_grad():
        out = enc.eval()(dict(data))
    res["enc_mode_eval_pred"], res["enc_mode_eval_loss"] = out["pred"].numpy(), out["loss"].numpy()

    # the float16 gradients alone are 1.8 MB: they go, in parameter order, into as many keypoint_spunet_tiny_grad{i}.npz
    # as it takes to keep every file under 1 MiB (load_golden() puts the parts back together)
    parts, room = [{}], GRAD_PART_BYTES
    for k in grads:
        if res["grad_" + k].nbytes > room:
            parts.append({})
            room = GRAD_PART_BYTES
        parts[-1]["grad_" + k] = res.pop("grad_" + k)
        room -= parts[-1]["grad_" + k].nbytes
    for old in os.listdir(HERE):
        if old.startswith("keypoint_spunet_tiny_grad"):
            os.remove(os.path.join(HERE, old))
    res["grad_parts"] = np.int32(len(parts))
    files = [("keypoint_spunet_tiny.npz", res)] + [(f"keypoint_spunet_tiny_grad{i}.npz", q) for i, q in enumerate(parts)]
    for fname, content in files:
        np.savez_compressed(os.path.join(HERE, fname), **content)
        size = os.path.getsize(os.path.join(HERE, fname))
        assert size < (1 << 20), (fname, size)
        print(fname, size // 1024, "KiB")
    print("eval loss", float(res["eval_loss"]), "enc_mode eval loss", float(res["enc_mode_eval_loss"]))

    from make_golden_keypoint_regression import write_listing
    from make_golden_swin3d import _cfg
    from pointcept.models.builder import MODELS
    fork = MODELS.build(_cfg("configs/my_dataset/keypoint_sparse_unet.py"))
    write_listing(fork, "state_dict_keypoint_spunet_fork.txt")
    print("fork model:", sum(p.numel() for p in fork.parameters()), "parameters")


if __name__ == "__main__":
    main()
