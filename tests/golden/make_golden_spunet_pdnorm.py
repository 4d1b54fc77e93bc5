"""Build-container-only: run the reference's SpUNet-v1m3 (pointcept/models/sparse_unet/spconv_unet_v1m3_pdnorm.py,
imported in place with the CPU stand-ins of make_golden_keypoint_oacnns.py / make_golden_keypoint_spunet.py) under the
reference's "PPT-v1m2" (decoupled heads, no CLIP; point_prompt_training_v1m2_decoupled.py), so that embedding_table.weight
receives the context's gradient, on the seeded two-scene batch of the OA-CNNs fixture with per-condition labels.

Tiny backbone: in_channels=4, base_channels=16, channels=(16, 32, 32, 64, 64, 32, 16, 16), layers=(1, 2, 1, 1, 1, 1, 2, 1),
context_channels=24, conditions ("A", "B", "C"), zero_init=False; heads of 5 / 7 / 3 classes.  Three variants:
  "affine"    norm_adaptive=True,  norm_affine=True,  norm_decouple=True    (the full record)
  "noaffine"  norm_adaptive=True,  norm_affine=False, norm_decouple=True
  "plain"     norm_adaptive=False, norm_affine=True,  norm_decouple=False
Stored in spunet_pdnorm_{variant}.npz (+ spunet_pdnorm_affine_grad{i}.npz):
  affine: the inputs; for "B" and "C" the eval seg_logits, loss and the nine feature taps (conv_input, every enc, every
    dec; the taps on the input sites keep every TAP_STRIDE-th row); the coarse site lists; for "B" the input and output of
    one PDBatchNorm (PD_TAP) in eval and in training; one training step under "B": loss, every parameter gradient as
    float16 of grad / max|grad| plus that maximum, the names without a gradient (`nograd`), every running buffer
    afterwards, num_batches_tracked included.
  noaffine, plain: eval seg_logits and loss under "B", the training loss, the gradients of the stem, of the last decoder
    block and (noaffine) of embedding_table.weight.
Weights are not stored: pdnorm_state_dict() derives them from the key names (seeded_state_dict, then perturb_bn) and the
tests call the same function.

The script asserts what the tests rely on: no site without a parent, no empty scene at the deepest level, every training
BatchNorm sees at least two rows, and the float64 step agrees with the fp32 one within check_step's tolerances.
Also lists the state_dict of the reference class built from configs/scannet/semseg-ppt-v1m1-0-sc-st-spunet.py.
usage: python tests/golden/make_golden_spunet_pdnorm.py"""
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))

CONDITIONS = ("A", "B", "C")
NUM_CLASSES = (5, 7, 3)
EVAL_CONDITIONS, TRAIN_CONDITION = ("B", "C"), "B"
CONTEXT_CHANNELS = 24
NUM_STAGES = 4
TAPS = ["conv_input"] + [f"enc.{i}" for i in range(NUM_STAGES)] + [f"dec.{i}" for i in reversed(range(NUM_STAGES))]
PD_TAP = "backbone.enc.1.block0.bn1"
TAP_STRIDE = 2
MARGIN = 96
GRAD_PART_BYTES = 900 * 1024
VARIANTS = {"affine": dict(norm_adaptive=True, norm_affine=True, norm_decouple=True),
            "noaffine": dict(norm_adaptive=True, norm_affine=False, norm_decouple=True),
            "plain": dict(norm_adaptive=False, norm_affine=True, norm_decouple=False)}
SMALL_GRADS = ("backbone.conv_input.", "backbone.dec.0.block0.", "embedding_table.")
HEAD_PREFIX = "seg_heads."


def tiny_backbone(variant):
    return dict(type="SpUNet-v1m3", in_channels=4, num_classes=0, base_channels=16, context_channels=CONTEXT_CHANNELS,
                channels=(16, 32, 32, 64, 64, 32, 16, 16), layers=(1, 2, 1, 1, 1, 1, 2, 1), conditions=CONDITIONS,
                zero_init=False, **VARIANTS[variant])


def tiny_kw(variant):
    return dict(backbone=tiny_backbone(variant), backbone_out_channels=16, context_channels=CONTEXT_CHANNELS,
                conditions=CONDITIONS, num_classes=NUM_CLASSES,
                criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)])


def load_golden(golden_dir, variant):
    """{name: array} of spunet_pdnorm_{variant}.npz and exactly the `grad_parts` gradient files it names"""
    out = {}
    with np.load(os.path.join(golden_dir, f"spunet_pdnorm_{variant}.npz")) as g:
        out.update({k: g[k] for k in g.files})
    want = [f"spunet_pdnorm_{variant}_grad{i}.npz" for i in range(int(out.pop("grad_parts")))]
    have = sorted(f for f in os.listdir(golden_dir) if f.startswith(f"spunet_pdnorm_{variant}_grad"))
    assert have == want, (have, want)
    for fname in want:
        with np.load(os.path.join(golden_dir, fname)) as g:
            assert not set(g.files) & set(out), fname
            out.update({k: g[k] for k in g.files})
    return out


def pdnorm_state_dict(model):
    """Loads the seeded weights into `model` (the reference class or the library's) and returns its state_dict."""
    from make_golden_keypoint_oacnns import seeded_state_dict
    from make_golden_keypoint_regression import perturb_bn
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    with torch.no_grad():
        perturb_bn(model)
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def make_data():
    """the OA-CNNs fixture's batch with one label vector per condition (about a tenth -1)"""
    from make_golden_keypoint_oacnns import make_data as base
    data = {k: v for k, v in base().items() if k in ("grid_coord", "feat", "offset", "coord")}
    g = torch.Generator().manual_seed(1071)
    n = data["feat"].shape[0]
    for cond, k in zip(CONDITIONS, NUM_CLASSES):
        seg = torch.randint(0, k, (n,), generator=g)
        seg[torch.rand(n, generator=g) < 0.1] = -1
        data["segment_" + cond] = seg
    return data


def batch_of(data, cond, with_segment=True, cast=None):
    out = {k: v for k, v in data.items() if not k.startswith("segment_")}
    if cast is not None:
        out = {k: (v.to(cast) if v.is_floating_point() else v) for k, v in out.items()}
    if with_segment:
        out["segment"] = data["segment_" + cond]
    out["condition"] = [cond]
    return out


def check_step(loss, grads, bufs, ref_loss, ref_grads, ref_bufs, gmax):
    """make_golden_keypoint_oacnns.check_step's numbers with this model's head prefix"""
    assert abs(loss - ref_loss) < 1e-4, (loss, ref_loss)
    for n, g in grads.items():
        r = np.asarray(ref_grads[n], dtype=np.float64)
        scale = max(np.abs(r).max(), 1e-3 * gmax)
        err = np.abs(np.asarray(g, dtype=np.float64) - r).max() / scale
        assert err < (2e-3 if n.startswith(HEAD_PREFIX) else 1e-2), (n, err)
    for n, b in bufs.items():
        r = np.asarray(ref_bufs[n], dtype=np.float64)
        assert np.abs(np.asarray(b, dtype=np.float64) - r).max() / max(np.abs(r).max(), 1e-6) < 1e-4, n


def _load_reference():
    from make_golden_keypoint_spunet import _load_reference as load_spunet
    load_spunet()            # the stand-ins, SparseModule / Identity, the SparseSequential that hands lists through
    importlib.import_module("pointcept.models.sparse_unet.spconv_unet_v1m3_pdnorm")
    return importlib.import_module("pointcept.models.point_prompt_training.point_prompt_training_v1m2_decoupled")


def _eval(model, data, cond, cast=None, taps=None, pd=None):
    mods = dict(model.named_modules())
    hooks = []
    if taps is not None:
        for name in TAPS:
            hooks.append(mods["backbone." + name].register_forward_hook(
                lambda m, i, o, name=name: taps.__setitem__(name, o[0] if isinstance(o, (tuple, list)) else o)))
    if pd is not None:
        hooks.append(mods[PD_TAP].register_forward_hook(
            lambda m, i, o: pd.update(pd_in=i[0].detach().clone(), pd_out=o.detach().clone())))
    with torch.no_grad():
        out = model.eval()(batch_of(data, cond, cast=cast))
    for h in hooks:
        h.remove()
    assert sorted(out.keys()) == ["loss", "seg_logits"]
    return out


def _train_step(model, data, cast=None, rows=None, pd=None):
    model.train()
    model.zero_grad()
    hooks = []
    if rows is not None:
        for m in model.modules():
            if isinstance(m, nn.BatchNorm1d):
                hooks.append(m.register_forward_pre_hook(lambda m, i: rows.append(i[0].shape[0])))
    if pd is not None:
        hooks.append(dict(model.named_modules())[PD_TAP].register_forward_hook(
            lambda m, i, o: pd.update(pd_in=i[0].detach().clone(), pd_out=o.detach().clone())))
    out = model(batch_of(data, TRAIN_CONDITION, cast=cast))
    out["loss"].backward()
    for h in hooks:
        h.remove()
    grads = {k: p.grad.detach().clone().numpy() for k, p in model.named_parameters() if p.grad is not None}
    nograd = [k for k, p in model.named_parameters() if p.grad is None]
    bufs = {k: b.detach().clone().numpy() for k, b in model.named_buffers()
            if "running" in k or k.endswith("num_batches_tracked")}
    return float(out["loss"].detach()), grads, nograd, bufs


def _one(cls, variant, data):
    from make_golden_keypoint_oacnns import _Rec
    kw = tiny_kw(variant)
    kw["backbone"] = sys.modules["addict"].Dict(kw["backbone"])
    model = cls(**kw)
    sd0 = pdnorm_state_dict(model)
    full = variant == "affine"
    res = {}
    n_in = data["feat"].shape[0]
    n_pd = sum(type(m).__name__ == "PDBatchNorm" for m in model.modules())
    print(f"{variant}: {len(sd0)} entries, {n_pd} PDBatchNorm")
    for cond in EVAL_CONDITIONS if full else (TRAIN_CONDITION,):
        taps, pd = ({}, {}) if full else (None, None)
        _Rec.dropped.clear()
        out = _eval(model, data, cond, taps=taps, pd=pd if cond == TRAIN_CONDITION else None)
        res[f"eval_seg_logits_{cond}"], res[f"eval_loss_{cond}"] = out["seg_logits"].numpy(), out["loss"].numpy()
        if not full:
            continue
        assert len(_Rec.dropped) == NUM_STAGES and sum(_Rec.dropped) == 0, "the +96 margin must keep every parent"
        for name in TAPS:
            f = taps[name].features.detach().numpy()
            res[f"tap_{cond}_{name}"] = f[::TAP_STRIDE].copy() if len(f) == n_in else f.copy()
        if cond == TRAIN_CONDITION:
            for i in range(NUM_STAGES):
                sites = taps[f"enc.{i}"].indices.numpy().astype(np.int32)
                res[f"sites{i + 1}"] = sites
                assert set(sites[:, 0].tolist()) == set(range(len(data["offset"]))), f"a scene is empty at level {i + 1}"
            assert list(taps["conv_input"].spatial_shape) == (data["grid_coord"].max(0).values + MARGIN).tolist()
            res["eval_pd_in"], res["eval_pd_out"] = pd["pd_in"].numpy(), pd["pd_out"].numpy()
    rows, pd = [], {}
    loss, grads, nograd, bufs = _train_step(model, data, rows=rows, pd=pd)
    assert min(rows) >= 2, "a training BatchNorm saw fewer than two rows"
    print(f"  smallest training BatchNorm batch {min(rows)} rows, {len(nograd)} parameters without a gradient")
    model64 = cls(**kw).double()
    model64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd0.items()}, strict=True)
    loss64, grads64, nograd64, bufs64 = _train_step(model64, data, cast=torch.float64)
    assert nograd == nograd64
    gmax = max(float(np.abs(v).max()) for v in grads64.values())
    check_step(loss, grads, bufs, loss64, grads64, bufs64, gmax)
    res["train_loss"] = np.float32(loss)
    keep = list(grads) if full else [k for k in grads if k.startswith(SMALL_GRADS)]
    stored = {}
    for k in keep:
        top = max(float(np.abs(grads[k]).max()), 1e-30)
        res["grad_" + k] = (grads[k] / top).astype(np.float16)
        res["gmax_" + k] = np.float32(top)
        stored[k] = res["grad_" + k].astype(np.float32) * res["gmax_" + k]
    check_step(loss, stored, {}, loss64, grads64, bufs64, gmax)
    res["gmax_all"] = np.float32(gmax)
    print(f"  float64 step agrees; loss {loss:.6f} / {loss64:.6f}; eval loss",
          [float(res[f"eval_loss_{c}"]) for c in (EVAL_CONDITIONS if full else (TRAIN_CONDITION,))])
    parts = [{}]
    if full:
        res.update({"in_" + k: v.numpy() for k, v in data.items()})
        res["nograd"] = np.array(nograd)
        res["train_pd_in"], res["train_pd_out"] = pd["pd_in"].numpy(), pd["pd_out"].numpy()
        res.update({"buf_" + k: b for k, b in bufs.items()})
        res["state_keys"] = np.array(list(sd0))
        # the float16 gradients, in parameter order, into as many files as keep each under 1 MiB
        room = GRAD_PART_BYTES
        for k in keep:
            if res["grad_" + k].nbytes > room:
                parts.append({})
                room = GRAD_PART_BYTES
            parts[-1]["grad_" + k] = res.pop("grad_" + k)
            room -= parts[-1]["grad_" + k].nbytes
    else:
        parts = []
    for old in os.listdir(HERE):
        if old.startswith(f"spunet_pdnorm_{variant}_grad"):
            os.remove(os.path.join(HERE, old))
    res["grad_parts"] = np.int32(len(parts))
    files = [(f"spunet_pdnorm_{variant}.npz", res)] + [(f"spunet_pdnorm_{variant}_grad{i}.npz", q)
                                                       for i, q in enumerate(parts)]
    for fname, content in files:
        np.savez_compressed(os.path.join(HERE, fname), **content)
        size = os.path.getsize(os.path.join(HERE, fname))
        assert size < (1 << 20), (fname, size)
        print("  ", fname, size // 1024, "KiB")


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    v1m2 = _load_reference()
    data = make_data()
    for variant in VARIANTS:
        _one(v1m2.PointPromptTraining, variant, data)

    from make_golden_ppt import _install_clip_stub
    from make_golden_keypoint_regression import write_listing
    from make_golden_swin3d import _cfg
    _install_clip_stub(512)                 # ViT-B/16
    v1m1 = importlib.import_module("pointcept.models.point_prompt_training.point_prompt_training_v1m1_language_guided")
    cfg = _cfg("configs/scannet/semseg-ppt-v1m1-0-sc-st-spunet.py")
    cfg["backbone"] = sys.modules["addict"].Dict(cfg["backbone"])
    cfg.pop("type")
    write_listing(v1m1.PointPromptTraining(**cfg), "state_dict_ppt_spunet_scannet.txt")


if __name__ == "__main__":
    main()
