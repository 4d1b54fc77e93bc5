"""CPU-side checks of Point Prompt Training: "PPT-v1m1" / "PPT-v1m2" and PDNorm registered and built with the reference's
exact state_dict, the collapse of the language-guided head against the reference formula in float64, the float64
yardstick of the GPU tests (tests/ppt_ref.py) pinned to the reference's own outputs (tests/golden/ppt_tiny_*.npz, written
by tests/golden/make_golden_ppt.py), and the refusals.

Tolerances against the fixture: four times its fp32-vs-float64 gap of the same tensor, with a floor of one fp32 rounding
at the tensor's scale (DESIGN.md sections 13 - 15)."""
import copy
import os

import numpy as np
import pytest
import torch

import ppt_ref as R
from make_golden_ppt import (load_golden, ppt_state_dict, tiny_kw, tiny_backbone, CONDITIONS, VALID, EVAL_CONDITIONS,
                             TRAIN_CONDITION, CHANNELS, WIDTH, BN_TAP, LN_TAP)

ULP = 2.0 ** -23
_G = {}


def golden(golden_dir, run="v1m1"):
    if run not in _G:
        _G[run] = load_golden(golden_dir, run)
    return _G[run]


def _close(name, got, want, gap):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    floor = ULP * np.abs(want).max()
    print(f"{name}: err {err.max():.3e} gap {gap:.3e} floor {floor:.3e}")
    assert (err <= max(4 * gap, floor)).all(), (name, err.max(), gap)


def _build(run):
    from pointcept.models import build_model
    from pointcept.models.point_prompt_training import point_prompt_training_v1m1_language_guided as V
    V.CLIP_TEXT_WIDTH.setdefault("stub", WIDTH)          # the fixture's text encoder: width 40
    return build_model(dict(type="PPT-v1m2" if run == "v1m2" else "PPT-v1m1", **tiny_kw(run)))


def test_registered_and_exported():
    import pointcept.models as M
    from pointcept.models.point_prompt_training import PDNorm, PointPromptTraining, PointPromptTrainingDecoupled
    assert M.MODELS.get("PPT-v1m1") is PointPromptTraining and M.MODELS.get("PPT-v1m2") is PointPromptTrainingDecoupled
    assert M.MODULES.get("PDNorm") is PDNorm and issubclass(PDNorm, M.PointModule)


def test_scannet_config_state_dict_equals_the_listing(golden_dir):
    from pointcept.models import build_model
    from ptv3_hip.configs import PPT_PTV3_SCANNET_CFG
    keep = copy.deepcopy(PPT_PTV3_SCANNET_CFG)
    model = build_model(PPT_PTV3_SCANNET_CFG)
    assert PPT_PTV3_SCANNET_CFG == keep
    with open(os.path.join(golden_dir, "state_dict_ppt_ptv3_scannet.txt")) as f:
        want = [line.rstrip("\n") for line in f]
    got = [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]
    assert sorted(got) == sorted(want)
    p = model.logit_scale
    assert not p.requires_grad and abs(p.item() - np.log(100.0)) < 1e-6 and not model.class_embedding.any()
    # a reference checkpoint loads strictly and fills the embedding
    sd = {k: torch.zeros_like(v) for k, v in model.state_dict().items()}
    assert not model._filled
    model.load_state_dict(sd, strict=True)
    assert model._filled


def test_tiny_v1m2_config_builds():
    from pointcept.models import build_model
    from ptv3_hip.configs import PPT_V1M2_TINY_CFG
    model = build_model(PPT_V1M2_TINY_CFG)
    head = {k: tuple(v.shape) for k, v in model.state_dict().items() if not k.startswith("backbone.")}
    assert head == {"embedding_table.weight": (3, 256), "seg_heads.0.weight": (5, 16), "seg_heads.0.bias": (5,),
                    "seg_heads.1.weight": (7, 16), "seg_heads.1.bias": (7,), "seg_heads.2.weight": (3, 16),
                    "seg_heads.2.bias": (3,)}


@pytest.mark.parametrize("run", ["v1m1", "v1m1_adaptive", "v1m2"])
def test_tiny_models_take_the_seeded_weights_and_pdnorm_keys(golden_dir, run):
    g = golden(golden_dir, run)
    model = _build(run)
    sd = ppt_state_dict(model, g.get("sd_class_embedding"), g.get("sd_logit_scale"))
    stem = {k for k in sd if k.startswith(BN_TAP + ".")}
    want = {f"{BN_TAP}.norm.{i}.{p}" for i in range(3)
            for p in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    if run == "v1m1_adaptive":
        want |= {BN_TAP + ".modulation.1.weight", BN_TAP + ".modulation.1.bias"}
    assert stem == want
    # every stored gradient and buffer names a parameter / buffer of the library's model, and nothing is missing
    params = dict(model.named_parameters())
    stored = {k[len("gmax_"):] for k in g if k.startswith("gmax_")} | set(g["nograd"].tolist())
    assert stored == set(params)
    assert {k[len("buf_"):] for k in g if k.startswith("buf_")} == {
        k for k, _ in model.named_buffers() if k.endswith("running_mean") or k.endswith("running_var")}


def _spectrum(d, c, cond, seed):
    g = torch.Generator().manual_seed(seed)
    u, _ = torch.linalg.qr(torch.randn(d, c, generator=g, dtype=torch.float64))
    v, _ = torch.linalg.qr(torch.randn(c, c, generator=g, dtype=torch.float64))
    sv = torch.logspace(0, -np.log10(cond), c, dtype=torch.float64)
    return (u * sv) @ v.t(), v


@pytest.mark.parametrize("bias", [False, True])
def test_collapse_equals_the_reference_formula_in_float64(bias):
    """cond(W) = 1000, a quarter of the rows along the four weakest singular directions of W, s = 100"""
    from ptv3_hip import ops
    c, d, k, n = 64, 512, 20, 4000
    W, v = _spectrum(d, c, 1000.0, 5)
    g = torch.Generator().manual_seed(6)
    b = torch.randn(d, generator=g, dtype=torch.float64) if bias else None
    E = torch.randn(36, d, generator=g, dtype=torch.float64)
    E = E / E.norm(dim=1, keepdim=True)
    valid = list(range(0, 36, 2))[:k] + [35, 33]
    x = torch.randn(n, c, generator=g, dtype=torch.float64)
    x[: n // 4] = torch.randn(n // 4, 4, generator=g, dtype=torch.float64) @ v[:, -4:].t()
    ref = R.head(x, W, b, E, valid, np.log(100.0))
    B, bb, beta, s = ops.ppt_head_collapse(W, b, E[valid], torch.tensor(np.log(100.0), dtype=torch.float64),
                                           dtype=torch.float64)
    assert tuple(B.shape) == (c, c + len(valid)) and tuple(bb.shape) == (c + len(valid),) and abs(s - 100.0) < 1e-9
    assert (beta == 0.0) if not bias else beta > 0
    y = x @ B + bb
    got = s * y[:, c:] / torch.sqrt((y[:, :c] ** 2).sum(1, keepdim=True) + beta)
    rel = ((got - ref).abs().max() / ref.abs().max()).item()
    print("relative error", rel)
    assert rel <= 1e-12
    # the operands the kernel takes are these, rounded once
    B32, b32, beta32, s32 = ops.ppt_head_collapse(W, b, E[valid], torch.tensor(np.log(100.0), dtype=torch.float64))
    assert B32.dtype == torch.float32 and torch.equal(B32, B.float()) and torch.equal(b32, bb.float())
    assert beta32 == beta and s32 == s


@pytest.mark.parametrize("run", ["v1m1", "v1m1_adaptive"])
def test_ppt_ref_head_reproduces_the_fixture(golden_dir, run):
    g = golden(golden_dir, run)
    sd = ppt_state_dict(_build(run), g["sd_class_embedding"], g["sd_logit_scale"])
    for cond in EVAL_CONDITIONS:
        valid = VALID[CONDITIONS.index(cond)]
        feat = torch.from_numpy(g[f"eval_feat_{cond}"]).double()
        got = R.head(feat, sd["proj_head.weight"].double(), sd["proj_head.bias"].double(),
                     sd["class_embedding"].double(), valid, float(sd["logit_scale"]))
        assert tuple(got.shape) == (feat.shape[0], len(valid))
        _close(f"seg_logits {cond}", got.numpy(), g[f"eval_seg_logits_{cond}"], float(g[f"gap_eval_seg_logits_{cond}"]))


@pytest.mark.parametrize("run", ["v1m1", "v1m1_adaptive"])
def test_ppt_ref_pdnorm_reproduces_the_fixture(golden_dir, run):
    g = golden(golden_dir, run)
    sd = ppt_state_dict(_build(run), g["sd_class_embedding"], g["sd_logit_scale"])
    index = CONDITIONS.index(TRAIN_CONDITION)
    context = sd["embedding_table.weight"][index: index + 1].double()
    for tap, kind, key in ((BN_TAP, "bn", "pdn_bn"), (LN_TAP, "ln", "pdn_ln")):
        params = [{p: sd[f"{tap}.norm.{i}.{p}"].double() for p in ("weight", "bias", "running_mean", "running_var")
                   if f"{tap}.norm.{i}.{p}" in sd} for i in range(3)]
        mod = None
        if run == "v1m1_adaptive":
            mod = (sd[tap + ".modulation.1.weight"].double(), sd[tap + ".modulation.1.bias"].double())
        for mode in ("eval", "train") if kind == "bn" else ("eval",):
            x = torch.from_numpy(g[f"{mode}_{key}_in"]).double()
            got = R.pdnorm(x, kind, params, index, training=mode == "train", context=context, modulation=mod)
            gap = float(g[f"gap_{mode}_{key}_out"]) + float(g[f"gap_{mode}_{key}_in"])
            _close(f"{mode} {key}", got.numpy(), g[f"{mode}_{key}_out"], gap)
            other = R.pdnorm(x, kind, params, (index + 1) % 3, training=False, context=context, modulation=mod)
            assert (other - got).abs().max() > 1e-3          # the conditions' norms differ


def test_refusals():
    from pointcept.models import build_model
    with pytest.raises(ValueError, match="decouple"):
        build_model(dict(tiny_backbone(False), pdnorm_decouple=False))
    from pointcept.models.point_prompt_training import PDNorm
    from pointcept.models.utils.hip_layers import LayerNorm
    with pytest.raises(ValueError, match="decouple"):
        PDNorm(16, LayerNorm, decouple=False)
    # pdnorm_affine=False builds (it runs composed)
    plain = build_model(dict(tiny_backbone(False), pdnorm_affine=False))
    keys = plain.embedding.state_dict().keys()
    assert "stem.norm.norm.0.running_mean" in keys and "stem.norm.norm.0.weight" not in keys

    class Features(torch.nn.Module):
        def forward(self, data_dict):
            return torch.zeros(4, CHANNELS)

    model = _build("v1m1")
    assert tuple(model.class_embedding.shape) == (9, WIDTH)
    data = dict(coord=torch.zeros(4, 3), condition=["B"])
    model.backbone = Features()
    with pytest.raises(RuntimeError, match="load_state_dict.*set_class_embedding"):
        model(dict(data))
    model.set_class_embedding(torch.randn(*model.class_embedding.shape))
    assert model._filled and torch.allclose(model.class_embedding.norm(dim=1), torch.ones(9))
    with pytest.raises(KeyError, match="condition"):
        model(dict(data, condition=["ScanNet"]))
    with pytest.raises(ValueError):
        model.set_class_embedding(torch.zeros(3, 3))


def test_unknown_clip_model_without_clip_is_refused():
    from pointcept.models import build_model
    with pytest.raises(KeyError, match="CLIP_TEXT_WIDTH"):
        build_model(dict(type="PPT-v1m1", **dict(tiny_kw("v1m1"), clip_model="RN50x64")))


def test_ptv3_plus_still_raises():
    from pointcept.models import build_model
    from ptv3_hip.configs import TINY_CFG
    with pytest.raises(NotImplementedError):
        build_model(dict(type="PT-v3m1-Plus", **dict(TINY_CFG, pdnorm_bn=True)))
