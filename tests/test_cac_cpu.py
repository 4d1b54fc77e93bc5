"""CPU-side checks of the context-aware classifier: "CAC-v1m1" registered and built from both config dicts with the
reference's exact state_dict - and the float64 yardstick of the GPU tests (tests/cac_ref.py) pinned to the reference's
own outputs (tests/golden/cac_tiny.npz, written by tests/golden/make_golden_cac.py).

Tolerances: four times the fixture's fp32-vs-float64 gap of the same tensor (DESIGN.md sections 13 - 15); a gradient is
stored as float16 of grad / max|grad|, so it is also allowed the float16 step of its stored value."""
import copy
import os

import numpy as np
import pytest
import torch

import cac_ref as R
from make_golden_cac import load_golden, CONF, TEMP, LOSSES, NUM_CLASSES, SIZES, ONCE, ABSENT

_G = {}


def golden(golden_dir):
    if not _G:
        _G.update(load_golden(golden_dir))
    return _G


def head_sd(g, dtype=torch.float64):
    sd = {}
    for k in g:
        if k.startswith("sd_"):
            v = torch.from_numpy(g[k])
            sd[k[3:]] = v.to(dtype) if v.is_floating_point() else v
    return sd


def grad_tol(g, name):
    """elementwise tolerance of the stored gradient `name`: 4 x gap + the float16 step of the stored value"""
    stored = g["grad_" + name].astype(np.float64) * float(g["gmax_" + name])
    return stored, 4 * float(g["gap_grad_" + name]) + (2.0 ** -11 * np.abs(stored) + 2.0 ** -24 * float(g["gmax_" + name]))


def test_registered_and_exported():
    import pointcept.models as M
    assert M.MODELS.get("CAC-v1m1") is M.CACSegmentor


@pytest.mark.parametrize("name", ["CAC_SPUNET_SCANNET_CFG", "CAC_PTV2_SCANNET200_CFG"])
def test_config_builds(name, golden_dir):
    from pointcept.models import build_model
    from ptv3_hip import configs
    cfg = getattr(configs, name)
    keep = copy.deepcopy(cfg)
    model = build_model(cfg)
    assert cfg == keep
    c, k = cfg["backbone_out_channels"], cfg["num_classes"]
    sd = model.state_dict()
    head = {key: tuple(v.shape) for key, v in sd.items() if not key.startswith("backbone.")}
    assert head == {
        "seg_head.weight": (k, c), "seg_head.bias": (k,), "proj.0.weight": (2 * c, 2 * c), "proj.2.weight": (c, 2 * c),
        "proj.2.bias": (c,), "apd_proj.0.weight": (2 * c, 2 * c), "apd_proj.2.weight": (c, 2 * c),
        "apd_proj.2.bias": (c,), "feat_proj_layer.0.weight": (c, c), "feat_proj_layer.1.weight": (c,),
        "feat_proj_layer.1.bias": (c,), "feat_proj_layer.1.running_mean": (c,), "feat_proj_layer.1.running_var": (c,),
        "feat_proj_layer.1.num_batches_tracked": (), "feat_proj_layer.3.weight": (c, c), "feat_proj_layer.3.bias": (c,)}
    assert (model.cos_temp, model.conf_thresh, model.detach_pre_logits) == (15, cfg["conf_thresh"], True)
    assert len(model.criteria.criteria) == 2
    if name == "CAC_SPUNET_SCANNET_CFG":
        ref = open(os.path.join(golden_dir, "state_dict_cac_spunet_scannet.txt")).read().strip().split("\n")
        assert [f"{key} {tuple(v.shape)} {v.dtype}" for key, v in sd.items()] == ref


def test_reference_defaults():
    from pointcept.models import build_model
    from make_golden_cac import TINY_BACKBONE
    m = build_model(dict(type="CAC-v1m1", num_classes=7, backbone_out_channels=16, backbone=TINY_BACKBONE))
    assert (m.cos_temp, m.main_weight, m.pre_weight, m.pre_self_weight, m.kl_weight, m.conf_thresh,
            m.detach_pre_logits) == (15, 1, 1, 1, 1, 0, False)


def test_fixture_is_what_the_tests_assume(golden_dir):
    g = golden(golden_dir)
    seg, off = g["in_segment"], g["in_offset"]
    assert off.tolist() == np.cumsum(SIZES).tolist()
    assert int((seg[off[0]:off[1]] == ONCE).sum()) == 1 and not (seg == ABSENT).any() and (seg == -1).any()
    for feat in ("eval_feat", "train_feat"):
        sd = head_sd(g)
        logits = torch.from_numpy(g[feat]).double() @ sd["seg_head.weight"].t() + sd["seg_head.bias"]
        top = torch.softmax(logits, 1).max(1)[0]
        assert ((top - CONF).abs() >= 0.9e-3).all()
        assert 0.05 < float((top >= CONF).double().mean()) < 0.95


def test_yardstick_reproduces_reference_eval(golden_dir):
    g = golden(golden_dir)
    sd = head_sd(g)
    feat, offset = torch.from_numpy(g["eval_feat"]).double(), torch.from_numpy(g["in_offset"])
    seg_logits, refined = R.head_eval(feat, sd, offset, CONF, TEMP)
    err = (refined - torch.from_numpy(g["eval_seg_logits"]).double()).abs().max().item()
    print("eval seg_logits: err", err, "gap", float(g["gap_eval_seg_logits"]))
    assert err <= 4 * float(g["gap_eval_seg_logits"])
    loss = R.cross_entropy(seg_logits, torch.from_numpy(g["in_segment"])).item()
    print("eval loss: err", abs(loss - float(g["eval_loss"])), "gap", float(g["gap_eval_loss"]))
    assert abs(loss - float(g["eval_loss"])) <= 4 * float(g["gap_eval_loss"])


def test_yardstick_reproduces_reference_training_step(golden_dir):
    g = golden(golden_dir)
    sd = head_sd(g)
    feat, offset = torch.from_numpy(g["train_feat"]).double(), torch.from_numpy(g["in_offset"])
    out = R.train_step(feat, sd, offset, torch.from_numpy(g["in_segment"]), CONF, TEMP)
    for k in LOSSES:
        err, gap = abs(out[k].item() - float(g["train_" + k])), float(g["gap_train_" + k])
        print(k, "err", err, "gap", gap)
        assert err <= 4 * gap, k
    err = (out["dfeat"] - torch.from_numpy(g["train_dfeat"]).double()).abs().max().item()
    print("dfeat err", err, "gap", float(g["gap_train_dfeat"]))
    assert err <= 4 * float(g["gap_train_dfeat"])
    for name in R.PARAMS:
        stored, tol = grad_tol(g, name)
        err = np.abs(out["d" + name].numpy() - stored)
        print(name, "err", err.max(), "gap", float(g["gap_grad_" + name]))
        assert (err <= tol).all(), name
    mean, var, tracked = out["stats"]
    assert tracked == len(SIZES) + 1 == int(g["buf_feat_proj_layer.1.num_batches_tracked"])
    for got, key in ((mean, "running_mean"), (var, "running_var")):
        err = (got - torch.from_numpy(g["buf_feat_proj_layer.1." + key]).double()).abs().max().item()
        assert err <= 4 * float(g["gap_buf_feat_proj_layer.1." + key]), key


def test_composed_path_is_the_yardsticks_arithmetic():
    """the torch functions the model's composed path is made of, against cac_ref in float64"""
    from pointcept.models.context_aware_classifier import context_aware_classifier_v1m1_base as M
    gen = torch.Generator().manual_seed(0)
    n, k, c = 300, NUM_CLASSES, 8
    x = torch.randn(n, c, generator=gen, dtype=torch.float64)
    logits = torch.randn(n, k, generator=gen, dtype=torch.float64) * 4
    labels = torch.randint(-1, k - 1, (n,), generator=gen)
    offset = torch.tensor([100, 300])
    want, _ = R.proto_softmax(x, logits, offset, 0.6)
    got = torch.stack([M.softmax_proto_torch(x[s:e], logits[s:e], 0.6) for s, e in R.scenes(offset)])
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-14)
    want, count = R.proto_label(x, labels, k)
    got, got_count = M.label_proto_torch(x, labels, k)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-14) and torch.equal(got_count, count) and count[k - 1] == 0
    soft = torch.randn(n, k, generator=gen, dtype=torch.float64) * 3
    assert abs(M.distill_loss_torch(logits, soft, labels).item() - R.distill_loss(logits, soft, labels).item()) < 1e-12
    none = torch.full((n,), -1)
    assert M.distill_loss_torch(logits, soft, none).item() == 0.0 == R.distill_loss(logits, soft, none).item()
    assert torch.allclose(M.get_pred(x, want) * 15, R.cos_logits(x, want, None, 15.0), rtol=1e-12, atol=1e-14)


def test_distill_yardstick_is_the_references_loop():
    """cac_ref.distill_loss against get_distill_loss written as the reference writes it (unique() and a loop over the
    classes present), in float64"""
    gen = torch.Generator().manual_seed(1)
    n, k = 200, 6
    pred = torch.randn(n, k, generator=gen, dtype=torch.float64) * 3
    soft = torch.randn(n, k, generator=gen, dtype=torch.float64) * 3
    target = torch.randint(-1, k - 1, (n,), generator=gen)
    loss_i, ent, valid, _ = R.distill_rows(pred, soft, target)
    ent = ent * valid.double()
    terms = []
    for y in target.unique().tolist():
        if y == -1:
            continue
        m = (target == y).double() * ent
        terms.append((loss_i * m).sum() / (m.sum() + 1e-4))
    want = sum(terms) / (len(terms) + 1e-4)
    assert abs(R.distill_loss(pred, soft, target).item() - want.item()) < 1e-12


def test_wiring_stays_inside_the_measured_widths():
    from pointcept.models.context_aware_classifier.context_aware_classifier_v1m1_base import wired
    for kernel in ("proto_softmax", "proto_label", "cos_logits"):
        for training in (True, False):
            assert not wired(kernel, 20, 97, training) and not wired(kernel, 20, 128, training)
    assert wired("distill", 200, 128, True)
    assert wired("proto_softmax", 100, 96, True) and not wired("proto_softmax", 200, 48, True)
    assert wired("proto_softmax", 200, 48, False) and not wired("proto_softmax", 200, 96, False)
    assert wired("proto_label", 100, 48, True) and not wired("proto_label", 100, 96, True)
    assert wired("cos_logits", 200, 48, False) and not wired("cos_logits", 100, 96, False)
    assert not wired("cos_logits", 20, 48, True)
