"""CPU-side checks of DefaultClassifier, PigBodyRegressor and RegressionL1Loss: registered, built from the fork config
with the reference's exact state_dict, refusing to run without a GPU - and the float64 yardstick of the GPU tests
(tests/cls_head_ref.py) pinned to the reference's own outputs (tests/golden/body_regressor_tiny.npz)."""
import copy
import os

import numpy as np
import pytest
import torch


def test_names_registered():
    from pointcept.models import MODELS
    from pointcept.models.losses import LOSSES
    for name in ("DefaultClassifier", "PigBodyRegressor"):
        assert MODELS.get(name) is not None, name
    assert LOSSES.get("RegressionL1Loss") is not None


def test_fork_config_builds_with_reference_state_dict(golden_dir):
    """configs/my_dataset/ptv3_weight.py through the registry: keys, shapes, dtypes and order equal the reference class
    built from the same config (tests/golden/make_golden_body_regressor.py); the dict is left as it was."""
    from pointcept.models import build_model
    from pointcept.models.default import DefaultClassifier
    from ptv3_hip.configs import PIG_WEIGHT_PTV3_CFG
    keep = copy.deepcopy(PIG_WEIGHT_PTV3_CFG)
    model = build_model(PIG_WEIGHT_PTV3_CFG)
    assert PIG_WEIGHT_PTV3_CFG == keep and repr(PIG_WEIGHT_PTV3_CFG) == repr(keep)
    assert type(model).__name__ == "PigBodyRegressor" and isinstance(model, DefaultClassifier)
    ref = open(os.path.join(golden_dir, "state_dict_pig_body_regressor_fork.txt")).read().strip().split("\n")
    assert [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()] == ref
    head = model.cls_head
    assert [type(m).__name__ for m in head] == ["Linear", "BatchNorm1d", "ReLU", "Dropout", "Linear", "BatchNorm1d",
                                                "ReLU", "Dropout", "Linear"]
    assert head[3].p == 0.5 and head[7].p == 0.5
    assert (head[0].in_features, head[0].out_features, head[4].out_features, head[8].out_features) == (64, 256, 128, 7)
    # head dimension 32 at every encoder level, 16 in the decoder
    blocks = [m for m in model.backbone.modules() if type(m).__name__ == "Block"]
    assert {b.channels // b.attn.num_heads for b in blocks} == {32, 16}


def test_default_classifier_defaults():
    from pointcept.models import build_model
    from ptv3_hip.configs import TINY_CFG
    model = build_model(dict(type="DefaultClassifier", backbone=dict(type="PT-v3m1", **TINY_CFG)))
    assert model.num_classes == 40 and model.backbone_embed_dim == 256
    assert model.cls_head[0].in_features == 256 and model.cls_head[8].out_features == 40
    assert set(k.split(".")[1] for k in model.state_dict() if k.startswith("cls_head.")) == {"0", "1", "4", "5", "8"}


def test_regression_l1_loss_on_cpu():
    from pointcept.models.losses import LOSSES
    loss = LOSSES.build(cfg=dict(type="RegressionL1Loss", loss_weight=2.5))
    g = torch.Generator().manual_seed(0)
    pred, target = torch.randn(5, 7, generator=g), torch.randn(35, generator=g)
    want = torch.nn.functional.l1_loss(pred, target.view(5, 7)) * 2.5
    assert torch.equal(loss(pred, target), want)
    assert LOSSES.build(cfg=dict(type="RegressionL1Loss")).loss_weight == 1.0
    with pytest.raises(RuntimeError):
        loss(torch.randn(3, 5), torch.randn(3, 5))


def _tiny(mode):
    from pointcept.models import build_model
    from ptv3_hip.configs import TINY_CFG
    return build_model(dict(type="PigBodyRegressor", num_classes=7, backbone_embed_dim=16,
                            criteria=[dict(type="RegressionL1Loss", loss_weight=1.0)],
                            backbone=dict(type="PT-v3m1", **TINY_CFG))).train(mode)


def test_cpu_tensors_are_refused():
    import ptv3_scenes as S
    data = S.make_batch([300, 200], in_channels=4, extent=32, seed=0)
    data["category"] = torch.zeros(2, 7)
    for mode in (True, False):
        with pytest.raises(RuntimeError, match="GPU tensor|No HIP GPUs"):
            _tiny(mode)(dict(data))


def test_one_scene_training_batch_raises_like_batchnorm():
    import ptv3_scenes as S
    data = S.make_batch([300], in_channels=4, extent=32, seed=0)
    data["category"] = torch.zeros(1, 7)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        _tiny(True)(data)


def test_yardstick_reproduces_reference_eval(golden_dir):
    """cls_head_ref on the fixture's pooled features and head weights gives the reference's eval logits, loss and
    column errors to 1e-5 relative: the float64 restatement the GPU tests measure against IS the reference's head."""
    import cls_head_ref as R
    g = np.load(os.path.join(golden_dir, "body_regressor_tiny.npz"))
    sd = {k[len("sd_cls_head."):]: torch.from_numpy(g[k]).double() for k in g.files if k.startswith("sd_cls_head.")}
    logits = R.head_eval(torch.from_numpy(g["eval_pooled"]).double(), sd)
    want = torch.from_numpy(g["eval_logits"]).double()
    assert ((logits - want).abs().max() / want.abs().max()).item() <= 1e-5
    stats = R.l1_stats(logits, torch.from_numpy(g["in_category"]).double(), 1.0, 100.0)
    assert abs(stats[0].item() - float(g["eval_loss"])) <= 1e-5 * float(g["eval_loss"])
    err = torch.from_numpy(g["eval_errors"]).double()
    assert ((stats[1:] - err).abs().max() / err.abs().max()).item() <= 1e-5
