"""CPU-side checks of the global-regression keypoint models (KeypointPTv3, KeypointSwin3D) and their evaluator hook:
registered, built from the fork configs with the reference's exact state_dict, and refusing to run without a GPU."""
import os

import pytest


def _listing(model):
    return [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]


def test_keypoint_regression_models_and_hook_registered():
    from pointcept.models import MODELS
    from pointcept.engines.hooks.builder import HOOKS
    import pointcept.engines.hooks  # noqa: F401
    for name in ("KeypointPTv3", "KeypointSwin3D"):
        assert MODELS.get(name) is not None, name
    hook = HOOKS.build(dict(type="KeypointEvaluator"))
    assert type(hook).__name__ == "KeypointEvaluator"


@pytest.mark.parametrize("cfg_name,listing", [("KEYPOINT_PTV3_CFG", "state_dict_keypoint_ptv3_fork.txt"),
                                              ("KEYPOINT_SWIN3D_CFG", "state_dict_keypoint_swin3d_fork.txt")])
def test_fork_configs_build_with_reference_state_dict(golden_dir, cfg_name, listing):
    """configs/my_dataset/keypoint_ptv3.py and keypoint_swin3d.py through the registry: keys, shapes, dtypes and order
    equal the reference classes built from the same configs (tests/golden/make_golden_keypoint_regression.py)."""
    from pointcept.models import build_model
    from ptv3_hip import configs
    cfg = getattr(configs, cfg_name)
    keep = repr(cfg)
    model = build_model(cfg)
    assert repr(cfg) == keep
    ref = open(os.path.join(golden_dir, listing)).read().strip().split("\n")
    assert _listing(model) == ref
    head = model.reg_head
    assert [type(m).__name__ for m in head] == ["Linear", "BatchNorm1d", "ReLU", "Dropout", "Linear", "ReLU", "Linear"]
    assert head[3].p == 0.3 and head[6].out_features == 18


def test_keypoint_regression_models_refuse_cpu_tensors():
    """Training and eval run on the HIP path only: CPU tensors are refused, never silently computed."""
    import torch
    from pointcept.models import build_model
    from ptv3_hip.configs import TINY_CFG
    import ptv3_scenes as S
    model = build_model(dict(type="KeypointPTv3", num_keypoints=6, hidden_dim=32,
                             backbone_conf=dict(type="PT-v3m1", **TINY_CFG)))
    data = S.make_batch([300, 200], in_channels=4, extent=32, seed=0)
    data["target"] = torch.zeros(12, 3)
    for mode in (True, False):
        with pytest.raises(RuntimeError, match="GPU tensor|No HIP GPUs"):
            model.train(mode)(dict(data))
    swin = build_model(dict(type="KeypointSwin3D", num_keypoints=6, hidden_dim=32,
                            backbone_conf=dict(TINY_SWIN3D_KP)))
    sdata = S.make_batch([300, 200], in_channels=6, extent=32, seed=0)
    sdata["target"] = torch.zeros(12, 3)
    for mode in (True, False):
        with pytest.raises(RuntimeError, match="GPU tensor|No HIP GPUs"):
            swin.train(mode)(dict(sdata))


def test_one_scene_training_batch_raises_like_batchnorm():
    """nn.BatchNorm1d refuses a training batch of one pooled row; the model says so before any device work."""
    import torch
    from pointcept.models import build_model
    from ptv3_hip.configs import TINY_CFG
    import ptv3_scenes as S
    model = build_model(dict(type="KeypointPTv3", num_keypoints=6, hidden_dim=32,
                             backbone_conf=dict(type="PT-v3m1", **TINY_CFG))).train()
    data = S.make_batch([300], in_channels=4, extent=32, seed=0)
    data["target"] = torch.zeros(6, 3)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        model(data)


# plumbing-size Swin3D whose output width equals channels[0] (the head's in_channels), as in the fork config
TINY_SWIN3D_KP = dict(type="Swin3D-v1m1", in_channels=9, num_classes=16, base_grid_size=0.02, depths=[2, 2, 2],
                      channels=[16, 32, 32], num_heads=[2, 2, 2], window_sizes=[5, 7, 7], quant_size=4,
                      drop_path_rate=0.0, up_k=3, num_layers=3, stem_transformer=True, down_stride=3,
                      upsample="linear_attn", knn_down=True, cRSE="XYZ_RGB_NORM", fp16_mode=1)
