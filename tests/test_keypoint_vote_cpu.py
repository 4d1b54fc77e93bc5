"""CPU-side checks of the voting keypoint model (KeypointSwin3DVote) and its entry points: registered, built from the
fork config with the reference's exact state_dict, refusing to run without a GPU, and validating arguments and target
shapes on the host before any launch."""
import os

import pytest


def test_keypoint_vote_model_registered():
    from pointcept.models import MODELS
    assert MODELS.get("KeypointSwin3DVote") is not None


def test_fork_config_builds_with_reference_state_dict(golden_dir):
    """configs/my_dataset/keypoint_swin3d_plus.py through the registry: keys, shapes, dtypes and order equal the
    reference class built from the same config (tests/golden/make_golden_keypoint_vote.py)."""
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_SWIN3D_VOTE_CFG as cfg
    keep = repr(cfg)
    model = build_model(cfg)
    assert repr(cfg) == keep
    ref = open(os.path.join(golden_dir, "state_dict_keypoint_swin3d_vote_fork.txt")).read().strip().split("\n")
    assert [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()] == ref
    head = model.vote_head
    assert [type(m).__name__ for m in head] == ["Linear", "BatchNorm1d", "ReLU", "Dropout", "Linear", "BatchNorm1d",
                                                "ReLU", "Linear"]
    assert head[3].p == 0.3 and head[7].out_features == 18 and model.vote_radius == 0.3
    assert sorted({k.split(".")[1] for k in model.state_dict() if k.startswith("vote_head.")}) == list("01457")


def test_constructor_defaults_match_reference():
    import inspect
    from pointcept.models import MODELS
    sig = inspect.signature(MODELS.get("KeypointSwin3DVote").__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[2:]] == [
        ("num_keypoints", 6), ("hidden_dim", 256), ("vote_radius", 0.4)]


def test_keypoint_vote_model_refuses_cpu_tensors():
    """Training and eval run on the HIP path only: CPU tensors are refused, never silently computed."""
    import torch
    from pointcept.models import build_model
    from test_keypoint_regression_cpu import TINY_SWIN3D_KP
    import ptv3_scenes as S
    model = build_model(dict(type="KeypointSwin3DVote", num_keypoints=6, hidden_dim=32,
                             backbone_conf=dict(TINY_SWIN3D_KP)))
    data = S.make_batch([300, 200], in_channels=6, extent=32, seed=0)
    data["target"] = torch.zeros(12, 3)
    for mode in (True, False):
        with pytest.raises(RuntimeError, match="GPU tensor|No HIP GPUs"):
            model.train(mode)(dict(data))


def test_ops_refuse_cpu_tensors():
    import torch
    from ptv3_hip import ops
    x, coord, off = torch.zeros(10, 18), torch.zeros(10, 3), torch.tensor([10])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.scene_median(x, coord, off)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.vote_loss(x, coord, torch.zeros(6, 3), off, 0.4)


def test_bad_target_shape_raises_reference_value_error():
    """keypoint_swin3d_plus.py:95-102, decided from host shapes: B * K * 3 numbers, or N leading rows."""
    import torch
    from ptv3_hip.ops import _vote_target
    n, k, b = 50, 6, 3
    assert _vote_target(torch.zeros(b * k, 3), n, k, b)[1] == 0
    assert _vote_target(torch.zeros(b, k, 3), n, k, b)[1] == 0
    t, flag = _vote_target(torch.zeros(n, k, 3), n, k, b)
    assert flag == 1 and tuple(t.shape) == (n * k, 3)
    assert _vote_target(torch.zeros(n, k * 3), n, k, b)[1] == 1
    for bad in (torch.zeros(b * k + 1, 3), torch.zeros(n + 1, k, 3), torch.zeros(n, k + 1, 3), torch.zeros(7)):
        with pytest.raises(ValueError, match="Target shape mismatch"):
            _vote_target(bad, n, k, b)


def test_argument_validation_without_gpu():
    """Host-side checks run before any launch: bad arguments come back as error codes + message."""
    from ptv3_hip.lib import lib
    one = 16   # a non-null, 16-byte aligned stand-in pointer: rejected calls never dereference it
    assert lib.ptv3_scene_median(one, None, one, 10, 0, 1, one, one, 1 << 20, None) != 0
    assert b"c=0 unsupported" in lib.ptv3_last_error()
    assert lib.ptv3_scene_median(one, None, one, 10, 33, 1, one, one, 1 << 20, None) != 0
    assert b"c=33 unsupported" in lib.ptv3_last_error()
    assert lib.ptv3_scene_median(one, one, one, 10, 16, 1, one, one, 1 << 20, None) != 0
    assert b"multiple of 3" in lib.ptv3_last_error()
    assert lib.ptv3_scene_median(one, None, None, 10, 18, 1, one, one, 1 << 20, None) != 0
    assert b"NULL" in lib.ptv3_last_error()
    assert lib.ptv3_scene_median(one, None, one, 10, 18, 1, one, one + 4, 1 << 20, None) != 0
    assert b"16-byte aligned" in lib.ptv3_last_error()
    assert lib.ptv3_scene_median(one, None, one, 10, 18, 2, one, one, 16, None) != 0
    assert b"workspace too small" in lib.ptv3_last_error()
    assert lib.ptv3_scene_median(one, None, one, -1, 18, 2, one, one, 1 << 20, None) != 0
    assert b"bad shape" in lib.ptv3_last_error()
    # four 256-bin histograms and a NaN counter per (scene, column)
    assert lib.ptv3_scene_median_workspace_bytes(18, 8) == 8 * 18 * (4 * 256 + 1) * 4
    assert lib.ptv3_vote_loss_workspace_bytes(100000, 6, 1) >= 3 * 6 * 4
    assert lib.ptv3_vote_loss(one, one, one, 0, one, None, 0, 10, 0, 1, 0.4, one, one, one, 1 << 20, None) != 0
    assert b"k=0 unsupported" in lib.ptv3_last_error()
    assert lib.ptv3_vote_loss(one, one, one, 0, one, None, 0, 10, 33, 1, 0.4, one, one, one, 1 << 20, None) != 0
    assert b"k=33 unsupported" in lib.ptv3_last_error()
    assert lib.ptv3_vote_loss(None, one, one, 0, one, None, 0, 10, 6, 1, 0.4, one, one, one, 1 << 20, None) != 0
    assert b"NULL" in lib.ptv3_last_error()
    assert lib.ptv3_vote_loss(one, one, one, 0, one, None, 0, 10, 6, 1, float("nan"), one, one, one, 1 << 20, None) != 0
    assert b"NaN" in lib.ptv3_last_error()
    assert lib.ptv3_vote_loss(one, one, one, 0, one, None, 0, 10, 6, 1, 0.4, one, one, one, 8, None) != 0
    assert b"workspace too small" in lib.ptv3_last_error()
    assert lib.ptv3_vote_loss_bwd(one, one, one, one, 0, one, one, 10, 6, 1, 0.4, None, None) != 0
    assert b"NULL" in lib.ptv3_last_error()
