"""CPU-side checks of KeypointPTv2 / PT-v2m2: registered under the reference's names and module paths, the fork config's
exact state_dict, the argument refusals of ptv3_gva_fwd and the grid-pool entries without a GPU, the golden fixture's
cell margins re-derived in float64, and the refusal of a scene without points."""
import ctypes
import os

import numpy as np
import pytest
import torch

from make_golden_keypoint_ptv2 import TINY_KW, TINY_BACKBONE, MARGIN, cell_margin

N_TINY_PARAMS = 224194


def test_names_registered_and_reference_module_paths_import():
    from pointcept.models import MODELS, build_model
    assert MODELS.get("PT-v2m2") is not None and MODELS.get("KeypointPTv2") is not None
    from pointcept.models.point_transformer_v2 import PointTransformerV2
    from pointcept.models.point_transformer_v2.point_transformer_v2m2_base import (
        PointBatchNorm, GroupedVectorAttention, Block, BlockSequence, GridPool, UnpoolWithSkip, Encoder, Decoder,
        GVAPatchEmbed)
    from pointcept.models.keypoint_ptv2 import KeypointPTv2
    model = build_model(dict(type="KeypointPTv2", **TINY_KW))
    assert isinstance(model, KeypointPTv2) and isinstance(model.backbone, PointTransformerV2)
    assert sum(p.numel() for p in model.parameters()) == N_TINY_PARAMS
    bb = model.backbone
    assert isinstance(bb.patch_embed, GVAPatchEmbed) and isinstance(bb.patch_embed.blocks, BlockSequence)
    assert isinstance(bb.enc_stages[0], Encoder) and isinstance(bb.enc_stages[0].down, GridPool)
    assert isinstance(bb.dec_stages[0], Decoder) and isinstance(bb.dec_stages[0].up, UnpoolWithSkip)
    block = bb.enc_stages[2].blocks.blocks[1]
    assert isinstance(block, Block) and isinstance(block.attn, GroupedVectorAttention)
    assert isinstance(block.norm1, PointBatchNorm) and isinstance(block.norm1.norm, torch.nn.BatchNorm1d)
    assert (block.attn.embed_channels, block.attn.groups) == (64, 8) and block.attn.fusable()
    # more neighbours than the kernel holds (or none) go to the composition, as an unsupported width does
    assert block.attn.fusable(32) and not block.attn.fusable(33) and not block.attn.fusable(0)
    # (n, l, c) input: statistics over every (point, slot) row, as BatchNorm1d gives them for (n, c, l)
    bn = PointBatchNorm(5).train()
    x = torch.randn(7, 3, 5)
    want = torch.nn.BatchNorm1d(5).train()(x.transpose(1, 2)).transpose(1, 2)
    assert torch.allclose(bn(x), want, atol=1e-6)
    # a plain segmentation head when num_classes > 0 (the reference's seg_head keys)
    seg = build_model(dict(TINY_BACKBONE, num_classes=13))
    assert [k for k in seg.state_dict() if k.startswith("seg_head.")][:2] == ["seg_head.0.weight", "seg_head.0.bias"]


def test_fork_config_builds_with_reference_state_dict(golden_dir):
    """configs/my_dataset/keypoint_ptv2.py through the registry: keys, shapes, dtypes and order of the reference class
    built from the same config (tests/golden/make_golden_keypoint_ptv2.py), and the parameter count."""
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_PTV2_CFG
    model = build_model(KEYPOINT_PTV2_CFG)
    got = [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]
    ref = open(os.path.join(golden_dir, "state_dict_keypoint_ptv2_fork.txt")).read().strip().split("\n")
    assert len(ref) == 964 and got == ref
    assert sum(p.numel() for p in model.parameters()) == 11403754
    # strict load of a checkpoint with the reference's keys
    model.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}, strict=True)
    rates = [b.drop_path.drop_prob for s in model.backbone.enc_stages for b in s.blocks.blocks
             if not isinstance(b.drop_path, torch.nn.Identity)]
    assert len(rates) == 11 and abs(rates[-1] - 0.3) < 1e-6     # linspace(0, 0.3, 12): the first block has none


def test_groups_must_divide_channels():
    from pointcept.models import build_model
    with pytest.raises(ValueError, match="groups=5 does not divide embed_channels=16"):
        build_model(dict(TINY_BACKBONE, patch_embed_groups=5))


def _gva(lib, p, n, c, g, ns, null=None):
    args = [p] * 5 + [n, c, g, ns] + [p] * 10 + [p, None]
    if null is not None:
        args[null] = None
    return lib.ptv3_gva_fwd(*args)


def test_gva_refuses_bad_arguments_without_a_gpu():
    """Argument checks come before any pointer is touched or kernel launched: error code 1 and a message."""
    from ptv3_hip.lib import lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    for c in (12, 520, 0):
        assert _gva(lib, p, 4, c, 1, 8) == 1 and f"c={c} unsupported".encode() in lib.ptv3_last_error()
    assert _gva(lib, p, 4, 64, 5, 8) == 1 and b"groups=5 unsupported for c=64" in lib.ptv3_last_error()
    assert _gva(lib, p, 4, 512, 128, 8) == 1 and b"groups=128 unsupported" in lib.ptv3_last_error()
    assert _gva(lib, p, 4, 64, 0, 8) == 1 and b"groups=0 unsupported" in lib.ptv3_last_error()
    for ns in (0, 33):
        assert _gva(lib, p, 4, 64, 8, ns) == 1 and f"ns={ns} unsupported".encode() in lib.ptv3_last_error()
    assert _gva(lib, p, -1, 64, 8, 16) == 1 and b"outside [0, 2^31)" in lib.ptv3_last_error()
    assert _gva(lib, p, 1 << 31, 64, 8, 16) == 1 and b"outside [0, 2^31)" in lib.ptv3_last_error()
    for slot in (0, 1, 2, 3, 4, 19):          # q, k, v, xyz, idx, out
        assert _gva(lib, p, 4, 64, 8, 16, null=slot) == 1 and b"a NULL tensor" in lib.ptv3_last_error(), slot
    for slot in range(9, 19):                 # the ten weights
        assert _gva(lib, p, 4, 64, 8, 16, null=slot) == 1 and b"a NULL weight" in lib.ptv3_last_error(), slot
    with pytest.raises(RuntimeError, match="c=12 unsupported"):
        lib.check(_gva(lib, p, 4, 12, 1, 8), "ptv3_gva_fwd")


def test_zero_rows_return_ok_without_a_launch():
    """n = 0 returns PTV3_OK before any pointer is looked at (NULL tensors included) - on a box without a GPU a launch
    would fail."""
    from ptv3_hip.lib import lib
    assert lib.ptv3_gva_fwd(*([None] * 5), 0, 64, 8, 16, *([None] * 10), None, None) == 0
    assert lib.ptv3_grid_keys(None, 0, None, 1, 0.06, None, None, None, None, None) == 0
    assert lib.ptv3_segment_mean3(None, None, None, 0, None, None) == 0


def test_grid_entries_refuse_bad_arguments_without_a_gpu():
    from ptv3_hip.lib import lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    keys = lambda n, b, size, coord=p: lib.ptv3_grid_keys(coord, n, p, b, size, p, p, p, p, None)   # noqa: E731
    for size in (0.0, -0.5, float("nan"), float("inf")):
        assert keys(4, 1, size) == 1 and b"must be positive and finite" in lib.ptv3_last_error(), size
    for b in (0, 4097):
        assert keys(4, b, 0.06) == 1 and f"{b} scenes outside".encode() in lib.ptv3_last_error()
    assert keys(-1, 1, 0.06) == 1 and b"outside [0, 2^31)" in lib.ptv3_last_error()
    assert keys(4, 1, 0.06, coord=None) == 1 and b"a NULL tensor" in lib.ptv3_last_error()
    assert lib.ptv3_segment_mean3(p, p, p, -1, p, None) == 1 and b"n_out=-1" in lib.ptv3_last_error()
    assert lib.ptv3_segment_mean3(p, None, p, 3, p, None) == 1 and b"a NULL tensor" in lib.ptv3_last_error()


def test_unfused_ptv2_pointops_steps_keep_raising():
    """The attention is fused (ptv3_gva_fwd): the PTv2 step functions of libs/pointops stay unbuilt."""
    import pointops
    for name in ("attention_relation_step", "attention_fusion_step", "subtraction", "aggregation"):
        with pytest.raises(NotImplementedError):
            getattr(pointops, name)()


def test_golden_cells_hold_the_margin_in_float64(golden_dir):
    """Every level the fixture's model pools, from the stored coordinates and offsets: each non-zero (coord - start) /
    size is at least 1e-4 from an integer in float64 - three orders above the fp32 rounding of the quotient (cells stay
    below 64: 64 * 2^-23 is about 8e-6 with the subtraction's error) - and the fp32 cell equals the float64 one, so an
    fp32 kernel cannot legitimately place a point in another cell.  An exact zero (a scene's minimum minus itself) is
    zero in any arithmetic.  The stored cluster maps follow from those cells ranked by (scene, z, y, x)."""
    g = np.load(os.path.join(golden_dir, "keypoint_ptv2_tiny.npz"))
    coord, ends = g["in_coord"], g["in_offset"]
    for i, size in enumerate(TINY_BACKBONE["grid_sizes"]):
        margin, same, cells, batch = cell_margin(coord, ends, size)
        assert margin >= MARGIN and same, (i, margin)
        assert cells.max() < 64
        key = ((batch * 64 + cells[:, 2]) * 64 + cells[:, 1]) * 64 + cells[:, 0]
        _, inverse = np.unique(key, return_inverse=True)
        assert np.array_equal(inverse, g[f"cluster{i}"]), i
        assert int(g[f"count{i + 1}"]) == inverse.max() + 1 == len(g[f"coord{i + 1}"])
        coord, ends = g[f"coord{i + 1}"], g[f"offset{i + 1}"]
    sizes = np.diff(np.concatenate([[0], g["offset4"]]))
    assert sizes[1] < 16 <= sizes[2]      # -1 neighbours occur in the 0.5-wide scene only
    assert all(np.diff(np.concatenate([[0], g[f"offset{i}"]]))[2] >= 16 for i in range(1, 5))


def test_scene_without_points_raises():
    """A scene without points has no mean (the reference divides by zero there): refused by name before device work."""
    from pointcept.models import build_model
    model = build_model(dict(type="KeypointPTv2", **TINY_KW))
    data = dict(coord=torch.rand(30, 3), feat=torch.rand(30, 4), offset=torch.tensor([20, 20, 30]))
    for mode in (True, False):
        with pytest.raises(ValueError, match="scene 1 has no points"):
            model.train(mode)(dict(data))
    with pytest.raises(ValueError, match="a scene without points"):
        model.backbone.eval()(dict(data))
    ok = dict(data, offset=torch.tensor([10, 20, 30]))
    with pytest.raises(RuntimeError, match="GPU tensor|No HIP GPUs"):
        model.eval()(ok)
