"""CPU-side checks of PT-v3m1-Plus / KeypointPTv3Plus: registered under the reference's names and module path, the fork
config's exact state_dict, the bottleneck width rule, the folded expand matrix against the two-step product in float64,
and the fixture's stored re-serialization orders."""
import os

import numpy as np
import torch

from make_golden_keypoint_ptv3_plus import PLUS_TINY_CFG
from keypoint_ptv3_plus_params import seeded_state_dict


def test_names_registered_and_reference_module_path_imports():
    from pointcept.models import MODELS, build_model, BlockPlus, PointTransformerV3Plus, KeypointPTv3Plus
    from pointcept.models import keypoint_ptv3_plus as mod
    from pointcept.models.keypoint_ptv3 import KeypointPTv3
    assert MODELS.get("PT-v3m1-Plus") is PointTransformerV3Plus is mod.PointTransformerV3Plus
    assert MODELS.get("KeypointPTv3Plus") is KeypointPTv3Plus and issubclass(KeypointPTv3Plus, KeypointPTv3)
    assert mod.BlockPlus is BlockPlus
    model = build_model(dict(type="KeypointPTv3Plus", num_keypoints=6, hidden_dim=32,
                             backbone_conf=dict(type="PT-v3m1-Plus", **PLUS_TINY_CFG)))
    bb = model.backbone
    assert isinstance(bb, PointTransformerV3Plus) and not hasattr(bb, "use_engine")
    blocks = [m for m in bb.modules() if isinstance(m, BlockPlus)]
    assert len(blocks) == 10 and all(b.attn.order_index == 0 for b in blocks)
    assert all(b.cpe[3].kernel_size == 5 and b.cpe[3].indice_key.startswith("stage") for b in blocks)
    assert tuple(blocks[0].cpe[0].weight.shape) == (16, 1, 1, 1, 16)
    assert tuple(bb.enc_stages[2].block0.cpe[6].weight.shape) == (64, 1, 1, 1, 16)
    # a strict load of the seeded fixture parameters (drawn from this model's own listing)
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    for bad in ("pdnorm_bn", "pdnorm_ln"):
        try:
            build_model(dict(type="PT-v3m1-Plus", **dict(PLUS_TINY_CFG, **{bad: True})))
        except NotImplementedError as e:
            assert "pdnorm_bn" in str(e) and "pdnorm_ln" in str(e)
        else:
            raise AssertionError(f"{bad}=True must raise")


def test_block_plus_is_a_block_with_unchanged_construction():
    """BlockPlus subclasses Block but keeps its own class name (the native executor matches on "Block"), and building
    either backbone draws from the RNG as before the two classes were joined: float64 sum of |p| over all parameters
    after torch.manual_seed(0), recorded at the commit before (CPU initialisation is deterministic)."""
    from pointcept.models import build_model, BlockPlus
    from pointcept.models.point_transformer_v3.point_transformer_v3m1_base import Block
    from make_golden_cfg import TINY_CFG
    assert issubclass(BlockPlus, Block)
    for cfg, expected in ((dict(type="PT-v3m1-Plus", **PLUS_TINY_CFG), 27887.581024057035),
                          (dict(type="PT-v3m1", **TINY_CFG), 16141.89209908651)):
        torch.manual_seed(0)
        model = build_model(cfg)
        total = sum(p.detach().double().abs().sum().item() for p in model.parameters())
        assert abs(total - expected) <= 1e-12 * expected, (cfg["type"], repr(total))
        names = {type(m).__name__ for m in model.modules() if isinstance(m, Block)}
        assert names == ({"BlockPlus"} if cfg["type"] == "PT-v3m1-Plus" else {"Block"})


def test_fork_config_builds_with_reference_state_dict(golden_dir):
    """configs/my_dataset/keypoint_ptv3_plus.py through the registry: keys, shapes, dtypes and order of the reference
    class built from the same config (tests/golden/make_golden_keypoint_ptv3_plus.py)."""
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_PTV3_PLUS_CFG
    model = build_model(KEYPOINT_PTV3_PLUS_CFG)
    got = [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]
    ref = open(os.path.join(golden_dir, "state_dict_keypoint_ptv3_plus_fork.txt")).read().strip().split("\n")
    assert len(ref) == 629 and got == ref
    # the 5^3 convolutions of the fork widths run at these bottleneck widths (encoder, then decoder top-down)
    mids = [b.cpe[3].in_channels for s in model.backbone.enc_stages for n, b in s.named_children() if n == "block0"]
    assert mids == [32, 16, 32, 64, 128]
    mids = [d.block0.cpe[3].in_channels for d in model.backbone.dec.children()]
    assert mids == [64, 32, 16, 16]


def test_bottleneck_width_rule():
    from pointcept.models.keypoint_ptv3_plus import cpe_mid_channels
    assert [cpe_mid_channels(c) for c in (16, 32, 60, 64, 512)] == [16, 32, 60, 16, 128]


def test_folded_expand_equals_two_steps_in_float64():
    from pointcept.models.keypoint_ptv3_plus import fold_expand
    g = torch.Generator().manual_seed(6)
    for c, mid in ((16, 16), (64, 16), (512, 128)):
        w_up = torch.randn(c, 1, 1, 1, mid, generator=g, dtype=torch.float64)
        w_lin = torch.randn(c, c, generator=g, dtype=torch.float64)
        h = torch.randn(37, mid, generator=g, dtype=torch.float64)
        two = (h @ w_up.view(c, mid).t()) @ w_lin.t()
        one = h @ fold_expand(w_up, w_lin).t()
        assert tuple(fold_expand(w_up, w_lin).shape) == (c, mid)
        assert (one - two).abs().max().item() <= 1e-12 * two.abs().max().item()


def test_fixture_orders_are_permutations(golden_dir):
    g = np.load(os.path.join(golden_dir, "keypoint_ptv3_plus_tiny.npz"))
    enc = np.load(os.path.join(golden_dir, "keypoint_ptv3_plus_tiny_enc.npz"))
    assert g["order_0"].size == 0 and g["order_3"].size == 0          # stage 0 and s % 3 == 0 are not reordered
    for s in (1, 2, 4):
        order = g[f"order_{s}"]
        assert order.dtype == np.int64 and order.size == enc[f"enc_{s}"].shape[0] > 0
        assert np.array_equal(np.sort(order), np.arange(order.size))
        assert not np.array_equal(order, np.arange(order.size))
    assert 0 < float(g["eval_fp64_gap"]) < 1e-4


def test_fixture_entries_are_the_tiny_models_state_dict(golden_dir):
    """The fixture's parameters are drawn, not stored, so a strict load alone shows nothing about names: the gradients
    and running statistics the reference class wrote carry its own entry names and shapes, and they must be exactly the
    tiny model's parameters and buffers here."""
    from pointcept.models import build_model
    model = build_model(dict(type="KeypointPTv3Plus", num_keypoints=6, hidden_dim=32,
                             backbone_conf=dict(type="PT-v3m1-Plus", **PLUS_TINY_CFG)))
    stored = {}
    for part in ("_grad_cpe", "_grad_rest"):
        z = np.load(os.path.join(golden_dir, f"keypoint_ptv3_plus_tiny{part}.npz"))
        stored.update({k[5:]: tuple(z[k].shape) for k in z.files if k.startswith("grad_")})
    assert stored == {n: tuple(p.shape) for n, p in model.named_parameters()}
    assert sum(n.endswith("cpe.3.weight") for n in stored) == 10
    g = np.load(os.path.join(golden_dir, "keypoint_ptv3_plus_tiny.npz"))
    bufs = {k[4:]: tuple(g[k].shape) for k in g.files if k.startswith("buf_")}
    assert bufs == {n: tuple(b.shape) for n, b in model.named_buffers() if "running" in n}
