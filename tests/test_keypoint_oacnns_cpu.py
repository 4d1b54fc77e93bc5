"""CPU-side checks of KeypointOACNNs: registered under the reference's names and module paths, the fork config's exact
state_dict, argument refusals of the new C entries without a GPU, the refusal of a batch too small for four stride-2
convs, and the golden fixture's coarse site lists re-derived from its input coordinates with numpy."""
import ctypes
import os

import numpy as np
import pytest
import torch


def test_names_registered_and_reference_module_paths_import():
    from pointcept.models import MODELS
    assert MODELS.get("OACNNs") is not None and MODELS.get("KeypointOACNNs") is not None
    from pointcept.models.oacnns import OACNNs
    from pointcept.models.oacnns.oacnns_v1m1_base import BasicBlock, DonwBlock, UpBlock
    from pointcept.models.keypoint_oa_cnns import KeypointOACNNs
    from pointcept.models.utils.sparse import SparseConv3d, SparseInverseConv3d, SparseSequential
    assert issubclass(KeypointOACNNs, OACNNs) and MODELS.get("KeypointOACNNs") is KeypointOACNNs
    down = DonwBlock(16, 32, 2, "spconv0", [4, 6, 6], groups=2, norm_fn=torch.nn.BatchNorm1d, sub_indice_key="subm1")
    assert isinstance(down.down, SparseSequential) and isinstance(down.down[0], SparseConv3d)
    assert tuple(down.down[0].weight.shape) == (32, 2, 2, 2, 16) and down.down[0].bias is None
    assert len(down.blocks) == 2 and isinstance(down.blocks[0], BasicBlock) and len(down.blocks[0].l_w) == 3
    up = UpBlock(32, 16, 16, 2, "spconv0", norm_fn=torch.nn.BatchNorm1d)
    assert isinstance(up.up[0], SparseInverseConv3d) and len(up.blocks) == 0
    model = KeypointOACNNs(num_keypoints=6, hidden_dim=32, in_channels=4, embed_channels=16,
                           enc_channels=[16, 16, 32, 32], groups=[2, 2, 4, 4], enc_depth=[1, 1, 2, 1],
                           dec_channels=[16, 16, 32, 32], point_grid_size=[[4, 6, 6], [3, 4, 4], [2, 3, 3], [2, 2, 3]])
    assert isinstance(model.final, torch.nn.Identity) and hasattr(model, "set_fused")
    assert sum(p.numel() for p in model.parameters()) == 304434 and len(model.state_dict()) == 453


def test_strided_convs_refuse_everything_but_kernel_2_stride_2():
    from pointcept.models.utils.sparse import SparseConv3d, SparseInverseConv3d
    with pytest.raises(NotImplementedError, match="kernel_size"):
        SparseConv3d(16, 16, kernel_size=3, stride=2)
    with pytest.raises(NotImplementedError, match="stride"):
        SparseConv3d(16, 16, kernel_size=2, stride=1)
    with pytest.raises(NotImplementedError, match="kernel_size"):
        SparseInverseConv3d(16, 16, kernel_size=3, indice_key="k")
    with pytest.raises(ValueError, match="point_grid_size 200"):
        from pointcept.models.oacnns.oacnns_v1m1_base import DonwBlock
        DonwBlock(16, 16, 1, "k", [4, 200], groups=2, norm_fn=torch.nn.BatchNorm1d)


def test_fork_config_builds_with_reference_state_dict(golden_dir):
    """configs/my_dataset/keypoint_oa_cnns.py through the registry: keys, shapes, dtypes and order of the reference
    class built from the same config (tests/golden/make_golden_keypoint_oacnns.py)."""
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_OACNNS_CFG
    model = build_model(KEYPOINT_OACNNS_CFG)
    got = [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]
    ref = open(os.path.join(golden_dir, "state_dict_keypoint_oacnns_fork.txt")).read().strip().split("\n")
    assert len(ref) == 1904 and got == ref
    assert sum(p.numel() for p in model.parameters()) == 51617426
    assert sum(len(s.blocks) for s in model.enc) == 23 and all(len(s.point_grid_size) == 4 for s in model.enc)


def test_new_entries_refuse_bad_arguments_without_a_gpu():
    """Argument checks come before any pointer is touched or kernel launched: error code 1 and a message."""
    from ptv3_hip.lib import lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ptrs = (ctypes.c_void_p * 4)(p, p, p, p)
    center = lambda c, x=p: lib.ptv3_cluster_center(x, c, p, p, p, 4, c, p, None)                 # noqa: E731
    ssum = lambda c, v=p: lib.ptv3_cluster_softmax_sum(p, c, v, c, p, p, p, p, 4, c, p, None)      # noqa: E731
    mix = lambda c, levels, lg=p: lib.ptv3_cluster_mix(lg, 4, ptrs, ptrs, levels, None, 0, 4, c, p, c, 0, None)  # noqa: E731
    for c in (6, 520, 0):
        for call in (center, ssum, lambda c: mix(c, 3)):
            assert call(c) == 1 and f"C={c} unsupported".encode() in lib.ptv3_last_error()
    for levels in (5, 0):
        assert mix(16, levels) == 1 and f"L={levels} aggregates unsupported".encode() in lib.ptv3_last_error()
    for g in (0, 200, -1):
        assert lib.ptv3_cluster_keys(p, 4, p, g, p, None) == 1
        assert f"g={g} outside".encode() in lib.ptv3_last_error()
    assert center(16, None) == 1 and b"NULL" in lib.ptv3_last_error()
    assert ssum(16, None) == 1 and b"NULL" in lib.ptv3_last_error()
    assert mix(16, 3, None) == 1 and b"NULL" in lib.ptv3_last_error()
    assert lib.ptv3_cluster_keys(p, 4, None, 4, p, None) == 1 and b"NULL" in lib.ptv3_last_error()
    starts = (ctypes.c_int32 * 10)(0, 1, 1, 2, 2, 3, 3, 4, 4, 4)
    assert lib.ptv3_down2_conv(p, p, None, 4, 2, 16, 16, None, None, 0, p, None) == 1 and b"NULL" in lib.ptv3_last_error()
    assert lib.ptv3_down2_conv(p, p, p, 4, 2, 6, 16, None, None, 0, p, None) == 1 and b"cin=6" in lib.ptv3_last_error()
    assert lib.ptv3_down2_conv(p, p, p, 4, 2, 16, 16, p, None, 0, p, None) == 1 and b"together" in lib.ptv3_last_error()
    assert lib.ptv3_up2_conv(p, p, p, None, starts, 4, 2, 16, 16, None, None, 0, p, None) == 1
    assert b"NULL" in lib.ptv3_last_error()
    assert lib.ptv3_up2_conv(p, p, p, p, starts, 5, 2, 16, 16, None, None, 0, p, None) == 1
    assert b"tap_start" in lib.ptv3_last_error()
    assert lib.ptv3_up2_conv(p, p, p, p, starts, 4, 2, 16, 16, None, None, 1, p, None) == 1 and b"act=1" in lib.ptv3_last_error()
    assert lib.ptv3_down2_keys(p, 4, 0, 4, 4, 64, p, p, None) == 1 and b"coarse shape" in lib.ptv3_last_error()
    assert lib.ptv3_down2_keys(None, 4, 4, 4, 4, 64, p, p, None) == 1 and b"NULL" in lib.ptv3_last_error()
    assert lib.ptv3_down2_children(p, p, p, p, p, p, p, 4, 64, p, None, p, p, p, None) == 1 and b"NULL" in lib.ptv3_last_error()
    assert lib.ptv3_add_act(p, p, 0, p, 6, None) == 1 and b"count=6" in lib.ptv3_last_error()
    with pytest.raises(RuntimeError, match="C=6 unsupported"):
        lib.check(center(6), "ptv3_cluster_center")


def test_too_small_batch_raises_before_device_work():
    """Four stride-2 convs need 2 cells per axis at every level: an extent under 16 is refused on the host, with the
    axis and the level named, in both modes; a large enough batch goes on to ask for the GPU."""
    import ptv3_scenes as S
    from pointcept.models import build_model
    from pointcept.models.oacnns.oacnns_v1m1_base import check_extent
    model = build_model(dict(type="KeypointOACNNs", num_keypoints=6, hidden_dim=32, in_channels=4, embed_channels=16,
                             enc_channels=[16, 16, 32, 32], groups=[2, 2, 4, 4], enc_depth=[1, 1, 1, 1],
                             dec_channels=[16, 16, 32, 32],
                             point_grid_size=[[4, 6], [3, 4], [2, 3], [2, 3]]))
    data = S.make_batch([300, 200], in_channels=4, extent=32, seed=0)
    small = dict(data)
    small["grid_coord"] = data["grid_coord"].clone()
    small["grid_coord"][:, 2] %= 15       # z extent 15: 15 -> 7 -> 3 -> 1, under 2 in front of the fourth conv
    for mode in (True, False):
        with pytest.raises(ValueError, match="axis z at level 3"):
            model.train(mode)(dict(small))
    with pytest.raises(ValueError, match="axis x at level 0"):
        check_extent("m", [1, 40, 40])
    check_extent("m", [16, 16, 16])
    with pytest.raises(ValueError, match="axis y at level 3"):
        check_extent("m", [16, 15, 16])
    with pytest.raises(RuntimeError, match="GPU tensor|No HIP GPUs"):
        model.eval()(dict(data))


def _down2_numpy(sites, shape):
    """kernel 2, stride 2: (coarse sites sorted by (b, x, y, z), coarse shape, number of sites without a parent)"""
    out_shape = [(s - 2) // 2 + 1 for s in shape]
    par = np.concatenate([sites[:, :1], sites[:, 1:] >> 1], axis=1)
    ok = np.all(par[:, 1:] < np.asarray(out_shape), axis=1)
    coarse = np.unique(par[ok], axis=0)         # lexicographic: (b, x, y, z)
    return coarse, out_shape, int((~ok).sum())


def test_golden_coarse_sites_rederived_with_numpy(golden_dir):
    """The reference run's site lists at the four coarse levels follow from its input coordinates by the stated rule,
    including the sites that lose their parent at an odd extent."""
    g = np.load(os.path.join(golden_dir, "keypoint_oacnns_tiny.npz"))
    grid, ends = g["in_grid_coord"].astype(np.int64), g["in_offset"].tolist()
    batch = np.repeat(np.arange(len(ends)), np.diff([0] + ends))
    sites = np.concatenate([batch[:, None], grid], axis=1)
    shape = (grid.max(0) + 1).tolist()
    assert any(s % 2 for s in shape) and grid[ends[0]:, 1].min() > 0
    dropped = []
    for level in range(1, 5):
        sites, shape, lost = _down2_numpy(sites, shape)
        dropped.append(lost)
        assert np.array_equal(sites, g[f"sites{level}"].astype(np.int64)), level
        assert set(sites[:, 0].tolist()) == set(range(len(ends)))
    assert dropped == g["dropped"].tolist() and dropped[0] >= 1 and sum(dropped) == 85
