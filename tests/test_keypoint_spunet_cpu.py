"""CPU-side checks of SpUNet-v1m1 / KeypointSparseUNet: registered under the reference's names and module paths, the
fork config's exact state_dict, argument refusals of ptv3_res_conv without a GPU, and the golden fixture's coarse site
lists re-derived from its input coordinates with numpy."""
import ctypes
import os

import numpy as np
import pytest
import torch


def test_names_registered_and_reference_module_paths_import():
    from pointcept.models import MODELS
    from pointcept.models.sparse_unet import SpUNetBase
    from pointcept.models.sparse_unet.spconv_unet_v1m1_base import BasicBlock, SpUNetBase as Base
    from pointcept.models.keypoint_sparse_unet import KeypointSparseUNet
    from pointcept.models.utils.sparse import SparseSequential, SubMConv3d
    from make_golden_keypoint_spunet import TINY_KW
    assert MODELS.get("SpUNet-v1m1") is SpUNetBase and Base is SpUNetBase
    assert MODELS.get("KeypointSparseUNet") is KeypointSparseUNet and issubclass(KeypointSparseUNet, SpUNetBase)
    same = BasicBlock(16, 16, norm_fn=torch.nn.BatchNorm1d, indice_key="subm1")
    assert isinstance(same.proj, SparseSequential) and isinstance(same.proj[0], torch.nn.Identity)
    front = BasicBlock(48, 16, norm_fn=torch.nn.BatchNorm1d, indice_key="subm1")
    assert isinstance(front.proj[0], SubMConv3d) and tuple(front.proj[0].weight.shape) == (16, 1, 1, 1, 48)
    assert tuple(front.conv1.weight.shape) == (16, 3, 3, 3, 48) and front.conv1.bias is None
    model = KeypointSparseUNet(num_classes=13, **TINY_KW)          # a num_classes in the config is dropped
    assert model.num_classes == 0 and isinstance(model.final, torch.nn.Identity) and hasattr(model, "set_fused")
    assert sum(p.numel() for p in model.parameters()) == 923218 and len(model.state_dict()) == 209
    assert model.reg_head[0].in_features == 16
    enc = KeypointSparseUNet(enc_mode=True, **TINY_KW)
    assert enc.dec is None and len(enc.up) == 0 and enc.reg_head[0].in_features == 64
    seg = SpUNetBase(in_channels=4, num_classes=13, base_channels=16, channels=TINY_KW["channels"],
                     layers=TINY_KW["layers"])
    assert tuple(seg.final.weight.shape) == (13, 1, 1, 1, 16) and tuple(seg.final.bias.shape) == (13,)


def test_fork_config_builds_with_reference_state_dict(golden_dir):
    """configs/my_dataset/keypoint_sparse_unet.py through the registry: keys, shapes, dtypes and order of the reference
    class built from the same config (tests/golden/make_golden_keypoint_spunet.py)."""
    from pointcept.models import build_model
    from pointcept.models.sparse_unet.spconv_unet_v1m1_base import BasicBlock
    from ptv3_hip.configs import KEYPOINT_SPUNET_CFG
    model = build_model(KEYPOINT_SPUNET_CFG)
    got = [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]
    ref = open(os.path.join(golden_dir, "state_dict_keypoint_spunet_fork.txt")).read().strip().split("\n")
    assert len(ref) == 365 and got == ref
    assert sum(p.numel() for p in model.parameters()) == 39243666
    assert sum(isinstance(m, BasicBlock) for m in model.modules()) == 23


def test_res_conv_refuses_bad_arguments_without_a_gpu():
    """Argument checks come before any pointer is touched or kernel launched: error code 1 and a message."""
    from ptv3_hip.lib import lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(ca=16, cb=0, cout=16, kvol=27, xb=None, nbr=p, out=p, w_proj=None, proj_out=None):
        return lib.ptv3_res_conv(p, xb, p, nbr, None, None, None, None, 0, out, w_proj, None, None, proj_out, 4, ca, cb,
                                 cout, kvol, None)
    assert call(ca=6) == 1 and b"ca=6" in lib.ptv3_last_error()
    assert call(cout=0) == 1 and b"cout=0" in lib.ptv3_last_error()
    assert call(kvol=1, nbr=None) == 1 and b"kvol=1" in lib.ptv3_last_error()
    assert call(out=None) == 1 and b"out are required" in lib.ptv3_last_error()
    assert call(w_proj=p) == 1 and b"w_proj and proj_out" in lib.ptv3_last_error()
    assert call(cb=16) == 1 and b"xb" in lib.ptv3_last_error()
    with pytest.raises(RuntimeError, match="ca=6"):
        lib.check(call(ca=6), "ptv3_res_conv")
    assert lib.ptv3_res_conv_capable(300, 96, 32, 96, 27) == 1 and lib.ptv3_res_conv_capable(300, 4, 4, 8, 27) == 1
    for bad in ((300, 96, 32, 96, 125), (300, 6, 0, 16, 27), (300, 16, 2, 16, 27), (300, 16, 0, 18, 27),
                (0, 16, 0, 16, 27), (300, 1024, 4, 16, 27), (300, 16, 0, 516, 27)):
        assert lib.ptv3_res_conv_capable(*bad) == 0, bad


def _down2_numpy(sites, shape):
    """kernel 2, stride 2: (coarse sites sorted by (b, x, y, z), coarse shape, number of sites without a parent)"""
    out_shape = [(s - 2) // 2 + 1 for s in shape]
    par = np.concatenate([sites[:, :1], sites[:, 1:] >> 1], axis=1)
    ok = np.all(par[:, 1:] < np.asarray(out_shape), axis=1)
    return np.unique(par[ok], axis=0), out_shape, int((~ok).sum())


def test_golden_coarse_sites_rederived_with_numpy(golden_dir):
    """The reference run's site lists at the four coarse levels follow from its input coordinates; under
    sparse_shape = max(grid_coord) + 96 no site loses its parent and no scene is empty at the deepest level."""
    g = np.load(os.path.join(golden_dir, "keypoint_spunet_tiny.npz"))
    grid, ends = g["in_grid_coord"].astype(np.int64), g["in_offset"].tolist()
    batch = np.repeat(np.arange(len(ends)), np.diff([0] + ends))
    sites = np.concatenate([batch[:, None], grid], axis=1)
    shape = (grid.max(0) + 96).tolist()
    for level in range(1, 5):
        sites, shape, lost = _down2_numpy(sites, shape)
        assert lost == 0
        assert np.array_equal(sites, g[f"sites{level}"].astype(np.int64)), level
        assert set(sites[:, 0].tolist()) == set(range(len(ends)))
    assert len(sites) == g["tap_enc.3"].shape[0]
