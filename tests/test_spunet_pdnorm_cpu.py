"""SpUNet-v1m3 without a GPU: registration, the reference's state_dict from the config, constructor and input refusals,
the modulation identities of tests/pdnorm_ref.py against torch autograd on the reference's statement order, the argument
checks of the new entry points, and SyncBatchNorm adoption inside PDBatchNorm."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pdnorm_ref as R
from make_golden_spunet_pdnorm import load_golden, tiny_kw, CONDITIONS


def _listing(model):
    return [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]


def test_registered_and_importable_like_the_reference():
    from pointcept.models import MODELS, PDBatchNorm
    import pointcept.models.sparse_unet.spconv_unet_v1m3_pdnorm as v1m3
    import pointcept.models.sparse_unet.spconv_unet_v1m1_base as v1m1
    import pointcept.models.sparse_unet as pkg
    import pointcept.models as models
    assert MODELS.get("SpUNet-v1m3") is v1m3.SpUNetBase
    for name in ("PDBatchNorm", "BasicBlock", "SPConvDown", "SPConvUp", "SPConvPatchEmbedding", "SpUNetBase"):
        assert isinstance(getattr(v1m3, name), type), name
    assert PDBatchNorm is v1m3.PDBatchNorm
    # SpUNet-v1m1 is still what it was
    assert MODELS.get("SpUNet-v1m1") is v1m1.SpUNetBase and pkg.SpUNetBase is v1m1.SpUNetBase
    assert models.SpUNetBase is v1m1.SpUNetBase and pkg.BasicBlock is v1m1.BasicBlock


def test_scannet_config_state_dict_equals_the_listing(golden_dir):
    from pointcept.models import build_model, PDBatchNorm
    from ptv3_hip.configs import PPT_SPUNET_SCANNET_CFG
    keep = copy.deepcopy(PPT_SPUNET_SCANNET_CFG)
    model = build_model(PPT_SPUNET_SCANNET_CFG)
    assert PPT_SPUNET_SCANNET_CFG == keep
    with open(os.path.join(golden_dir, "state_dict_ppt_spunet_scannet.txt")) as f:
        want = [line.rstrip("\n") for line in f]
    assert _listing(model) == want
    pds = [m for m in model.modules() if isinstance(m, PDBatchNorm)]
    assert len(pds) == 59
    assert sum(m.modulation[1].weight.numel() for m in pds) == 4390912
    assert len(model.backbone.state_dict()) == 1062


def test_default_constructor_matches_the_issue_counts():
    from pointcept.models import build_model
    model = build_model(dict(type="SpUNet-v1m3", in_channels=6))
    sd = model.state_dict()
    assert len(sd) == 708
    assert "conv_input.conv.weight" in sd and "conv_input.bn.bns.0.running_mean" in sd
    assert "dec.0.block0.proj_conv.weight" in sd and "dec.0.block0.proj_norm.modulation.1.weight" in sd
    assert not any(k.endswith("bns.0.weight") or k.endswith("bns.0.bias") for k in sd)        # norm_affine=False
    # zero_init=True: every modulation Linear is zero, after the trunc-normal of the Linear itself
    mods = [v for k, v in sd.items() if ".modulation.1." in k]
    assert len(mods) == 2 * 59 and not any(v.any() for v in mods)
    single = build_model(dict(type="SpUNet-v1m3", in_channels=6, norm_decouple=False))
    keys = list(single.state_dict())
    assert "conv_input.bn.bn.running_mean" in keys and not any(".bns." in k for k in keys)


def test_tiny_model_lists_the_fixture_keys(golden_dir):
    from pointcept.models import build_model
    g = load_golden(golden_dir, "affine")
    model = build_model(dict(type="PPT-v1m2", **tiny_kw("affine")))
    assert list(model.state_dict()) == [str(k) for k in g["state_keys"]]
    assert len(model.backbone.state_dict()) == 594
    from ptv3_hip.configs import SPUNET_PDNORM_TINY_CFG
    assert list(build_model(SPUNET_PDNORM_TINY_CFG).state_dict()) == list(model.backbone.state_dict())


def test_constructor_and_input_refusals():
    from pointcept.models import build_model
    with pytest.raises(ValueError, match="zero_init.*norm_adaptive"):
        build_model(dict(type="SpUNet-v1m3", in_channels=4, zero_init=True, norm_adaptive=False))
    kw = dict(tiny_kw("affine")["backbone"])
    model = build_model(kw).eval()
    n = 12
    data = dict(grid_coord=torch.randint(0, 8, (n, 3)), feat=torch.randn(n, 4), offset=torch.tensor([n]),
                coord=torch.randn(n, 3))
    ctx = torch.randn(1, kw["context_channels"])
    with pytest.raises(KeyError, match="'D'.*'A', 'B', 'C'"):
        model(dict(data, condition="D", context=ctx))
    with pytest.raises(KeyError, match="'D'"):
        model(dict(data, condition=["D"], context=ctx))
    with pytest.raises(ValueError, match="context"):
        model(dict(data, condition="B"))
    with pytest.raises(ValueError, match=r"context.*\(2, 24\)"):
        model(dict(data, condition="B", context=torch.randn(2, kw["context_channels"])))


@pytest.mark.parametrize("affine", [True, False])
def test_reference_identities_against_autograd(affine):
    """bn(x) * (1 + scale) + shift with batch statistics, the reference's statement order, in float64 under autograd,
    against pdnorm_ref: one BatchNorm with (gamma_eff, beta_eff), and the backward identities from d gamma_eff / d beta_eff"""
    widths, cc = (4, 20, 96), 24
    layers, context = R.make_layers(widths, cc, affine, seed=5, magnitude=1.0)
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(37, c, generator=g, dtype=torch.float64) * 2 + 0.5 for c in widths]
    rs = [torch.randn(37, c, generator=g, dtype=torch.float64) for c in widths]
    leaves = [context] + [t for ly in layers for t in (ly["W"], ly["b"], ly["gamma"], ly["beta"]) if t is not None]
    for t in leaves:
        t.requires_grad_(True)
    loss, ys = 0.0, []
    for ly, x, r in zip(layers, xs, rs):
        feat = F.batch_norm(x, None, None, ly["gamma"], ly["beta"], training=True, eps=1e-3)
        shift, scale = F.linear(F.silu(context), ly["W"], ly["b"]).chunk(2, dim=1)
        ys.append(feat * (1.0 + scale) + shift)
        loss = loss + (ys[-1] * r).sum()
    loss.backward()

    det = [{k: None if v is None else v.detach() for k, v in ly.items()} for ly in layers]
    pairs = R.forward(context.detach(), det)
    d0, d1 = [], []
    for (ge, be, _), x, r, y in zip(pairs, xs, rs, ys):
        ge, be = ge.clone().requires_grad_(True), be.clone().requires_grad_(True)
        mine = F.batch_norm(x, None, None, ge, be, training=True, eps=1e-3)
        assert (mine - y.detach()).abs().max().item() <= 1e-12 * max(1.0, y.abs().max().item())
        (mine * r).sum().backward()
        d0.append(ge.grad)
        d1.append(be.grad)
    outs, dctx = R.backward(context.detach(), det, d0, d1)

    def close(name, got, want):
        assert (got - want).abs().max().item() <= 1e-10 * want.abs().max().item(), name
    close("dcontext", dctx, context.grad)
    for i, (ly, (dW, db, dg, dbeta)) in enumerate(zip(layers, outs)):
        close(f"dW{i}", dW, ly["W"].grad)
        close(f"db{i}", db, ly["b"].grad)
        if affine:
            close(f"dgamma{i}", dg, ly["gamma"].grad)
            close(f"dbeta{i}", dbeta, ly["beta"].grad)
        else:
            assert dg is None and dbeta is None


def test_entry_points_refuse_bad_arguments():
    """code 1 (PTV3_ERR_ARG) and a message before any pointer is touched: the pointers here are not addresses"""
    from ptv3_hip.lib import lib, PTV3_ERR_ARG
    fake = 0x1000
    w = (ctypes.c_int32 * 3)(4, 20, 96)

    def fwd(widths=w, L=3, cc=24, fold=0, stats=1, out0=fake, out1=fake, table=fake, context=fake):
        return lib.ptv3_pdnorm_fwd(table, widths, L, cc, context, fold, stats, 1e-3, out0, out1, None, None)

    def bwd(widths=w, L=3, cc=24, dW=fake, dctx=fake, d0=fake):
        return lib.ptv3_pdnorm_bwd(fake, widths, L, cc, fake, d0, fake, fake, dW, fake, None, None, fake, dctx, None)

    def refused(rc, word):
        assert rc == PTV3_ERR_ARG == 1
        assert word in lib.ptv3_last_error().decode(), lib.ptv3_last_error()
    refused(fwd(out0=None), "NULL")
    refused(fwd(out1=None), "NULL")
    refused(fwd(table=None), "NULL")
    refused(fwd(context=None), "NULL")
    refused(fwd(L=0), "L=0")
    refused(fwd(widths=(ctypes.c_int32 * 3)(4, 0, 96)), "width 0")
    refused(fwd(widths=(ctypes.c_int32 * 3)(4, 20, 4097)), "width 4097")
    refused(fwd(cc=0), "Cc=0")
    refused(fwd(cc=1025), "Cc=1025")
    refused(fwd(fold=1, stats=0), "running statistics")
    refused(bwd(dW=None), "NULL")
    refused(bwd(dctx=None), "NULL")
    refused(bwd(d0=None), "NULL")
    refused(bwd(L=0), "L=0")
    refused(bwd(widths=(ctypes.c_int32 * 3)(4, 20, 5000)), "width 5000")
    refused(bwd(dW=fake + 4), "aligned")
    assert lib.ptv3_pdnorm_capable(4, 1) and lib.ptv3_pdnorm_capable(260, 100) and lib.ptv3_pdnorm_capable(256, 256)
    assert not lib.ptv3_pdnorm_capable(0, 24) and not lib.ptv3_pdnorm_capable(16, 2048)
    assert 1 <= lib.ptv3_pdnorm_partial_rows(4) <= lib.ptv3_pdnorm_partial_rows(1 << 20) <= 512


def test_sync_batchnorm_is_adopted_inside_pdbatchnorm():
    from pointcept.models import build_model, PDBatchNorm
    from pointcept.models.utils.hip_layers import BatchNorm1d, adopt_sync_batchnorm
    model = build_model(dict(tiny_kw("affine")["backbone"]))
    keys = list(model.state_dict())
    bufs, params = list(model.buffers()), list(model.parameters())
    model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
    pds = [m for m in model.modules() if isinstance(m, PDBatchNorm)]
    assert all(isinstance(bn, torch.nn.SyncBatchNorm) for m in pds for bn in m.bns)
    assert adopt_sync_batchnorm(model) == 33 * len(CONDITIONS)
    assert all(type(bn) is BatchNorm1d and bn.sync_group is True for m in pds for bn in m.bns)
    assert all(a is b for a, b in zip(bufs, model.buffers())) and all(a is b for a, b in zip(params, model.parameters()))
    assert list(model.state_dict()) == keys
    assert all(m.active("B") is m.bns[1] for m in pds)
