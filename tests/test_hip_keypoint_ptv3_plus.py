"""KeypointPTv3Plus / PT-v3m1-Plus on the GPU against the reference's own outputs (tests/golden/keypoint_ptv3_plus_tiny*.npz,
written by make_golden_keypoint_ptv3_plus.py): the re-serialization orders exactly, every encoder / decoder stage, `pred`
and the loss in eval, fused against composed, bf16 compute, one training step (loss, curves, every gradient, running
statistics), a kernel size the fused kernel does not serve, and the fork config at 8 x 20 000 sites.

Eval bound: max(FP32_TOL, 4 x eval_fp64_gap) - FP32_TOL = 1e-4 is the project's fp32 budget, eval_fp64_gap the distance
of the reference's fp32 `pred` from its own float64 run, measured by the maker on the reference alone."""
import os

import numpy as np
import pytest
import torch

from make_golden_keypoint_ptv3_plus import PLUS_TINY_CFG
from keypoint_ptv3_plus_params import seeded_state_dict

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


_G = {}


def _golden(golden_dir):
    if not _G:
        for part in ("", "_enc", "_dec", "_grad_cpe", "_grad_rest"):
            z = np.load(os.path.join(golden_dir, f"keypoint_ptv3_plus_tiny{part}.npz"))
            _G.update({k: z[k] for k in z.files})
    return _G


def _tiny_model(dev, **override):
    from pointcept.models import build_model
    model = build_model(dict(type="KeypointPTv3Plus", num_keypoints=6, hidden_dim=32,
                             backbone_conf=dict(type="PT-v3m1-Plus", **dict(PLUS_TINY_CFG, **override))))
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    return model.to(dev)


def _data(g, dev):
    return {k[3:]: torch.from_numpy(v).to(dev) for k, v in g.items() if k.startswith("in_")}


def _run_eval(model, g, data, taps=None):
    handles = []
    if taps is not None:
        bb = model.backbone
        for s, stage in enumerate(bb.enc_stages):
            last = list(stage.children())[-1]
            handles.append(last.register_forward_hook(
                lambda m, i, o, s=s: taps.__setitem__(f"enc_{s}", o.feat.detach().float().cpu().numpy())))
        for name, dec in bb.dec.named_children():
            handles.append(dec.register_forward_hook(
                lambda m, i, o, name=name: taps.__setitem__(name, o.feat.detach().float().cpu().numpy())))
    torch.manual_seed(int(g["shuffle_seed"]))
    with torch.no_grad():
        out = model(dict(data))
    for h in handles:
        h.remove()
    return out


def test_eval_vs_reference_golden(dev, golden_dir, monkeypatch):
    from pointcept.models import keypoint_ptv3_plus as mod
    g = _golden(golden_dir)
    tol = max(FP32_TOL, 4 * float(g["eval_fp64_gap"]))
    model = _tiny_model(dev).eval()
    data = _data(g, dev)
    taps = {}
    orders = []
    real = mod.reserialize
    monkeypatch.setattr(mod, "reserialize", lambda point, perm: orders.append(real(point, perm).cpu().numpy()))
    out = _run_eval(model, g, data, taps)
    monkeypatch.undo()
    # the orders first: a wrong order moves every later number.  Stages 1, 2 and 4 reorder, 0 and 3 do not
    assert len(orders) == 3 and g["order_0"].size == 0 and g["order_3"].size == 0
    for got, s in zip(orders, (1, 2, 4)):
        assert got.dtype == np.int64 and np.array_equal(got, g[f"order_{s}"]), f"order of stage {s}"
    for key in [f"enc_{s}" for s in range(5)] + [f"dec{s}" for s in (3, 2, 1, 0)]:
        assert taps[key].shape == g[key].shape, key
        err = np.abs(taps[key] - g[key]).max()
        print(f"{key}: max error {err:.3e} at scale {np.abs(g[key]).max():.3f}")
        assert err < tol, (key, err)
    assert tuple(out["pred"].shape) == (3, 6, 3) and out["pred"].dtype == torch.float32
    assert np.abs(out["pred"].cpu().numpy() - g["eval_pred"]).max() < tol
    assert abs(out["loss"].item() - float(g["eval_loss"])) < tol
    # the composed path (the reference's statement order on the unfused ops) within the same bound, of the reference
    # and of the fused path
    fused_pred = out["pred"]
    model.set_fused(False)
    comp = _run_eval(model, g, data)
    assert np.abs(comp["pred"].cpu().numpy() - g["eval_pred"]).max() < tol
    assert (comp["pred"] - fused_pred).abs().max().item() < tol
    model.set_fused(True)
    # the wiring rule sends the 125-tap convolution to its composition at present: with ptv3_subm_conv_ln switched in
    # for the fixture's width the model stays within the same bound
    monkeypatch.setattr(mod, "FUSED_CONV_ON", frozenset({(16, 125, torch.float32)}))
    assert mod.use_fused_cpe(64, 16, 125, torch.float32) == (True, True)
    conv = _run_eval(model, g, data)
    monkeypatch.undo()
    assert np.abs(conv["pred"].cpu().numpy() - g["eval_pred"]).max() < tol
    assert (conv["pred"] - fused_pred).abs().max().item() < tol
    # int32 offsets give identical bits
    out32 = _run_eval(model, g, dict(data, offset=data["offset"].int()))
    assert torch.equal(out32["pred"], fused_pred)
    # bf16 compute: backbone features bf16, head fp32; the bound of test_keypoint_ptv3_eval_vs_reference_golden
    model.backbone.compute_dtype = torch.bfloat16
    out16 = _run_eval(model, g, data)
    err = np.abs(out16["pred"].cpu().numpy() - g["eval_pred"])
    scale = max(1.0, float(np.abs(g["eval_pred"]).max()))
    print(f"bf16 pred error max {err.max():.3e} mean {err.mean():.3e}")
    assert err.max() < 64 * 2.0 ** -8 * scale and err.mean() < 8 * 2.0 ** -8 * scale, (err.max(), err.mean())


def test_train_step_vs_reference_golden(dev, golden_dir):
    """Loss, curves, every parameter gradient and the running statistics of one training step (drop_path = 0, the head's
    Dropout at p = 0), with the tolerances of test_keypoint_ptv3_train_step_vs_reference_golden: 2e-3 for the head,
    1e-2 for the backbone, 1e-4 for the running statistics."""
    g = _golden(golden_dir)
    model = _tiny_model(dev).train()
    model.reg_head[3].p = 0.0
    data = _data(g, dev)
    torch.manual_seed(int(g["shuffle_seed"]))
    out = model(dict(data))
    out["loss"].backward()
    assert abs(out["loss"].item() - float(g["loss"])) < 1e-4
    assert abs(out["train/mean_dist"].item() - float(g["mean_dist"])) < 1e-4
    assert np.abs(np.array([out[f"train/kp{i}_dist"].item() for i in range(6)]) - g["kp_dist"]).max() < 1e-4
    grads = {k[5:]: torch.from_numpy(g[k].astype(np.float32) * g["gmax_" + k[5:]]) for k in g if k.startswith("grad_")}
    assert set(grads) == {n for n, _ in model.named_parameters()}
    gmax = max(float(g[k]) for k in g if k.startswith("gmax_"))
    bias0 = model.reg_head[0].bias.grad.abs().max().item()      # exact zero behind the batch-statistic BatchNorm
    assert bias0 <= 1e-4 * grads["reg_head.0.weight"].abs().max().item(), bias0
    rel = {n: (p.grad.float().cpu() - grads[n]).abs().max().item() / max(grads[n].abs().max().item(), 1e-3 * gmax)
           for n, p in model.named_parameters() if n != "reg_head.0.bias"}
    worst = max(rel.items(), key=lambda t: t[1])
    worst_cpe = max(((n, v) for n, v in rel.items() if n.endswith("cpe.3.weight")), key=lambda t: t[1])
    print(f"worst gradient {worst}, worst 5^3 weight gradient {worst_cpe}")
    for n, v in rel.items():
        assert v < (2e-3 if n.startswith("reg_head.") else 1e-2), (n, v)
    for n, b in model.named_buffers():
        if "running" in n:
            ref = torch.from_numpy(g["buf_" + n])
            assert (b.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6) < 1e-4, n


def test_one_scene_training_raises(dev, golden_dir):
    g = _golden(golden_dir)
    model = _tiny_model(dev).train()
    data = _data(g, dev)
    n0 = int(data["offset"][0])
    one = {k: v[:n0] for k, v in data.items() if k not in ("offset", "target", "scale", "grid_size")}
    one.update(offset=data["offset"][:1], target=data["target"][:6], grid_size=data["grid_size"][:1])
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        model(one)


def test_kernel_size_7_takes_the_composed_path(dev, golden_dir):
    """cpe_kernel_size = 7 (343 taps) is not served by ptv3_subm_conv_ln: the block composes it from the unfused ops
    without being told; the fused front and the folded expand GEMM still run.  Compared against set_fused(False) only."""
    from ptv3_hip import ops
    g = _golden(golden_dir)
    assert not ops.subm_conv_ln_capable(16, 343, torch.float32)
    model = _tiny_model(dev, cpe_kernel_size=7).eval()
    assert tuple(model.backbone.enc_stages[0].block0.cpe[3].weight.shape) == (16, 7, 7, 7, 16)
    data = _data(g, dev)
    out = _run_eval(model, g, data)
    comp = _run_eval(model.set_fused(False), g, data)
    assert torch.isfinite(out["pred"]).all()
    assert (out["pred"] - comp["pred"]).abs().max().item() < FP32_TOL


def test_fork_config_at_8x20000(dev):
    """The fork config on 8 scenes of 20 000 sites: runs in fp32 and bf16, finite predictions, fused against composed
    fp32 within the fp32 budget."""
    import ptv3_scenes as S
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_PTV3_PLUS_CFG
    torch.manual_seed(0)
    model = build_model(KEYPOINT_PTV3_PLUS_CFG).to(dev).eval()
    data = {k: v.to(dev) for k, v in S.make_batch([20000] * 8, in_channels=4, extent=256, seed=3).items()}
    preds = {}
    for name, fused, dtype in (("fused", True, torch.float32), ("composed", False, torch.float32),
                               ("bf16", True, torch.bfloat16)):
        model.set_fused(fused)
        model.backbone.compute_dtype = dtype
        torch.manual_seed(1)
        with torch.no_grad():
            preds[name] = model(dict(data))["pred"]
        assert tuple(preds[name].shape) == (8, 6, 3) and torch.isfinite(preds[name]).all(), name
    gap = (preds["fused"] - preds["composed"]).abs().max().item()
    print(f"fork config 8 x 20000: fused vs composed {gap:.3e}, bf16 vs fp32 "
          f"{(preds['bf16'] - preds['fused']).abs().max().item():.3e}")
    assert gap < FP32_TOL
