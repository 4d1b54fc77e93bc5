"""SpUNet-v1m1 / KeypointSparseUNet on the GPU: the model against the reference's own outputs
(tests/golden/keypoint_spunet_tiny.npz: eval taps, coarse sites, one training step, the enc_mode=True entry), the fused
eval forward against the torch composition, ptv3_res_conv forced on against forced off, the host-read count, the
segmentation backbone under DefaultSegmentorV2 and the fork config end to end.  Tolerances and the 4x rule are those of
test_hip_keypoint_oacnns.py."""
import numpy as np
import pytest
import torch

from make_golden_keypoint_spunet import seeded_state_dict, load_golden, TINY_KW, TAPS, TAP_STRIDE
from test_hip_keypoint_oacnns import FP32_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


_GOLDEN = {}


def _tiny(golden_dir, dev, **extra):
    from pointcept.models import build_model
    if not _GOLDEN:
        _GOLDEN.update(load_golden(golden_dir))
    g = _GOLDEN
    model = build_model(dict(type="KeypointSparseUNet", **TINY_KW, **extra))
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    data = {k[3:]: torch.from_numpy(v).to(dev) for k, v in g.items() if k.startswith("in_")}
    return g, model.to(dev), data


def _tapped_eval(model, data):
    taps = []
    with torch.no_grad():
        out = model.eval()(dict(data), taps=taps)
    assert len(taps) == len(TAPS)
    return out, dict(zip(TAPS, taps))


def _stored(feat, n_in):
    return feat[::TAP_STRIDE] if feat.shape[0] == n_in else feat


def _kernel_calls(monkeypatch):
    """counts ops.res_conv launches of a forward"""
    from ptv3_hip import ops
    calls, inner = [], ops.res_conv

    def counting(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    monkeypatch.setattr(ops, "res_conv", counting)
    return calls


def test_eval_vs_reference_golden(dev, golden_dir, monkeypatch):
    """Coarse site lists exactly; the nine taps, `pred` and the loss within FP32_TOL of the tap's scale; with the kernel
    on, every one of the 8 blocks' conv2 and the 4 decoder fronts runs ptv3_res_conv."""
    g, model, data = _tiny(golden_dir, dev)
    model.set_res_conv(True)
    calls = _kernel_calls(monkeypatch)
    out, taps = _tapped_eval(model, data)
    assert len(calls) == sum(TINY_KW["layers"]) + 4
    n_in = data["feat"].shape[0]
    for i in range(4):
        assert np.array_equal(taps[f"enc.{i}"].indices.cpu().numpy(), g[f"sites{i + 1}"]), i
    for name in TAPS:
        ref = g["tap_" + name]
        err = np.abs(_stored(taps[name].features, n_in).cpu().numpy() - ref).max()
        print(f"tap {name}: error {err:.3e}, scale {np.abs(ref).max():.3e}")
        assert err < FP32_TOL * np.abs(ref).max(), (name, err)
    assert tuple(out["pred"].shape) == (2, 6, 3) and out["pred"].dtype == torch.float32
    assert np.abs(out["pred"].cpu().numpy() - g["eval_pred"]).max() < FP32_TOL
    assert abs(out["loss"].item() - float(g["eval_loss"])) < FP32_TOL


def test_enc_mode_eval_vs_reference_golden(dev, golden_dir):
    """enc_mode=True: the head on the per-scene mean of the deepest level, scene ends derived on the device."""
    g, model, data = _tiny(golden_dir, dev, enc_mode=True)
    with torch.no_grad():
        out = model.eval()(dict(data))
    assert tuple(out["pred"].shape) == (2, 6, 3)
    assert np.abs(out["pred"].cpu().numpy() - g["enc_mode_eval_pred"]).max() < FP32_TOL
    assert abs(out["loss"].item() - float(g["enc_mode_eval_loss"])) < FP32_TOL


def _compare(g, name_a, a_taps, b_taps, n_in):
    """every row of every tap: |a - b| at most 4x b's own distance from the reference's fp32 run on the stored rows"""
    for name in TAPS:
        a, b, ref = a_taps[name].features, b_taps[name].features, g["tap_" + name]
        err = (a - b).abs().max().item()
        base = np.abs(_stored(b, n_in).cpu().numpy() - ref).max()
        print(f"tap {name}: {name_a} {err:.3e}, composed - reference {base:.3e}")
        assert err <= max(4 * base, 2.0 ** -23 * np.abs(ref).max()), (name, err, base)


def test_fused_eval_vs_composition(dev, golden_dir):
    """The fused eval forward (default wiring) against set_fused(False); the yardstick is the composition's own fp32
    error against the golden."""
    g, model, data = _tiny(golden_dir, dev)
    fused, taps = _tapped_eval(model, data)
    plain, ref_taps = _tapped_eval(model.set_fused(False), data)
    _compare(g, "fused - composed", taps, ref_taps, data["feat"].shape[0])
    assert (fused["pred"] - plain["pred"]).abs().max().item() < FP32_TOL
    assert abs(fused["loss"].item() - plain["loss"].item()) < FP32_TOL


def test_kernel_forced_on_and_off_agree(dev, golden_dir, monkeypatch):
    """model.set_res_conv(True) runs ptv3_res_conv in every block, set_res_conv(False) in none (ptv3_gemm + cat +
    add_act); both sit within 4x the composition's distance from the golden of the composition."""
    g, model, data = _tiny(golden_dir, dev)
    calls = _kernel_calls(monkeypatch)
    on, on_taps = _tapped_eval(model.set_res_conv(True), data)
    assert len(calls) == sum(TINY_KW["layers"]) + 4
    del calls[:]
    off, off_taps = _tapped_eval(model.set_res_conv(False), data)
    assert not calls
    plain, ref_taps = _tapped_eval(model.set_fused(False), data)
    n_in = data["feat"].shape[0]
    _compare(g, "kernel on - composed", on_taps, ref_taps, n_in)
    _compare(g, "kernel off - composed", off_taps, ref_taps, n_in)
    assert (on["pred"] - off["pred"]).abs().max().item() < FP32_TOL


def test_eval_reads_the_device_five_times(dev, golden_dir, monkeypatch):
    """One read at entry (spatial shape and offsets) and one per stage (the plan's counters); counted as in
    test_hip_keypoint_oacnns.py."""
    g, model, data = _tiny(golden_dir, dev)
    model.eval()
    with torch.no_grad():
        model(dict(data))            # parameter caches filled
    reads = []
    for name in ("tolist", "item", "cpu", "numpy"):
        inner = getattr(torch.Tensor, name)

        def counting(self, *a, _inner=inner, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _inner(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counting)
    with torch.no_grad():
        out = model(dict(data))
    monkeypatch.undo()
    assert reads == ["tolist"] * 5, reads
    assert np.abs(out["pred"].cpu().numpy() - g["eval_pred"]).max() < FP32_TOL


def test_train_step_vs_reference_golden(dev, golden_dir):
    """Loss, curves, every parameter gradient and the running statistics of one training step (the head's Dropout at
    p = 0), with check_step's tolerances (make_golden_keypoint_oacnns.py)."""
    g, model, data = _tiny(golden_dir, dev)
    model.train()
    model.reg_head[3].p = 0.0
    out = model(dict(data))
    out["loss"].backward()
    assert abs(out["loss"].item() - float(g["loss"])) < 1e-4
    assert abs(out["train/mean_dist"].item() - float(g["mean_dist"])) < 1e-4
    assert np.abs(np.array([out[f"train/kp{i}_dist"].item() for i in range(6)]) - g["kp_dist"]).max() < 1e-4
    grads = {k[5:]: torch.from_numpy(g[k].astype(np.float32) * g["gmax_" + k[5:]]) for k in g if k.startswith("grad_")}
    gmax = max(float(g[k]) for k in g if k.startswith("gmax_"))
    params = dict(model.named_parameters())
    assert set(params) == set(grads)
    # reg_head.0.bias stands straight in front of a batch-statistic BatchNorm: its exact gradient is zero, both sides
    # hold rounding noise, so it is held to noise level against its layer's weight
    zero = "reg_head.0.bias"
    assert params[zero].grad.abs().max().item() <= 1e-4 * params["reg_head.0.weight"].grad.abs().max().item()
    worst = ("", 0.0)
    for n, p in params.items():
        if n != zero:
            assert p.grad is not None and p.grad.abs().max().item() > 0, n
            err = (p.grad.float().cpu() - grads[n]).abs().max().item() / max(grads[n].abs().max().item(), 1e-3 * gmax)
            worst = max(worst, (n, err), key=lambda q: q[1])
            assert err < (2e-3 if n.startswith("reg_head.") else 1e-2), (n, err)
    print("worst gradient error", worst)
    for n, b in model.named_buffers():
        if "running" in n:
            ref = torch.from_numpy(g["buf_" + n])
            assert (b.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6) < 1e-4, n


def test_spunet_segmentor_fused_vs_composition(dev, golden_dir):
    """"SpUNet-v1m1" with its `final` 1x1x1 conv (13 classes) under DefaultSegmentorV2 on the golden's batch: fused
    eval against the composition."""
    from pointcept.models import build_model
    g, _, data = _tiny(golden_dir, dev)
    kw = {k: v for k, v in TINY_KW.items() if k not in ("num_keypoints", "hidden_dim")}
    model = build_model(dict(type="DefaultSegmentorV2", num_classes=0, backbone_out_channels=13,
                             backbone=dict(type="SpUNet-v1m1", num_classes=13, **kw),
                             criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)]))
    model.backbone.load_state_dict(seeded_state_dict(model.backbone.state_dict()), strict=True)
    model = model.to(dev).eval()
    batch = {k: data[k] for k in ("grid_coord", "feat", "offset", "coord")}
    with torch.no_grad():
        fused = model(dict(batch))["seg_logits"]
        model.backbone.set_fused(False)
        plain = model(dict(batch))["seg_logits"]
    assert tuple(fused.shape) == (data["feat"].shape[0], 13) and torch.isfinite(fused).all()
    assert (fused - plain).abs().max().item() < FP32_TOL * max(1.0, plain.abs().max().item())


def test_fork_config_eval_and_train_step(dev):
    """configs/my_dataset/keypoint_sparse_unet.py's model dict (23 BasicBlocks) on two scenes of 3000 sites."""
    import ptv3_scenes as S
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_SPUNET_CFG
    torch.manual_seed(7)
    model = build_model(KEYPOINT_SPUNET_CFG).to(dev)
    data = {k: v.to(dev) for k, v in S.make_batch([3000, 3000], in_channels=4, extent=64, seed=3).items()}
    data["target"] = torch.randn(12, 3, device=dev) * 0.5
    with torch.no_grad():
        pred = model.eval()(dict(data))["pred"]
    assert tuple(pred.shape) == (2, 6, 3) and torch.isfinite(pred).all()
    opt = torch.optim.AdamW(model.parameters(), lr=2e-3, weight_decay=0.05)
    out = model.train()(dict(data))
    out["loss"].backward()
    opt.step()
    assert torch.isfinite(out["loss"]).item()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and torch.isfinite(p).all() for p in model.parameters())
