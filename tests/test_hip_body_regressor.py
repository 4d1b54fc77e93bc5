"""PigBodyRegressor and DefaultClassifier on the GPU: the reference's own outputs (tests/golden/body_regressor_tiny.npz,
written by make_golden_body_regressor.py) with the fused batch head and with the composed one, through the native
executor and module by module (the first model here with head dimension 32 in a PT-v3m1 encoder), hooks on the head, the
result dicts, and arbitrary criteria through the given-dlogits mode of the training head.

Tolerances are those test_hip_keypoint_regression.py holds the same quantities to: 1e-4 absolute on fp32 predictions and
losses; the e_* are 100 x a mean absolute difference of predictions, so 1e-2; gradients 2e-3 (head) / 1e-2 (backbone) of
the tensor's largest entry; running statistics 1e-4 relative."""
import os

import numpy as np
import pytest
import torch

from make_golden_cfg import TINY_CFG  # noqa: E402

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
ERROR_KEYS = ("e_Len", "e_Wid", "e_Hei", "e_Che", "e_Wai", "e_Hip", "e_Wei")
BODY_TINY_BACKBONE = dict(TINY_CFG, drop_path=0.0, enc_num_head=(1, 1, 1, 1, 2))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "body_regressor_tiny.npz")))
    g.update(np.load(os.path.join(golden_dir, "body_regressor_tiny_backbone_grads.npz")))
    base = np.load(os.path.join(golden_dir, "ptv3_tiny_train.npz"))
    sd = {k[3:]: torch.from_numpy(base[k]) for k in base.files if k.startswith("sd_backbone.")}
    sd.update({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd_")})
    return g, sd


def _model(sd, dev, fused=True):
    from pointcept.models import build_model
    model = build_model(dict(type="PigBodyRegressor", num_classes=7, backbone_embed_dim=16,
                             criteria=[dict(type="RegressionL1Loss", loss_weight=1.0)],
                             backbone=dict(type="PT-v3m1", **BODY_TINY_BACKBONE)))
    model.load_state_dict(sd, strict=True)
    model.cls_head[3].p = model.cls_head[7].p = 0.0
    return model.to(dev).set_fused(fused)


def _data(g, dev):
    return {k[3:]: torch.from_numpy(v).to(dev) for k, v in g.items() if k.startswith("in_")}


def _errors(out):
    for k in ERROR_KEYS:
        assert out[k].dim() == 0 and out[k].is_cuda and not out[k].requires_grad, k
    return np.array([out[k].item() for k in ERROR_KEYS])


@pytest.mark.parametrize("use_engine", [True, False], ids=["executor", "modules"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_eval_vs_reference_golden(dev, golden, fused, use_engine):
    g, sd = golden
    model = _model(sd, dev, fused).eval()
    assert model._fused_eval() == fused and 3 <= model.fused_eval_max_scenes
    model.backbone.use_engine = use_engine
    data = _data(g, dev)
    torch.manual_seed(int(g["shuffle_seed"]))
    with torch.no_grad():
        out = model(dict(data))
    assert sorted(out) == sorted(("loss", "cls_logits") + ERROR_KEYS)
    assert tuple(out["cls_logits"].shape) == (3, 7) and out["cls_logits"].dtype == torch.float32
    err = np.abs(out["cls_logits"].cpu().numpy() - g["eval_logits"]).max()
    print("eval logits", err, "loss", out["loss"].item(), float(g["eval_loss"]))
    assert err < FP32_TOL
    assert abs(out["loss"].item() - float(g["eval_loss"])) < FP32_TOL
    assert np.abs(_errors(out) - g["eval_errors"]).max() < 100 * FP32_TOL
    # without "category": the logits alone, and the same ones
    torch.manual_seed(int(g["shuffle_seed"]))
    with torch.no_grad():
        bare = model({k: v for k, v in data.items() if k != "category"})
    assert sorted(bare) == ["cls_logits"]
    assert (bare["cls_logits"] - out["cls_logits"]).abs().max().item() < FP32_TOL


def test_eval_bf16_forward(dev, golden):
    """bf16 compute: backbone features bf16, head fp32; the bound of the sibling tests"""
    g, sd = golden
    model = _model(sd, dev).eval()
    assert model._fused_eval()
    model.backbone.compute_dtype = torch.bfloat16
    torch.manual_seed(int(g["shuffle_seed"]))
    with torch.no_grad():
        out = model(_data(g, dev))
    err = np.abs(out["cls_logits"].cpu().numpy() - g["eval_logits"])
    scale = max(1.0, float(np.abs(g["eval_logits"]).max()))
    assert err.max() < 64 * 2.0 ** -8 * scale and err.mean() < 8 * 2.0 ** -8 * scale, (err.max(), err.mean())


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_train_step_vs_reference_golden(dev, golden, fused):
    """Loss, e_*, every parameter gradient and the head's running statistics of one training step (drop_path = 0, both
    Dropouts at p = 0)."""
    g, sd = golden
    model = _model(sd, dev, fused).train()
    if fused:
        assert model._fused_train()
    data = _data(g, dev)
    torch.manual_seed(int(g["shuffle_seed"]))
    out = model(dict(data))
    assert sorted(out) == sorted(("loss",) + ERROR_KEYS)
    out["loss"].backward()
    assert abs(out["loss"].item() - float(g["loss"])) < FP32_TOL
    assert np.abs(_errors(out) - g["errors"]).max() < 100 * FP32_TOL
    grads = {k[5:]: torch.from_numpy(g[k].astype(np.float32) * g["gmax_" + k[5:]]) for k in g if k.startswith("grad_")}
    gmax = max(float(g[k]) for k in g if k.startswith("gmax_"))
    # the biases of the two Linears in front of a batch-statistic BatchNorm have an exact gradient of zero (the batch
    # mean removes any shift): both sides hold rounding noise, held to noise level against that layer's weight
    zero = ("cls_head.0.bias", "cls_head.4.bias")
    for n in zero:
        noise = dict(model.named_parameters())[n].grad.abs().max().item()
        assert noise <= 1e-4 * grads[n.replace("bias", "weight")].abs().max().item(), (n, noise)
    worst = max(((n, (p.grad.float().cpu() - grads[n]).abs().max().item()
                  / max(grads[n].abs().max().item(), 1e-3 * gmax)) for n, p in model.named_parameters()
                 if n not in zero), key=lambda t: t[1])
    print("worst gradient", worst)
    assert worst[1] < (2e-3 if worst[0].startswith("cls_head.") else 1e-2), worst
    for n, b in model.named_buffers():
        if "running" in n and n.startswith("cls_head."):
            ref = torch.from_numpy(g["buf_" + n])
            assert (b.cpu() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-6) < 1e-4, n
        if n.startswith("cls_head.") and n.endswith("num_batches_tracked"):
            assert b.item() == 1


def test_forward_hook_on_the_head_fires_once(dev, golden):
    """A user's hook on cls_head[8] sees the logits, once per forward (the hooked head takes the composed path), and
    the result is the unhooked one."""
    g, sd = golden
    model = _model(sd, dev).eval()
    data = _data(g, dev)
    torch.manual_seed(int(g["shuffle_seed"]))
    with torch.no_grad():
        plain = model(dict(data))
    seen = []
    handle = model.cls_head[8].register_forward_hook(lambda m, i, o: seen.append(o))
    assert not model._head_plain()
    torch.manual_seed(int(g["shuffle_seed"]))
    with torch.no_grad():
        hooked = model(dict(data))
    handle.remove()
    assert model._head_plain()
    assert len(seen) == 1 and torch.equal(seen[0], hooked["cls_logits"])
    assert (hooked["cls_logits"] - plain["cls_logits"]).abs().max().item() < FP32_TOL
    assert abs(hooked["loss"].item() - plain["loss"].item()) < FP32_TOL
    assert np.abs(_errors(hooked) - _errors(plain)).max() < 100 * FP32_TOL


def test_default_classifier_arbitrary_criteria_train_step(dev, golden):
    """DefaultClassifier on an encoder-only backbone with [CrossEntropyLoss, LovaszLoss]: the fused training head in its
    given-dlogits mode against the composed path - loss and head gradients (Dropouts at p = 0: the two paths draw
    their masks differently)."""
    from pointcept.models import build_model
    g, _ = golden
    cfg = dict(type="DefaultClassifier", num_classes=5, backbone_embed_dim=64,
               criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1),
                         dict(type="LovaszLoss", mode="multiclass", loss_weight=1.0, ignore_index=-1)],
               backbone=dict(type="PT-v3m1", **dict(BODY_TINY_BACKBONE, enc_mode=True)))
    torch.manual_seed(21)
    model = build_model(cfg).to(dev).train()
    model.cls_head[3].p = model.cls_head[7].p = 0.0
    data = {k: v for k, v in _data(g, dev).items() if k != "category"}
    data["category"] = torch.tensor([1, 4, 0], device=dev)
    results = {}
    for fused in (True, False):
        model.set_fused(fused)
        assert model._fused_train() == fused and model._l1() is None
        model.zero_grad(set_to_none=True)
        torch.manual_seed(9)
        out = model(dict(data))
        assert sorted(out) == ["loss"]
        out["loss"].backward()
        results[fused] = (out["loss"].item(), {n: p.grad.clone() for n, p in model.cls_head.named_parameters()})
    (lf, gf), (lc, gc) = results[True], results[False]
    assert abs(lf - lc) < 1e-5 * max(1.0, abs(lc)), (lf, lc)
    for n in gc:
        if n in ("0.bias", "4.bias"):   # exact zero behind the batch mean: noise on both sides
            assert gf[n].abs().max().item() <= 1e-4 * gc[n.replace("bias", "weight")].abs().max().item(), n
            continue
        assert (gf[n] - gc[n]).abs().max().item() <= 1e-4 * max(gc[n].abs().max().item(), 1e-3), n
    model.eval()
    with torch.no_grad():
        out = model(dict(data))
    assert sorted(out) == ["cls_logits", "loss"] and tuple(out["cls_logits"].shape) == (3, 5)
