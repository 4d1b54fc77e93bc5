"""Build-container-only: run the reference's PigBodyRegressor (pointcept/models/pig_regressor.py over DefaultClassifier,
pointcept/models/default.py:289-338, with RegressionL1Loss; imported in place through ref_loader's stubs) on a seeded
three-scene batch and store, in body_regressor_tiny.npz (the backbone's gradients apart, in
body_regressor_tiny_backbone_grads.npz, so that neither file is larger than keypoint_ptv3_tiny.npz): the inputs (with
`category` (3, 7)), the head's state_dict (BatchNorm buffers perturbed), the pooled (3, 16) features of the eval run,
the eval `cls_logits`, loss and seven column errors, and one training step (loss, errors, every parameter gradient, the updated running statistics of both head
BatchNorms).  The backbone is TINY_CFG with drop_path = 0 and enc_num_head = (1, 1, 1, 1, 2) - head dimensions 16, 16,
32, 32, 32, as the real config has 32 in its encoder - and carries the weights of ptv3_tiny_train.npz (head counts do not
change parameter shapes).  Both Dropouts of the head are at p = 0: the RNG streams cannot be shared between CPU and
device.  Gradients are stored as float16 of grad / max|grad| plus that fp32 maximum, as in
make_golden_keypoint_regression.py.  Also lists the state_dict of the reference class built from
configs/my_dataset/ptv3_weight.py.
usage: python tests/golden/make_golden_body_regressor.py"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "pointcept-keypointdetection_amd"))
import ptv3_scenes as S  # noqa: E402
import ref_loader  # noqa: E402
from make_golden_cfg import TINY_CFG  # noqa: E402
from make_golden_keypoint_regression import perturb_bn, write_listing  # noqa: E402
from make_golden_swin3d import _cfg  # noqa: E402

BODY_TINY_BACKBONE = dict(TINY_CFG, drop_path=0.0, enc_num_head=(1, 1, 1, 1, 2))
ERROR_KEYS = ("e_Len", "e_Wid", "e_Hei", "e_Che", "e_Wai", "e_Hip", "e_Wei")


def main():
    assert ref_loader.available()
    ref_loader.load()
    importlib.import_module("pointcept.models.pig_regressor")
    from pointcept.models.builder import MODELS
    torch.manual_seed(1234)
    model = MODELS.build(dict(type="PigBodyRegressor", num_classes=7, backbone_embed_dim=16,
                              criteria=[dict(type="RegressionL1Loss", loss_weight=1.0)],
                              backbone=dict(type="PT-v3m1", **BODY_TINY_BACKBONE)))
    model.cls_head[3].p = model.cls_head[7].p = 0.0
    perturb_bn(model)
    base = np.load(os.path.join(HERE, "ptv3_tiny_train.npz"))
    bb = {k[3 + len("backbone."):]: torch.from_numpy(base[k]) for k in base.files if k.startswith("sd_backbone.")}
    model.backbone.load_state_dict(bb, strict=True)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    sizes = [900, 400, 1300]
    data = S.make_batch(sizes, in_channels=4, extent=48, seed=11)
    g = torch.Generator().manual_seed(5)
    data["category"] = torch.rand(len(sizes), 7, generator=g) + 0.3
    res = {"in_" + k: v.numpy() for k, v in data.items()}
    res.update({"sd_" + k: v.numpy() for k, v in sd0.items() if not k.startswith("backbone.")})
    cap = {}
    handle = model.cls_head.register_forward_pre_hook(lambda m, a: cap.__setitem__("pooled", a[0].detach().clone()))
    torch.manual_seed(7)
    with torch.no_grad():
        out = model.eval()(dict(data))
        handle.remove()   # the next call draws other serialization orders: its pooled rows are not those of `out`
        bare = model(dict({k: v for k, v in data.items() if k != "category"}))
    assert sorted(bare) == ["cls_logits"]
    res["eval_pooled"] = cap["pooled"].numpy()
    res["eval_logits"], res["eval_loss"] = out["cls_logits"].numpy(), out["loss"].numpy()
    res["eval_errors"] = np.array([out[k].item() for k in ERROR_KEYS], dtype=np.float32)
    torch.manual_seed(7)
    out = model.train()(dict(data))
    out["loss"].backward()
    res["loss"] = out["loss"].detach().numpy()
    res["errors"] = np.array([out[k].item() for k in ERROR_KEYS], dtype=np.float32)
    for k, p in model.named_parameters():
        top = p.grad.abs().max().clamp(min=1e-30)
        res["grad_" + k] = (p.grad / top).to(torch.float16).numpy()
        res["gmax_" + k] = top.numpy()
    res.update({"buf_" + k: b.detach().numpy() for k, b in model.named_buffers()
                if "running" in k and k.startswith("cls_head.")})
    res["shuffle_seed"] = np.array(7)
    # two files, so that each stays below the size of keypoint_ptv3_tiny.npz: the backbone's gradients on their own
    parts = {"body_regressor_tiny_backbone_grads.npz": {k: v for k, v in res.items() if "_backbone." in k}}
    parts["body_regressor_tiny.npz"] = {k: v for k, v in res.items() if "_backbone." not in k}
    for name, part in parts.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        print(name, os.path.getsize(path) // 1024, "KiB")
    print("eval loss", float(res["eval_loss"]), "; train loss", float(res["loss"]))
    write_listing(MODELS.build(_cfg("configs/my_dataset/ptv3_weight.py")), "state_dict_pig_body_regressor_fork.txt")


if __name__ == "__main__":
    main()
