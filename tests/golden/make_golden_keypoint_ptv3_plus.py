"""Build-container-only: run the reference's KeypointPTv3Plus (pointcept/models/keypoint_ptv3_plus.py, imported in place
through ref_loader's stubs plus the scatter_mean stand-in of make_golden_keypoint_regression.py) on a seeded three-scene
batch and store what it computes:

  keypoint_ptv3_plus_tiny.npz            inputs; eval `pred` and loss; per encoder stage the re-serialization order it
                                         applied (int64, empty where the stage is not reordered); one training step's
                                         loss, curves and BatchNorm running statistics (head Dropout at p = 0,
                                         drop_path = 0);
                                         `shuffle_seed`; `eval_fp64_gap` = max |pred32 - pred64| and, per tensor,
                                         `gap64_<name>` = max |grad32 - grad64| / max |grad64| of the same step run in
                                         float64 (the reference's own rounding, which bounds what parity can ask)
  keypoint_ptv3_plus_tiny_enc.npz        the output features of every encoder stage (enc_<s>)
  keypoint_ptv3_plus_tiny_dec.npz        the output features of every decoder stage (dec<s>)
  keypoint_ptv3_plus_tiny_grad_cpe.npz   the gradients of the ten 5^3 convolution weights
  keypoint_ptv3_plus_tiny_grad_rest.npz  every other parameter gradient
                                         (float16 of grad / max|grad| plus that fp32 maximum, as keypoint_ptv3_tiny.npz;
                                         separate files so that each stays under the size limit of a committed file)

The state dict is not stored as numbers: keypoint_ptv3_plus_params.seeded_state_dict draws it from the model's own key /
shape listing, here for the reference class and in the tests for this package's (both load it strict).
Config: TINY_CFG with enc_channels (16, 16, 64, 64, 64), dec_channels (16, 16, 64, 64), cpe_kernel_size 5: both
branches of the mid rule (16 -> 16, 64 -> 16), five stages and so both axis permutations, every 5^3 weight at 16
channels.  Asserts that every order is a permutation, that every z code is unique (the sort is unambiguous) and that the
float64 training loss agrees with the fp32 one to 1e-5.  Also lists the state_dict of the reference class built from
the fork config configs/my_dataset/keypoint_ptv3_plus.py.
usage: python tests/golden/make_golden_keypoint_ptv3_plus.py"""
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
from make_golden_keypoint_regression import scatter_mean, write_listing  # noqa: E402
from make_golden_swin3d import _cfg  # noqa: E402
from keypoint_ptv3_plus_params import seeded_state_dict  # noqa: E402

PLUS_TINY_CFG = dict(TINY_CFG, enc_channels=(16, 16, 64, 64, 64), enc_num_head=(1, 1, 4, 4, 4),
                     dec_channels=(16, 16, 64, 64), dec_num_head=(1, 1, 4, 4), cpe_kernel_size=5, drop_path=0.0)
SIZES = [900, 400, 1300]
SHUFFLE_SEED = 7


def make_model(kp):
    model = kp.KeypointPTv3Plus(backbone_conf=dict(type="PT-v3m1-Plus", **PLUS_TINY_CFG), num_keypoints=6,
                                hidden_dim=32)
    model.reg_head[3].p = 0.0
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    return model


def make_data():
    data = S.make_batch(SIZES, in_channels=4, extent=48, seed=11)
    g = torch.Generator().manual_seed(5)
    data["target"] = torch.randn(len(SIZES) * 6, 3, generator=g) * 0.5          # collated (B*K, 3)
    data["scale"] = torch.rand(len(SIZES), generator=g) + 0.5
    return data


class Taps:
    """Records, during one forward, the order of every re-serialization (Point.serialization called with the bare
    string "z", keypoint_ptv3_plus.py:407) and the output features of every encoder / decoder stage."""

    def __init__(self, ns, model):
        self.orders, self.enc, self.dec = [], {}, {}
        self.handles = []
        point_cls = ns.Point
        original = point_cls.serialization
        taps = self

        def serialization(self, order="z", depth=None, shuffle_orders=False):
            original(self, order=order, depth=depth, shuffle_orders=shuffle_orders)
            if isinstance(order, str):
                code = self.serialized_code[0]
                assert torch.unique(code).numel() == code.numel(), "z codes must be unique"
                taps.orders.append(self.serialized_order[0].clone())

        point_cls.serialization = serialization
        self.restore = lambda: setattr(point_cls, "serialization", original)
        bb = model.backbone
        for s, stage in enumerate(bb.enc_stages):
            last = list(stage.children())[-1]
            self.handles.append(last.register_forward_hook(
                lambda m, i, o, s=s: self.enc.__setitem__(s, o.feat.detach().clone())))
        for name, dec in bb.dec.named_children():
            self.handles.append(dec.register_forward_hook(
                lambda m, i, o, name=name: self.dec.__setitem__(name, o.feat.detach().clone())))

    def close(self):
        self.restore()
        for h in self.handles:
            h.remove()


def train_step(model, data):
    torch.manual_seed(SHUFFLE_SEED)
    out = model.train()(dict(data))
    out["loss"].backward()
    return out


def main():
    assert ref_loader.available()
    ns = ref_loader.load()
    sys.modules["torch_scatter"].scatter_mean = scatter_mean
    kp = importlib.import_module("pointcept.models.keypoint_ptv3_plus")
    data = make_data()
    model = make_model(kp)
    res = {"in_" + k: v.numpy() for k, v in data.items()}
    enc_out = {}

    taps = Taps(ns, model)
    torch.manual_seed(SHUFFLE_SEED)
    with torch.no_grad():
        out = model.eval()(dict(data))
    taps.close()
    res["eval_pred"], res["eval_loss"] = out["pred"].numpy(), out["loss"].numpy()
    stages = len(model.backbone.enc_stages)
    reordered = [s for s in range(stages) if s > 0 and s % 3 != 0]
    assert len(taps.orders) == len(reordered)
    for s in range(stages):
        order = taps.orders[reordered.index(s)] if s in reordered else torch.empty(0, dtype=torch.int64)
        if s in reordered:
            assert torch.equal(torch.sort(order).values, torch.arange(order.numel())), "order must be a permutation"
            assert order.numel() == taps.enc[s].shape[0]
        res[f"order_{s}"] = order.numpy().astype(np.int64)
        enc_out[f"enc_{s}"] = taps.enc[s].numpy()
    dec_out = {name: feat.numpy() for name, feat in taps.dec.items()}

    out = train_step(model, data)
    res["loss"] = out["loss"].detach().numpy()
    res["mean_dist"] = out["train/mean_dist"].numpy()
    res["kp_dist"] = np.array([out[f"train/kp{i}_dist"].item() for i in range(6)], dtype=np.float32)
    res.update({"buf_" + k: b.detach().numpy() for k, b in model.named_buffers() if "running" in k})
    res["shuffle_seed"] = np.array(SHUFFLE_SEED)

    # the same model in float64: what fp32 rounding alone moves in the reference
    model64 = make_model(kp).double()
    data64 = {k: (v.double() if v.is_floating_point() else v) for k, v in data.items()}
    torch.manual_seed(SHUFFLE_SEED)
    with torch.no_grad():
        out64 = model64.eval()(dict(data64))
    res["eval_fp64_gap"] = np.array(np.abs(res["eval_pred"].astype(np.float64) - out64["pred"].numpy()).max())
    out64 = train_step(model64, data64)
    assert abs(float(out64["loss"].detach()) - float(res["loss"])) < 1e-5
    g64 = dict(model64.named_parameters())

    grads = {"cpe": {}, "rest": {}}
    for k, p in model.named_parameters():
        top = p.grad.abs().max().clamp(min=1e-30)
        part = grads["cpe" if k.endswith("cpe.3.weight") else "rest"]
        part["grad_" + k] = (p.grad / top).to(torch.float16).numpy()
        part["gmax_" + k] = top.numpy()
        ref = g64[k].grad
        res["gap64_" + k] = np.array(float((p.grad.double() - ref).abs().max() / ref.abs().max().clamp(min=1e-30)))

    for fname, part in (("keypoint_ptv3_plus_tiny.npz", res),
                        ("keypoint_ptv3_plus_tiny_enc.npz", enc_out),
                        ("keypoint_ptv3_plus_tiny_dec.npz", dec_out),
                        ("keypoint_ptv3_plus_tiny_grad_cpe.npz", grads["cpe"]),
                        ("keypoint_ptv3_plus_tiny_grad_rest.npz", grads["rest"])):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **part)
        print(fname, os.path.getsize(path) // 1024, "KiB")
        assert os.path.getsize(path) < 1024 * 1024
    print("eval loss", float(res["eval_loss"]), "; train loss", float(res["loss"]), "; eval fp64 gap",
          float(res["eval_fp64_gap"]), "; worst gradient fp64 gap",
          max((float(v), k) for k, v in res.items() if k.startswith("gap64_")))

    from pointcept.models.builder import MODELS
    write_listing(MODELS.build(_cfg("configs/my_dataset/keypoint_ptv3_plus.py")),
                  "state_dict_keypoint_ptv3_plus_fork.txt")


if __name__ == "__main__":
    main()
