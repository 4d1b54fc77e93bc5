"""Build-container-only: run the reference's Point Prompt Training classes (pointcept/models/point_prompt_training/
point_prompt_training_v1m1_language_guided.py and ..._v1m2_decoupled.py, imported in place through ref_loader's stubs, with
the reference's real PDNorm put into the loaded PT-v3m1 module in place of ref_loader's dummy) over a tiny PT-v3m1 with
pdnorm_bn = pdnorm_ln = True, backbone_out_channels = 16, conditions ("A", "B", "C") and valid index lists of 5 / 7 / 3 out
of 9 class names.  `clip` is a stub: a seeded random text encoder of width 40 with unit rows and logit_scale = ln(100).
"PPT-v1m1" runs once with pdnorm_adaptive=False and once with True, "PPT-v1m2" once (not adaptive).

Stored per run in ppt_tiny_{v1m1,v1m1_adaptive,v1m2}.npz (+ ..._grads{i}.npz, the backbone's gradients): the inputs (three scenes, labels per condition with about a tenth
-1), class_embedding and logit_scale, for the conditions "B" and "C" the eval `seg_logits`, `loss` and backbone features
(the test dict's seg_logits is asserted equal to the eval dict's), for "B" the input and output of one BatchNorm PDNorm
(the stem's) and of one LayerNorm PDNorm (the first block's norm1) in eval and of the former in training, one training step
under "B": the loss, every parameter gradient as float16 of grad / max|grad| plus that fp32 maximum (parameters of the
inactive conditions have no gradient and are listed in `nograd`), every BatchNorm running statistic afterwards - and, as
`gap_*`, the largest difference of each tensor between this fp32 run and the same computation in float64.

Weights are not stored: ppt_state_dict() derives them from the key names (make_golden_keypoint_oacnns.seeded_state_dict,
so the norms of the three conditions differ, then perturb_bn) and the tests call the same function.  torch.manual_seed(SEED)
precedes every forward: the serialization shuffles its orders with torch's CPU generator.
Also lists the state_dict of the class built from configs/scannet/semseg-pt-v3m1-1-ppt-extreme.py.
usage: python tests/golden/make_golden_ppt.py"""
import importlib
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

SIZES = [310, 190, 240]
CONDITIONS = ("A", "B", "C")
CLASS_NAMES = ("n0", "n1", "n2", "n3", "n4", "n5", "n6", "n7", "n8")
VALID = ((0, 1, 2, 3, 4), (0, 1, 2, 3, 5, 6, 8), (1, 4, 7))
WIDTH, CHANNELS = 40, 16
EVAL_CONDITIONS, TRAIN_CONDITION = ("B", "C"), "B"
SEED, DATA_SEED = 3, 71
PART_BYTES = 900 * 1024
BN_TAP, LN_TAP = "backbone.embedding.stem.norm", "backbone.enc.enc0.block0.norm1.0"
RUNS = ("v1m1", "v1m1_adaptive", "v1m2")


def tiny_backbone(adaptive):
    return dict(type="PT-v3m1", in_channels=4, order=("z", "z-trans"), stride=(2, 2), enc_depths=(1, 1, 1),
                enc_channels=(16, 16, 32), enc_num_head=(1, 1, 2), enc_patch_size=(16, 16, 16), dec_depths=(1, 1),
                dec_channels=(16, 16), dec_num_head=(1, 1), dec_patch_size=(16, 16), drop_path=0.0, enable_flash=False,
                pdnorm_bn=True, pdnorm_ln=True, pdnorm_adaptive=adaptive, pdnorm_conditions=CONDITIONS)


def tiny_kw(run):
    kw = dict(backbone=tiny_backbone(run == "v1m1_adaptive"), backbone_out_channels=CHANNELS, conditions=CONDITIONS,
              criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)])
    if run == "v1m2":
        kw["num_classes"] = tuple(len(v) for v in VALID)
    else:
        kw.update(class_name=CLASS_NAMES, valid_index=VALID, clip_model="stub")
    return kw


def load_golden(golden_dir, run):
    """{name: array} of ppt_tiny_{run}.npz and exactly the `grad_parts` backbone-gradient files it names"""
    out = {}
    with np.load(os.path.join(golden_dir, f"ppt_tiny_{run}.npz")) as g:
        out.update({k: g[k] for k in g.files})
    want = [f"ppt_tiny_{run}_grads{i}.npz" for i in range(int(out.pop("grad_parts")))]
    have = sorted(f for f in os.listdir(golden_dir) if f.startswith(f"ppt_tiny_{run}_grads"))
    assert have == want, (have, want)
    for fname in want:
        with np.load(os.path.join(golden_dir, fname)) as g:
            out.update({k: g[k] for k in g.files})
    return out


def ppt_state_dict(model, class_embedding=None, logit_scale=None):
    """Loads the seeded weights into `model` (the reference class or the library's) and returns its state_dict;
    class_embedding and logit_scale, which are not weights, are kept, or set when given."""
    from make_golden_keypoint_oacnns import seeded_state_dict
    from make_golden_keypoint_regression import perturb_bn
    own = model.state_dict()
    sd = seeded_state_dict(own)
    for k in ("class_embedding", "logit_scale"):
        if k in own:
            sd[k] = own[k].detach().clone()
    if class_embedding is not None:
        sd["class_embedding"] = torch.as_tensor(class_embedding).to(own["class_embedding"].dtype)
    if logit_scale is not None:
        sd["logit_scale"] = torch.as_tensor(logit_scale).to(own["logit_scale"].dtype).reshape(own["logit_scale"].shape)
    model.load_state_dict(sd, strict=True)
    with torch.no_grad():
        perturb_bn(model)
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def make_data(seed=DATA_SEED):
    sys.path.insert(0, os.path.join(ROOT, "pointcept-keypointdetection_amd"))
    import ptv3_scenes as S
    batch = S.make_batch(SIZES, in_channels=4, extent=51, seed=seed)
    data = {k: batch[k] for k in ("grid_coord", "feat", "offset", "coord")}
    g = torch.Generator().manual_seed(seed + 1000)
    n = sum(SIZES)
    for cond, valid in zip(CONDITIONS, VALID):
        seg = torch.randint(0, len(valid), (n,), generator=g)
        seg[torch.rand(n, generator=g) < 0.1] = -1
        data["segment_" + cond] = seg
    return data


def batch_of(data, cond, with_segment=True, cast=None):
    out = {k: v for k, v in data.items() if not k.startswith("segment_")}
    if cast is not None:
        out = {k: (v.to(cast) if v.is_floating_point() else v) for k, v in out.items()}
    if with_segment:
        out["segment"] = data["segment_" + cond]
    out["condition"] = [cond]
    return out


def _install_clip_stub(width=WIDTH):
    clip = types.ModuleType("clip")

    class Text(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.text_projection = torch.nn.Parameter(torch.zeros(8, width))
            self.logit_scale = torch.nn.Parameter(torch.tensor(math.log(100.0)))

        def encode_text(self, tokens):
            g = torch.Generator().manual_seed(2024)
            e = torch.randn(len(tokens), width, generator=g)
            return 3.0 * e          # the class normalises the rows itself (:70-72)

    clip.load = lambda name, device="cpu", download_root=None: (Text(), None)
    clip.tokenize = lambda prompts: torch.arange(len(prompts))
    sys.modules["clip"] = clip


def _tap(model, name, cap, key):
    mod = dict(model.named_modules())[name]
    return [mod.register_forward_pre_hook(lambda m, i: cap.__setitem__(key + "_in", i[0].feat.detach().clone())),
            mod.register_forward_hook(lambda m, i, o: cap.__setitem__(key + "_out", o.feat.detach().clone()))]


def _collect(model, data, cast=None):
    res = {}
    for cond in EVAL_CONDITIONS:
        cap = {}
        hooks = [model.backbone.register_forward_hook(lambda m, i, o: cap.__setitem__("feat", o.feat.detach().clone()))]
        if cond == TRAIN_CONDITION:
            hooks += _tap(model, BN_TAP, cap, "pdn_bn") + _tap(model, LN_TAP, cap, "pdn_ln")
        model.eval()
        with torch.no_grad():
            torch.manual_seed(SEED)
            out = model(batch_of(data, cond, cast=cast))
            torch.manual_seed(SEED)
            bare = model(batch_of(data, cond, with_segment=False, cast=cast))
        for h in hooks:
            h.remove()
        assert sorted(out.keys()) == ["loss", "seg_logits"] and sorted(bare.keys()) == ["seg_logits"]
        assert torch.equal(bare["seg_logits"], out["seg_logits"])
        res[f"eval_seg_logits_{cond}"], res[f"eval_loss_{cond}"] = out["seg_logits"], out["loss"]
        res[f"eval_feat_{cond}"] = cap.pop("feat")
        res.update({"eval_" + k: v for k, v in cap.items()})
    cap = {}
    hooks = _tap(model, BN_TAP, cap, "pdn_bn")
    model.train()
    model.zero_grad()
    torch.manual_seed(SEED)
    out = model(batch_of(data, TRAIN_CONDITION, cast=cast))
    assert sorted(out.keys()) == ["loss"]
    out["loss"].backward()
    for h in hooks:
        h.remove()
    res["train_loss"] = out["loss"].detach()
    res.update({"train_" + k: v for k, v in cap.items()})
    res["nograd"] = [k for k, p in model.named_parameters() if p.grad is None]
    for k, p in model.named_parameters():
        if p.grad is not None:
            res["fullgrad_" + k] = p.grad.detach().clone()
    for k, b in model.named_buffers():
        if k.endswith("running_mean") or k.endswith("running_var"):
            res["buf_" + k] = b.detach().clone()
    return res


def _one(cls, run, data):
    kw = tiny_kw(run)
    kw["backbone"] = sys.modules["addict"].Dict(kw["backbone"])
    model = cls(**kw)
    sd0 = ppt_state_dict(model)
    r32 = _collect(model, data)
    model64 = cls(**kw).double()
    model64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd0.items()}, strict=True)
    r64 = _collect(model64, data, cast=torch.float64)
    assert r32["nograd"] == r64["nograd"] and r32["nograd"]
    active = "." + str(CONDITIONS.index(TRAIN_CONDITION)) + "."
    assert all(".norm." in k and active not in k[k.index(".norm."):] for k in r32["nograd"]
               if not any(w in k for w in ("logit_scale", "seg_heads", "embedding_table"))), r32["nograd"]
    res = {"in_" + k: v.numpy() for k, v in data.items()}
    res["nograd"] = np.array(r32.pop("nograd"))
    r64.pop("nograd")
    for k in ("class_embedding", "logit_scale"):
        if k in sd0:
            res["sd_" + k] = sd0[k].numpy()
    for k, v in r32.items():
        v32 = v.detach()
        gap = np.float64((v32.double() - r64[k].detach().double()).abs().max().item())
        if k.startswith("fullgrad_"):
            name = k[len("fullgrad_"):]
            top = v32.abs().max().clamp(min=1e-30)
            res["grad_" + name] = (v32 / top).to(torch.float16).numpy()
            res["gmax_" + name] = top.numpy()
            res["gap_grad_" + name] = gap
        else:
            res[k] = v32.numpy()
            res["gap_" + k] = gap
    print(run, "train loss", float(res["train_loss"]), "eval loss", [float(res[f"eval_loss_{c}"]) for c in EVAL_CONDITIONS])
    print(" gaps:", {k: float(v) for k, v in res.items() if k.startswith("gap_") and "grad_" not in k and "buf_" not in k})
    # the backbone's float16 gradients, in parameter order, into as many files as keep each under the limit
    grads, room = [{}], PART_BYTES // 2
    for k in [k for k in res if k.startswith("grad_backbone.")]:
        if res[k].nbytes > room:
            grads.append({})
            room = PART_BYTES // 2
        grads[-1][k] = res.pop(k)
        room -= grads[-1][k].nbytes
    for old in os.listdir(HERE):
        if old.startswith(f"ppt_tiny_{run}_grads"):
            os.remove(os.path.join(HERE, old))
    res["grad_parts"] = np.int32(len(grads))
    parts = {f"ppt_tiny_{run}_grads{i}.npz": q for i, q in enumerate(grads)}
    parts[f"ppt_tiny_{run}.npz"] = res
    for name, part in parts.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        print(" ", name, os.path.getsize(path) // 1024, "KiB")
        assert os.path.getsize(path) <= PART_BYTES, path


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import ref_loader
    from make_golden_keypoint_regression import write_listing
    from make_golden_swin3d import _cfg
    ns = ref_loader.load()
    pdn = importlib.import_module("pointcept.models.point_prompt_training.prompt_driven_normalization")
    ns.v3m1.PDNorm = pdn.PDNorm             # in place of ref_loader's dummy
    _install_clip_stub()
    v1m1 = importlib.import_module("pointcept.models.point_prompt_training.point_prompt_training_v1m1_language_guided")
    v1m2 = importlib.import_module("pointcept.models.point_prompt_training.point_prompt_training_v1m2_decoupled")
    data = make_data()
    for run in RUNS:
        _one(v1m2.PointPromptTraining if run == "v1m2" else v1m1.PointPromptTraining, run, data)
    _install_clip_stub(512)                 # ViT-B/16
    cfg = _cfg("configs/scannet/semseg-pt-v3m1-1-ppt-extreme.py")
    cfg["backbone"] = sys.modules["addict"].Dict(cfg["backbone"])
    cfg.pop("type")
    write_listing(v1m1.PointPromptTraining(**cfg), "state_dict_ppt_ptv3_scannet.txt")


if __name__ == "__main__":
    main()
