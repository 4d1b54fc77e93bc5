"""CPU-side checks of Concerto pretraining: "Concerto-v1m1" registered and built from the base config with the reference's
exact state_dict, the float64 yardstick of the GPU tests (tests/concerto_ref.py) pinned to the reference's own outputs
(tests/golden/concerto_tiny*.npz, written by tests/golden/make_golden_concerto.py), and everything of the model that runs
without the GPU: the heads, the composed losses and the composed image branch on the fixture's up-cast features (the
backbone has no CPU path; its gradients are checked by tests/test_hip_concerto.py), the moving average in both model
types, the checkpoint remapping, the fallback without images and the encoder's error.

Tolerances against the fixture (the rule of test_sonata_cpu.py): four times its fp32-vs-float64 gap of the same tensor,
with a floor of one fp32 rounding at the tensor's scale; a gradient is stored as float16 of grad / max|grad|, so it is
also allowed the float16 step of its stored value.  Pooled correspondences and patch ids are compared exactly."""
import copy
import os

import numpy as np
import pytest
import torch

import concerto_ref as R
from make_golden_sonata import PAIRINGS, MOMENTUM
from make_golden_concerto import load_golden, concerto_state_dict, with_stub_encoder, StubEncoder, TINY_KW, IMG_NUM, PATCH

ULP = 2.0 ** -23
WEIGHTS = dict(mask=1 / 8, roll_mask=1 / 8, unmask=2 / 8, enc2d=4 / 8)
_G = {}


def golden(golden_dir):
    if not _G:
        _G.update(load_golden(golden_dir))
    return _G


def close(name, got, want, gap):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    floor = ULP * np.abs(want).max()
    print(f"{name}: err {err.max():.3e} gap {gap:.3e} floor {floor:.3e}")
    assert (err <= max(4 * gap, floor)).all(), (name, err.max(), gap)


def grad_close(g, name, got):
    stored = g["grad_" + name].astype(np.float64) * float(g["gmax_" + name])
    tol = 4 * float(g["gap_grad_" + name]) + 2.0 ** -11 * np.abs(stored) + 2.0 ** -24 * float(g["gmax_" + name])
    err = np.abs(np.asarray(got, dtype=np.float64) - stored)
    print(f"{name}: err {err.max():.3e} gap {float(g['gap_grad_' + name]):.3e}")
    assert (err <= tol).all(), (name, err.max())


def stub_class():
    from pointcept.models.concerto import Concerto
    return with_stub_encoder(Concerto)


def tiny_model(**kw):
    model = stub_class()(**dict(copy.deepcopy(TINY_KW), **kw))
    if not kw:
        concerto_state_dict(model)
    return model


def test_registered_and_exported():
    import pointcept.models as M
    from pointcept.models.concerto import Concerto
    from pointcept.models.concerto.concerto_v1m1_base import OnlineCluster
    from pointcept.models.sonata import Sonata, OnlineCluster as SonataCluster
    assert M.MODELS.get("Concerto-v1m1") is Concerto is M.Concerto
    assert Concerto.__module__ == "pointcept.models.concerto.concerto_v1m1_base"
    assert issubclass(Concerto, M.PointModel) and issubclass(Concerto, Sonata)
    # Sonata's registration and exports stay what they were
    assert M.MODELS.get("Sonata-v1m1") is Sonata is M.Sonata and M.OnlineCluster is SonataCluster
    bare = OnlineCluster(8, 16, 8, 5, enable_mlp=False)
    assert list(bare.state_dict()) == ["prototype.parametrizations.weight.original0",
                                       "prototype.parametrizations.weight.original1"]
    assert tuple(bare(torch.randn(3, 8)).shape) == (3, 5)


def test_base_config_state_dict_equals_the_listing(golden_dir):
    from pointcept.models.concerto import Concerto
    from ptv3_hip.configs import CONCERTO_BASE_CFG, CONCERTO_TINY_CFG
    keep = copy.deepcopy(CONCERTO_BASE_CFG)
    cfg = {k: v for k, v in CONCERTO_BASE_CFG.items() if k != "type"}
    model = with_stub_encoder(Concerto, channels=8, tokens=cfg["patch_h"], pixels=cfg["patch_h"])(**cfg)
    assert CONCERTO_BASE_CFG == keep
    assert {k: v for k, v in CONCERTO_TINY_CFG.items() if k != "type"} == TINY_KW
    with open(os.path.join(golden_dir, "state_dict_concerto_base.txt")) as f:
        want = [line.rstrip("\n") for line in f]
    assert [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()] == want
    assert (model.patch_h, model.patch_w, model.enc2d_upcast_level, model.up_cast_level) == (37, 37, 3, 2)
    assert tuple(model.patch_proj.weight.shape) == (1536, 1184) and model.sonata_model_type == "online"
    # online: the teacher starts as the student; nothing of the teacher, the 2D teacher head or the encoder learns
    for (k, p), q in zip(model.student.named_parameters(), model.teacher.parameters()):
        assert torch.equal(p, q) and not q.requires_grad, k
    assert not any(p.requires_grad for p in model.enc2d_model.parameters())
    assert not any(p.requires_grad for p in model.enc2d_head_teacher.parameters())
    assert torch.equal(model.enc2d_head_student.prototype.weight, model.enc2d_head_teacher.prototype.weight)
    assert not hasattr(model.enc2d_head_teacher, "mlp") and hasattr(model.enc2d_head_student, "mlp")


def test_reference_defaults_and_head_layout():
    model = tiny_model(mask_loss_weight=0, roll_mask_loss_weight=0, unmask_loss_weight=0, enc2d_loss_weight=1.0)
    assert sorted(model.student.keys()) == ["backbone", "unmask_head"] == sorted(model.teacher.keys())
    plain = tiny_model(enc2d_loss_weight=0)
    assert not hasattr(plain, "patch_proj") and not hasattr(plain, "enc2d_model")
    import inspect
    from pointcept.models.concerto import Concerto
    sig = inspect.signature(Concerto.__init__).parameters
    assert (sig["enc2d_loss_weight"].default, sig["mask_loss_weight"].default, sig["enc2d_upcast_level"].default,
            sig["sonata_model_type"].default, sig["enc2d_head_num_prototypes"].default) == (0.2, 0.2, 4, "offline", 384)
    for bad in (dict(mask_loss_weight=0, roll_mask_loss_weight=0, unmask_loss_weight=0, enc2d_loss_weight=0),
                dict(num_global_view=3), dict(sonata_model_type="frozen")):
        with pytest.raises(AssertionError):
            tiny_model(**bad)


def test_fixture_is_what_the_tests_assume(golden_dir):
    g = golden(golden_dir)
    corr = g["in_global_correspondence"]
    assert 0.25 < (corr == -1).all(-1).mean() < 0.75 and (corr[(corr != -1)] >= 0).all()
    pooled = g["pooled_corr"]
    assert ((pooled == -1).all(-1)).any() and not ((pooled == -1).any(-1) != (pooled == -1).all(-1)).any()
    assert g["patch_ids"].shape[0] >= 20 and (np.diff(g["patch_ids"]) > 0).all()
    assert g["patch_ids"].max() < sum(IMG_NUM) * PATCH * PATCH
    assert ((pooled != -1).any(-1).sum(1) > 1).any()


def test_yardstick_reproduces_reference(golden_dir):
    g = golden(golden_dir)
    model = tiny_model().double()
    corr0 = torch.from_numpy(g["in_global_correspondence"]).double()
    pooled = R.pool_corr(corr0, [(torch.from_numpy(g["pool_inverse"]), torch.from_numpy(g["pool_idx_ptr"]))])
    close("pooled", pooled.numpy(), g["pooled_corr"], float(g["gap_pooled_corr"]))
    assert np.array_equal(pooled.long().numpy(), g["pooled_corr"].astype(np.int64))
    rows, scene = model.principal_rows(torch.from_numpy(g["offset_enc2d"]))
    with torch.no_grad():
        f2d = model.ENC2D_forward(torch.from_numpy(g["in_images"]).double())
    f2d = f2d.reshape(-1, f2d.shape[-1])
    out = R.enc2d_loss(torch.from_numpy(g["enc2d_feat"]).double(), pooled, rows, scene, f2d, model.patch_proj.weight.detach(),
                       model.patch_proj.bias.detach(), torch.tensor(IMG_NUM), PATCH, PATCH)
    assert np.array_equal(out["patch_ids"].numpy(), g["patch_ids"])
    for k in ("patch_mean", "projected", "encoder_rows"):
        close(k, out[k].numpy(), g[k], float(g["gap_" + k]))
    close("enc2d_loss", out["loss"].item(), g["enc2d_loss"], float(g["gap_enc2d_loss"]))


def pairing(g, name):
    head = "unmask_head" if name == "unmask" else "mask_head"
    match = torch.from_numpy(g["match_" + name])
    offset = torch.from_numpy(g["offset_local" if name == "unmask" else "offset_mask"])
    return head, match[:, 1].contiguous(), match[:, 0].contiguous(), offset


def test_composed_path_reproduces_reference(golden_dir):
    """the library's heads, composed losses and composed image branch on the fixture's up-cast features: pooled
    correspondences and patch ids exactly, patch means, rows, the five losses and every gradient outside the backbone"""
    from pointcept.models.concerto import concerto_v1m1_base as M
    g = golden(golden_dir)
    model = tiny_model().train()
    assert not any(p.requires_grad for p in model.teacher.parameters())
    with torch.no_grad():
        teacher = model.teacher.mask_head(torch.from_numpy(g["teacher_mask_head_in"]))
    close("teacher mask_head", teacher.numpy(), g["teacher_mask_head_out"], float(g["gap_teacher_mask_head_out"]))
    terms, got = [], {}
    students = {}
    for name in PAIRINGS:
        head, idx_t, idx_s, offset = pairing(g, name)
        if head not in students:
            students[head] = model.student[head](torch.from_numpy(g[f"student_{head}_in"]))
            close(f"student {head}", students[head].detach().numpy(), g[f"student_{head}_out"],
                  float(g[f"gap_student_{head}_out"]))
        got[name] = model.distill_loss(students[head], teacher, idx_t, idx_s, offset)
        close(name + "_loss", got[name].item(), g[name + "_loss"], float(g["gap_" + name + "_loss"]))
        terms.append(got[name] * WEIGHTS[name])
    # the image branch
    corr0 = torch.from_numpy(g["in_global_correspondence"])
    inverse = torch.from_numpy(g["pool_inverse"])
    pooled = M.pool_corr_torch(corr0, inverse, g["pool_idx_ptr"].shape[0] - 1)
    assert pooled.dtype == torch.float32 and np.array_equal(pooled.numpy(), g["pooled_corr"])
    assert np.array_equal(M.pool_corr_torch(corr0.long(), inverse, pooled.shape[0]).numpy(), g["pooled_corr"])
    rows, scene = model.principal_rows(torch.from_numpy(g["offset_enc2d"]))
    with torch.no_grad():
        f2d = model.ENC2D_forward(torch.from_numpy(g["in_images"]))
    f2d = f2d.reshape(-1, f2d.shape[-1])
    assert tuple(f2d.shape) == (sum(IMG_NUM) * PATCH * PATCH, 24)
    feat = torch.from_numpy(g["enc2d_feat"]).requires_grad_(True)
    loss2d, mid = model.enc2d_loss(feat, pooled, rows, scene, f2d, torch.from_numpy(g["in_img_num"]), check=True)
    assert np.array_equal(mid["patch_ids"].numpy(), g["patch_ids"])
    close("patch_mean", mid["patch_mean"].detach().numpy(), g["patch_mean"], float(g["gap_patch_mean"]))
    close("projected", mid["projected"].detach().numpy(), g["projected"], float(g["gap_projected"]))
    close("encoder_rows", f2d[mid["patch_ids"]].numpy(), g["encoder_rows"], float(g["gap_encoder_rows"]))
    close("enc2d_loss", loss2d.item(), g["enc2d_loss"], float(g["gap_enc2d_loss"]))
    terms.append(loss2d * WEIGHTS["enc2d"])
    loss = sum(terms)
    close("loss", loss.item(), g["loss"], float(g["gap_loss"]))
    loss.backward()
    assert all(p.grad is None for p in model.teacher.parameters())
    assert all(p.grad is None for p in model.enc2d_model.parameters())
    nograd = set(g["nograd"].tolist())
    checked = 0
    for k, p in model.named_parameters():
        if k.startswith(("student.backbone.", "teacher.", "enc2d_model.")):
            continue
        if k in nograd:
            assert p.grad is None, k
            continue
        grad_close(g, k, p.grad.numpy())
        checked += 1
    assert checked == 12 and "gmax_patch_proj.weight" in g and "gmax_patch_proj.bias" in g
    # rows outside the principal views, and rows without a pair, get no gradient
    others = torch.ones(feat.shape[0], dtype=torch.bool)
    others[rows[(pooled[rows] != -1).any(-1).any(-1)]] = False
    assert others.any() and not feat.grad[others].any() and feat.grad[~others].abs().sum() > 0
    # the 2D heads take no part in the forward: no gradient, as in the reference
    assert all(k in nograd for k, _ in model.named_parameters() if k.startswith("enc2d_head_"))


def test_images_without_a_valid_correspondence(golden_dir):
    """the composed path over zero rows: the reference's mean over nothing"""
    g = golden(golden_dir)
    model = tiny_model()
    rows, scene = model.principal_rows(torch.from_numpy(g["offset_enc2d"]))
    feat = torch.from_numpy(g["enc2d_feat"])
    f2d = torch.randn(sum(IMG_NUM) * PATCH * PATCH, 24)
    loss, mid = model.enc2d_loss(feat, -torch.ones(feat.shape[0], 2, 2), rows, scene, f2d, torch.tensor(IMG_NUM))
    assert mid["patch_ids"].numel() == 0 and tuple(mid["projected"].shape) == (0, 24) and torch.isnan(loss)


@pytest.mark.parametrize("model_type", ["online", "offline"])
def test_after_step_and_load_sonata(golden_dir, tmp_path, model_type):
    """both model types average the heads and copy the 2D prototypes; only `online` averages the backbone.  The offline
    teacher comes from a Sonata checkpoint whose student backbone keys are remapped"""
    g = golden(golden_dir)
    online = tiny_model()
    kw = {}
    if model_type == "offline":
        ckpt = {"state_dict": {"module.student.backbone." + k: v + 0.25 for k, v in online.student.backbone.state_dict().items()}}
        ckpt["state_dict"]["module.student.mask_head.prototype.bias"] = torch.zeros(3)      # not a backbone key: dropped
        ckpt["state_dict"]["module.teacher.backbone.embedding.stem.linear.weight"] = torch.zeros(1)
        path = str(tmp_path / "sonata.pth")
        torch.save(ckpt, path)
        kw = dict(sonata_model_type="offline", teacher_pretrained_path=path)
    model = stub_class()(**dict(copy.deepcopy(TINY_KW), **kw))
    sd = concerto_state_dict(model)
    if model_type == "offline":
        fresh = stub_class()(**dict(copy.deepcopy(TINY_KW), **kw))
        for k, v in online.student.backbone.state_dict().items():
            assert torch.equal(fresh.teacher.backbone.state_dict()[k], v + 0.25), k
        assert not any(p.requires_grad for p in fresh.teacher.parameters())
    with torch.no_grad():
        model.enc2d_head_student.prototype.parametrizations.weight.original1.add_(0.5)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    model.momentum = MOMENTUM
    model.after_step()
    for k, p in model.teacher.named_parameters():
        if model_type == "online" or "head" in k:
            close("ema " + k, p.detach().numpy(), g["ema_teacher." + k], float(g["gap_ema_teacher." + k]))
            want = MOMENTUM * before["teacher." + k] + (1 - MOMENTUM) * before["student." + k]
            assert torch.allclose(p, want, rtol=1e-6, atol=1e-7), k
        else:
            assert torch.equal(p, before["teacher." + k]), k
        assert not p.requires_grad
    for k, p in model.enc2d_head_teacher.named_parameters():
        assert torch.equal(p, before["enc2d_head_student." + k]) and not p.requires_grad, k
    assert not torch.equal(before["enc2d_head_teacher.prototype.parametrizations.weight.original1"],
                           model.enc2d_head_teacher.prototype.parametrizations.weight.original1)
    del sd


def test_load_sonata_takes_a_plain_checkpoint(tmp_path):
    """without a module.student.backbone. key the checkpoint is loaded as it is"""
    model = tiny_model()
    plain = {k: v + 1.0 for k, v in model.student.backbone.state_dict().items()}
    path = str(tmp_path / "backbone.pth")
    torch.save(plain, path)
    target = copy.deepcopy(model.teacher.backbone)
    assert model.load_sonata(target, path) is target
    for k, v in target.state_dict().items():
        assert torch.equal(v, plain[k]) and v.device.type == "cpu", k
    torch.save({"state_dict": {"module.other." + k: v for k, v in plain.items()}}, path)
    with pytest.raises(RuntimeError, match="Missing key"):
        model.load_sonata(copy.deepcopy(model.teacher.backbone), path)


class _FakeBackbone(torch.nn.Module):
    """stands in for PT-v3m2, which has no CPU path: one Linear, no pooling"""

    def __init__(self, width):
        super().__init__()
        self.lin = torch.nn.Linear(4, width)

    def forward(self, point):
        from pointcept.models.utils.structure import Point
        from pointcept.models.utils import offset2batch
        return Point(feat=self.lin(point.feat), origin_coord=point.origin_coord, offset=point.offset,
                     batch=offset2batch(point.offset, point.feat.shape[0]))


def _fake_model(golden_dir, **kw):
    g = golden(golden_dir)
    torch.manual_seed(0)
    model = tiny_model(up_cast_level=0, enc2d_upcast_level=0, backbone_out_channels=64, **kw)
    model.student["backbone"], model.teacher["backbone"] = _FakeBackbone(64), _FakeBackbone(64)

    def match(view1_coord, view1_offset, view2_coord, view2_offset):
        n = min(view1_coord.shape[0], view2_coord.shape[0])
        rows = torch.arange(0, n, 3)
        return torch.stack([rows, (rows * 7) % view2_coord.shape[0]], dim=1)

    model.match_neighbour = match
    data = {k[3:]: torch.from_numpy(g[k]) for k in g if k.startswith("in_")}
    return model, data


def test_without_images_the_loss_falls_back(golden_dir):
    model, data = _fake_model(golden_dir)
    data["img_num"] = torch.zeros(2, dtype=torch.int64)
    model.ENC2D_forward = lambda x: pytest.fail("the encoder ran without an image")
    out = model(data)
    assert sorted(out) == ["enc2d_loss", "loss", "mask_loss", "roll_mask_loss", "unmask_loss"]
    ssl = out["mask_loss"] / 8 + out["roll_mask_loss"] / 8 + out["unmask_loss"] / 4
    assert torch.allclose(out["enc2d_loss"], ssl / 0.5, rtol=1e-6) and torch.allclose(out["loss"], ssl * 2, rtol=1e-6)
    out["loss"].backward()
    assert model.patch_proj.weight.grad is None and model.student.backbone.lin.weight.grad is not None
    # only the image loss on, no image: nothing to average, the loss is 0 (:854-867)
    only, data = _fake_model(golden_dir, mask_loss_weight=0, roll_mask_loss_weight=0, unmask_loss_weight=0)
    data["img_num"] = torch.zeros(2, dtype=torch.int64)
    assert only(data) == dict(loss=0)


def test_one_student_forward_serves_mask_and_image_loss(golden_dir):
    """with exactly one of the two mask weights zero the reference runs the student a second time; here it runs once,
    and the image branch at level 0 (no pooling in between) goes through the composed path"""
    model, data = _fake_model(golden_dir, roll_mask_loss_weight=0)
    calls = []
    model.student.backbone.register_forward_hook(lambda m, i, o: calls.append(1))
    out = model(data)
    assert len(calls) == 2 and sorted(out) == ["enc2d_loss", "loss", "mask_loss", "unmask_loss"]       # masked, local
    assert torch.isfinite(out["enc2d_loss"]) and 0 <= out["enc2d_loss"].item() <= 20
    out["loss"].backward()
    assert model.patch_proj.weight.grad.abs().sum() > 0


def test_failing_encoder_names_its_cause(tmp_path):
    from pointcept.models.concerto import Concerto
    kw = dict(copy.deepcopy(TINY_KW), image_weight_name="dinov2_vitg14_reg")
    with pytest.raises(FileNotFoundError, match="image_weight_path 'facebook/dinov2-with-registers-giant'.*dinov2_vitg14_reg"):
        Concerto(**dict(kw, image_weight_path="facebook/dinov2-with-registers-giant"))
    empty = tmp_path / "weights"
    empty.mkdir()
    with pytest.raises(RuntimeError, match="could not load the image encoder 'dinov2_vitg14_reg'"):
        Concerto(**dict(kw, image_weight_path=str(empty)))


class _Siglip(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.vision_model = _Tokens()


class _Tokens(StubEncoder):
    def forward(self, x):
        import types
        return types.SimpleNamespace(last_hidden_state=super().forward(x).last_hidden_state[:, 1:])


class _Radio(StubEncoder):
    def forward(self, x):
        return None, super().forward(x).last_hidden_state[:, 1:].reshape(-1, 24)


def test_encoder_output_conventions():
    model = tiny_model()
    x = torch.rand(3, 3, 12, 12)
    assert tuple(model.ENC2D_forward(x).shape) == (3, 36, 24)          # the last patch_h * patch_w tokens
    model.enc2d_model = _Siglip()
    assert tuple(model.ENC2D_forward(x).shape) == (3, 36, 24)          # vision_model's tokens as they are
    model.image_weight_name, model.enc2d_model = "c-radio_v3", _Radio()
    assert tuple(model.ENC2D_forward(x).shape) == (3, 36, 24)          # (summary, features), reshaped


def test_wiring_follows_the_measurement():
    from pointcept.models.concerto.concerto_v1m1_base import wired
    with pytest.raises(KeyError):
        wired("nothing", 1184, 1000)
    # measured at 480 000 level-0 points with 4 views, 120 000 rows of C = 1184 / 1664, D = 1536 with 21 074 patches:
    # those shapes and more rows are listed, nothing smaller and no other width
    assert wired("pool_corr", 4, 480000) and wired("pool_corr", 4, 1000000)
    assert not wired("pool_corr", 4, 479999) and not wired("pool_corr", 3, 480000) and not wired("pool_corr", 6, 480000)
    assert wired("patch_mean", 1184, 120000) and wired("patch_mean", 1664, 120000) and wired("patch_mean", 1400, 500000)
    assert not wired("patch_mean", 80, 120000) and not wired("patch_mean", 1665, 120000)
    assert not wired("patch_mean", 1184, 119999)
    assert wired("cos", 1536, 21074) and wired("cos", 1536, 100000)
    assert not wired("cos", 384, 21074) and not wired("cos", 1536, 20999) and not wired("cos", 24, 79)
