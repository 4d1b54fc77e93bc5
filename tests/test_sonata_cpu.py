"""CPU-side checks of Sonata pretraining: "Sonata-v1m1" registered and built from both config dicts with the reference's
exact state_dict, the float64 yardstick of the GPU tests (tests/sonata_ref.py) pinned to the reference's own outputs
(tests/golden/sonata_tiny*.npz, written by tests/golden/make_golden_sonata.py), and everything of the model that runs
without the GPU: the heads and the composed losses on the fixture's up-cast features (the backbone has no CPU path; its
gradients are checked by tests/test_hip_sonata.py), the moving average, the schedules, the hook, the two-rank reduction and
the empty-scene rule.

Tolerances against the fixture (the rule of test_cac_cpu.py / test_ppt_cpu.py): four times its fp32-vs-float64 gap of the
same tensor, with a floor of one fp32 rounding at the tensor's scale; a gradient is stored as float16 of grad / max|grad|,
so it is also allowed the float16 step of its stored value."""
import copy
import os
import types

import numpy as np
import pytest
import torch

import sonata_ref as R
from make_golden_sonata import (load_golden, sonata_state_dict, TINY_KW, PAIRINGS, SCHEDULES, STEPS, TOTAL_STEPS,
                                MOMENTUM)

ULP = 2.0 ** -23
T, TAU = 0.04, 0.1
WEIGHTS = dict(mask=2 / 8, roll_mask=2 / 8, unmask=4 / 8)
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


def pairing(g, name, dtype=torch.float64):
    """(teacher logits, teacher rows, student logits, student rows, student offsets) of one of the three losses"""
    head = "unmask_head" if name == "unmask" else "mask_head"
    match = torch.from_numpy(g["match_" + name])
    offset = torch.from_numpy(g["in_local_offset" if name == "unmask" else "in_global_offset"])
    return (torch.from_numpy(g[f"teacher_{head}_out"]).to(dtype), match[:, 1].contiguous(),
            torch.from_numpy(g[f"student_{head}_out"]).to(dtype), match[:, 0].contiguous(), offset)


def tiny_model():
    from pointcept.models import build_model
    model = build_model(dict(type="Sonata-v1m1", **copy.deepcopy(TINY_KW)))
    sonata_state_dict(model)
    return model


def test_registered_and_exported():
    import pointcept.models as M
    from pointcept.models.sonata import Sonata, OnlineCluster
    assert M.MODELS.get("Sonata-v1m1") is Sonata is M.Sonata and M.OnlineCluster is OnlineCluster
    assert issubclass(Sonata, M.PointModel)


def test_base_config_state_dict_equals_the_listing(golden_dir):
    from pointcept.models import build_model
    from ptv3_hip.configs import SONATA_BASE_CFG
    keep = copy.deepcopy(SONATA_BASE_CFG)
    model = build_model(SONATA_BASE_CFG)
    assert SONATA_BASE_CFG == keep
    with open(os.path.join(golden_dir, "state_dict_sonata_base.txt")) as f:
        want = [line.rstrip("\n") for line in f]
    assert [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()] == want
    assert (model.momentum_base, model.match_max_r, model.mask_jitter, model.num_local_view) == (0.994, 0.32, 0.01, 4)
    # the teacher starts as the student, frozen, without the student's drop path
    for (k, p), q in zip(model.student.named_parameters(), model.teacher.parameters()):
        assert torch.equal(p, q) and not q.requires_grad, k
    frozen = [k for k, p in model.student.named_parameters() if not p.requires_grad]
    assert frozen == ["mask_head.prototype.parametrizations.weight.original0",
                      "unmask_head.prototype.parametrizations.weight.original0"]
    assert all((p == 1).all() for k, p in model.named_parameters() if k.endswith("original0"))
    drops = lambda net: [m.drop_prob for m in net.modules() if type(m).__name__ == "DropPath"]  # noqa: E731
    assert max(drops(model.student.backbone)) > 0.29 and not drops(model.teacher.backbone)


def test_tiny_config_and_reference_defaults():
    from pointcept.models import build_model
    from ptv3_hip.configs import SONATA_TINY_CFG
    model = build_model(SONATA_TINY_CFG)
    assert {k: v for k, v in SONATA_TINY_CFG.items() if k != "type"} == TINY_KW
    assert tuple(model.student.mask_head.prototype.weight.shape) == (100, 16)
    assert (model.mask_loss_weight, model.roll_mask_loss_weight, model.unmask_loss_weight, model.student_temp,
            model.teacher_temp, model.momentum, model.match_max_k, model.mask_size_base) == (0.25, 0.25, 0.5, 0.1, 0.04,
                                                                                             0.996, 8, 0.4)
    only = build_model(dict(type="Sonata-v1m1", **dict(TINY_KW, mask_loss_weight=0, roll_mask_loss_weight=0)))
    assert sorted(only.student.keys()) == ["backbone", "unmask_head"] == sorted(only.teacher.keys())
    for bad in (dict(mask_loss_weight=0, roll_mask_loss_weight=0, unmask_loss_weight=0), dict(num_global_view=1),
                dict(num_global_view=3)):
        with pytest.raises(AssertionError):
            build_model(dict(type="Sonata-v1m1", **dict(TINY_KW, **bad)))


def test_fixture_is_what_the_tests_assume(golden_dir):
    g = golden(golden_dir)
    assert sorted(np.sort(g["patch_index"]).tolist()) == list(range(g["patch_index"].shape[0]))
    for name in PAIRINGS:
        _, idx_t, _, idx_s, offset = pairing(g, name)
        assert (idx_s[1:] > idx_s[:-1]).all()
        assert torch.bincount(R.scene_of(idx_s, offset), minlength=offset.shape[0]).min() >= 4
    assert all(k.startswith("teacher.") or k.endswith("original0") for k in g["nograd"].tolist())
    for head in ("mask_head", "unmask_head"):
        assert np.abs(g[f"teacher_{head}_out"]).max() <= 1 + 1e-5 and np.abs(g[f"student_{head}_out"]).max() <= 1 + 1e-5


@pytest.mark.parametrize("name", PAIRINGS)
def test_yardstick_reproduces_reference(golden_dir, name):
    g = golden(golden_dir)
    x, idx_t, s, idx_s, offset = pairing(g, name)
    loss, target, _ = R.loss(x, idx_t, s, idx_s, offset, T, TAU)
    close("target", target.numpy(), g["target_" + name], float(g["gap_target_" + name]))
    close("loss", loss.item(), g[name + "_loss"], float(g["gap_" + name + "_loss"]))
    assert torch.allclose(target.sum(1), torch.ones(target.shape[0], dtype=torch.float64), atol=1e-12)


def test_scaling_form_is_the_literal_iteration():
    """softmax(x / T + log u_3) with u_3 from the three sweeps IS sinkhorn_knopp (float64, repeated rows, |x| = 1), for
    the yardstick's sweeps and for the model's composed functions"""
    from pointcept.models.sonata import sonata_v1m1_base as M
    gen = torch.Generator().manual_seed(0)
    for n, k, temp in ((301, 100, 0.04), (777, 130, 0.07), (64, 2, 0.04)):
        unit = lambda rows: torch.nn.functional.normalize(torch.randn(rows, 16, generator=gen, dtype=torch.float64), dim=1)  # noqa: E731
        x = unit(n // 2) @ unit(k).t()
        x[0, 0] = 1.0
        idx = torch.randint(0, n // 2, (n,), generator=gen)
        want = R.sinkhorn_knopp(x[idx], temp)
        steps, d = R.sweeps(x, idx, temp)
        got = torch.softmax(x[idx] / temp + torch.log(steps[-1][1]), 1)
        assert (got - want).abs().max() < 1e-13
        e = torch.exp(x[idx] / temp)
        assert torch.allclose((e * steps[-1][1]).sum(1), d, rtol=1e-12, atol=0)
        u = M.sinkhorn_scaling_torch(e)
        assert torch.allclose(u, steps[-1][1], rtol=1e-12, atol=0)
        s = unit(n + 9) @ unit(k).t()
        idx_s = torch.randperm(n + 9, generator=gen)[:n].sort()[0]
        offset = torch.tensor([n // 3, n // 2, n + 9])
        lit, _, per_pair = R.loss(x, idx, s, idx_s, offset, temp, 0.1)
        mine, target = M.pair_losses_torch(s, x, idx, idx_s, temp, 0.1)
        assert (target - want).abs().max() < 1e-13 and torch.allclose(mine, per_pair, rtol=1e-11, atol=1e-12)
        sv = s.clone().requires_grad_(True)
        M.sonata_loss_torch(sv, x, idx, idx_s, offset, temp, 0.1).backward()
        assert abs(M.sonata_loss_torch(s, x, idx, idx_s, offset, temp, 0.1).item() - lit.item()) < 1e-11
        assert (sv.grad - R.dstudent(x, idx, s, idx_s, offset, temp, 0.1)).abs().max() < 1e-12


def test_composed_heads_and_losses_reproduce_reference(golden_dir):
    """the library's heads and composed losses on the fixture's up-cast features: losses, head gradients, no gradient
    on the teacher, and the teacher after one after_step at momentum 0.9"""
    g = golden(golden_dir)
    model = tiny_model().train()
    assert not any(p.requires_grad for p in model.teacher.parameters())
    feats = {k: torch.from_numpy(g[k]) for k in g if k.endswith("_head_in")}
    terms, got = [], {}
    for name in PAIRINGS:
        head = "unmask_head" if name == "unmask" else "mask_head"
        with torch.no_grad():
            teacher = model.teacher[head](feats[f"teacher_{head}_in"])
        student = model.student[head](feats[f"student_{head}_in"])
        close(f"teacher {head}", teacher.numpy(), g[f"teacher_{head}_out"], float(g[f"gap_teacher_{head}_out"]))
        close(f"student {head}", student.detach().numpy(), g[f"student_{head}_out"], float(g[f"gap_student_{head}_out"]))
        _, idx_t, _, idx_s, offset = pairing(g, name)
        got[name] = model.distill_loss(student, teacher, idx_t, idx_s, offset)
        close(name + "_loss", got[name].item(), g[name + "_loss"], float(g["gap_" + name + "_loss"]))
        terms.append(got[name] * WEIGHTS[name])
    loss = sum(terms)
    close("loss", loss.item(), g["loss"], float(g["gap_loss"]))
    loss.backward()
    assert all(p.grad is None for p in model.teacher.parameters())
    checked = 0
    for k, p in model.student.named_parameters():
        if k.startswith("backbone."):
            continue
        if "student." + k in g["nograd"].tolist():
            assert p.grad is None and k.endswith("original0")
            continue
        grad_close(g, "student." + k, p.grad.numpy())
        checked += 1
    assert checked == 10
    model.momentum = MOMENTUM
    before = {k: p.detach().clone() for k, p in model.teacher.named_parameters()}
    model.after_step()
    for k, p in model.teacher.named_parameters():
        close("ema " + k, p.detach().numpy(), g["ema_" + k], float(g["gap_ema_" + k]))
        assert not p.requires_grad
        if not k.endswith("original0"):
            assert not torch.equal(p, before[k]), k


def _trainer(total=TOTAL_STEPS):
    return types.SimpleNamespace(cfg=types.SimpleNamespace(scheduler=types.SimpleNamespace(total_steps=total)),
                                 start_epoch=0, train_loader=[0] * 10, writer=None)


def test_schedules_and_model_hook(golden_dir):
    from pointcept.engines.hooks.builder import HOOKS
    from pointcept.engines.hooks import HookBase, ModelHook
    from pointcept.utils.scheduler import CosineScheduler
    g = golden(golden_dir)
    model = tiny_model()
    hook = HOOKS.build(dict(type="ModelHook"))
    assert isinstance(hook, ModelHook) and isinstance(model, HookBase)
    hook.trainer = _trainer()
    hook.trainer.model = model
    hook.before_train()
    assert model.trainer is hook.trainer and model.momentum_scheduler.total_iters == TOTAL_STEPS
    rows = []
    for step in range(TOTAL_STEPS):
        hook.before_step()
        if step in STEPS:
            rows.append([float(getattr(model, name)) for name in SCHEDULES])
    assert np.allclose(np.asarray(rows), g["schedules"], rtol=1e-12, atol=0)
    hook.after_step(), hook.before_epoch(), hook.after_epoch(), hook.after_train()
    # a model that is no HookBase gets an inert stand-in
    plain = HOOKS.build(dict(type="ModelHook"))
    plain.trainer = _trainer()
    plain.trainer.model = torch.nn.Linear(2, 2)
    plain.before_train(), plain.before_step(), plain.after_step()
    # the schedule itself: warm-up ends on the base value, the cosine ends next to the final one, then stays there
    s = CosineScheduler(base_value=1.0, final_value=0.0, total_iters=10, start_value=0.5, warmup_iters=3)
    vals = [s.step() for _ in range(12)]
    assert vals[0] == 0.5 and vals[2] == 1.0 and vals[3] == 1.0 and 0 < vals[9] < 0.1 and vals[10] == vals[11] == 0.0
    assert s.iter == 12 and s[4] == vals[4]


def test_two_rank_reduction_equals_one_rank(golden_dir):
    """the composed sweeps with a fake all_reduce that adds the other rank's partial sums (rows split 60 / 40) give the
    targets of the single-rank run on all rows"""
    from pointcept.models.sonata import sonata_v1m1_base as M
    g = golden(golden_dir)
    x, idx_t, s, idx_s, _ = pairing(g, "mask", torch.float32)
    m = idx_t.shape[0]
    cut = int(0.6 * m)
    whole, target = M.pair_losses_torch(s, x, idx_t, idx_s, T, TAU)
    parts = []
    for mine, other in ((slice(0, cut), slice(cut, m)), (slice(cut, m), slice(0, cut))):
        e_other = torch.exp(x[idx_t[other]] / T)
        state = {"u": None}

        def all_reduce(a, e_other=e_other, state=state):
            a += M.sk_sweep_torch(e_other, state["u"], m)
            state["u"] = 1.0 / (a.shape[0] * a)

        parts.append(M.pair_losses_torch(s, x, idx_t[mine], idx_s[mine], T, TAU, n_total=m, all_reduce=all_reduce))
    got_loss, got_target = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    gap = float(g["gap_target_mask"])
    close("target", got_target.numpy(), target.numpy(), gap)
    close("target vs reference", got_target.numpy(), g["target_mask"], gap)
    close("pair loss", got_loss.numpy(), whole.numpy(), float(g["gap_mask_loss"]))


def test_empty_scene_rule():
    """a middle scene without a pair counts with mean 0, trailing ones do not count; no pair at all is loss 0"""
    from pointcept.models.sonata import sonata_v1m1_base as M
    values = torch.tensor([1.0, 3.0, 10.0], dtype=torch.float64)
    offset = torch.tensor([4, 8, 12, 16])
    rows = torch.tensor([0, 2, 9])                     # scenes 0, 0, 2: scene 1 empty, scene 3 trailing
    scene = R.scene_of(rows, offset)
    assert scene.tolist() == [0, 0, 2]
    assert M.scene_mean_torch(values, scene, 4).item() == pytest.approx((2.0 + 0.0 + 10.0) / 3)
    means, count = R.scene_mean(values, scene)
    assert means.tolist() == [2.0, 0.0, 10.0] and count.tolist() == [2.0, 0.0, 1.0]
    assert M.scene_mean_torch(values[:2], scene[:2], 4).item() == pytest.approx(2.0)      # scenes 1 - 3 trailing
    gen = torch.Generator().manual_seed(3)
    x, s = torch.rand(5, 7, generator=gen, dtype=torch.float64), torch.rand(16, 7, generator=gen, dtype=torch.float64)
    idx_t = torch.tensor([4, 4, 1])
    got = M.sonata_loss_torch(s, x, idx_t, rows, offset, T, TAU)
    want, _, per_pair = R.loss(x, idx_t, s, rows, offset, T, TAU)
    assert got.item() == pytest.approx(want.item(), rel=1e-12)
    assert want.item() == pytest.approx(((per_pair[0] + per_pair[1]) / 2 + per_pair[2]).item() / 3, rel=1e-12)
    sv = s.clone().requires_grad_(True)
    zero = M.sonata_loss_torch(sv, x, idx_t[:0], rows[:0], offset, T, TAU)
    zero.backward()
    assert zero.item() == 0.0 and not sv.grad.any()


def test_wiring_follows_the_measurement():
    from pointcept.models.sonata.sonata_v1m1_base import wired
    with pytest.raises(KeyError):
        wired("nothing", 4096, 1000)
    # ahead at K = 3072 and 4096 from 20 000 pairs on; at K = 2048 only at 100 000 (a tie at 20 000); behind at 1088
    assert wired("loss", 4096, 100000) and wired("loss", 4096, 20000) and wired("loss", 3072, 20000)
    assert wired("loss", 3500, 20000) and wired("loss", 2048, 100000) and wired("loss", 2500, 150000)
    assert not wired("loss", 2048, 20000) and not wired("loss", 3071, 99999) and not wired("loss", 2047, 100000)
    assert not wired("loss", 1088, 100000) and not wired("loss", 1024, 100000) and not wired("loss", 4097, 100000)
    assert not wired("loss", 4096, 19999)
