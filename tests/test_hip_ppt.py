"""GPU tests of Point Prompt Training: the collapsed-head kernel of csrc/ppt_head.hip against tests/ppt_ref.py in float64,
PDNorm inside PT-v3m1 against a plain PT-v3m1 that carries the active condition's norms, and the models "PPT-v1m1" /
"PPT-v1m2" against the reference's fixtures (tests/golden/ppt_tiny_*.npz).

Kernel tolerance (the rule of test_hip_cac.py, DESIGN.md sections 13 - 15): the kernel's largest error against the float64
yardstick may be at most four times that of the reference formula (ppt_ref.head, the reference's statement order)
evaluated by torch in float32 on the device over the same rows, with a floor of 8 float32 ulps of the largest entry.
Model tolerances are four times the fixture's stored fp32-vs-float64 gap of the same tensor, with a floor of one fp32
rounding at the tensor's scale; a gradient, stored as float16 of grad / max|grad|, is also allowed the float16 step of its
stored value."""
import functools
import re

import numpy as np
import pytest
import torch

import ppt_ref as R
from make_golden_ppt import (load_golden, ppt_state_dict, tiny_kw, tiny_backbone, batch_of, CONDITIONS, VALID,
                             EVAL_CONDITIONS, TRAIN_CONDITION, WIDTH, SEED)

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
DEV = "cuda:0"
KC = [(1, 16), (13, 64), (20, 64), (25, 96), (36, 128), (49, 48), (200, 48)]
ROWS = [1, 15, 16, 17, 63, 64, 65, 129, 700]      # 129: one row into a second workgroup of 128
LOG_SCALE = float(np.log(100.0))


def check(name, got, ref64, ref32):
    ref64 = ref64.detach().cpu().double()
    err_k = (got.detach().cpu().double() - ref64).abs().max().item()
    err_t = (ref32.detach().cpu().double() - ref64).abs().max().item()
    top = ref64.abs().max().item()
    bound = max(4.0 * err_t, 8.0 * ULP * top)
    print(f"{name}: kernel {err_k:.3e} torch-fp32 {err_t:.3e} ratio {err_k / max(err_t, 1e-300):.2f} "
          f"max|ref| {top:.3e} bound {bound:.3e}")
    return err_k <= bound, (name, err_k, err_t, top)


@functools.lru_cache(maxsize=None)
def head_inputs(k, c, d, cond, bias):
    """fp32-representable W (D, C) with the given condition number, b, unit-row E (36 + k names, D), the K valid names,
    x (700, C) with every fourth row along the four weakest singular directions of W - as float64 on the CPU"""
    g = torch.Generator().manual_seed(10000 * k + 100 * c + d + int(cond) + int(bias))
    m = min(d, c)
    u, _ = torch.linalg.qr(torch.randn(d, m, generator=g, dtype=torch.float64))
    v, _ = torch.linalg.qr(torch.randn(c, m, generator=g, dtype=torch.float64))
    W = (u * torch.logspace(0, -np.log10(cond), m, dtype=torch.float64)) @ v.t()
    b = torch.randn(d, generator=g, dtype=torch.float64) * 0.05 if bias else None
    E = torch.randn(k + 7, d, generator=g, dtype=torch.float64)
    E = E / E.norm(dim=1, keepdim=True)
    valid = tuple(torch.randperm(k + 7, generator=g)[:k].tolist())
    x = torch.randn(max(ROWS), c, generator=g, dtype=torch.float64)
    x[3::4] = torch.randn(x[3::4].shape[0], 4, generator=g, dtype=torch.float64) @ v[:, -4:].t()
    f = lambda t: None if t is None else t.float().double()   # noqa: E731
    return f(W), f(b), f(E), valid, f(x)


@pytest.mark.parametrize("d", [40, 512])
@pytest.mark.parametrize("k,c", KC)
def test_head_kernel_against_float64(k, c, d):
    from ptv3_hip import ops
    assert ops.ppt_head_capable(c, k)
    failed = []
    for cond in (2.0, 100.0):
        for bias in (False, True):
            W, b, E, valid, x = head_inputs(k, c, d, cond, bias)
            ref64 = R.head(x, W, b, E, valid, LOG_SCALE)
            ref32 = R.head(x.float().to(DEV), W.float().to(DEV), None if b is None else b.float().to(DEV),
                           E.float().to(DEV), valid, LOG_SCALE)
            B, bb, beta, s = ops.ppt_head_collapse(W.float().to(DEV), None if b is None else b.float().to(DEV),
                                                   E[list(valid)].float().to(DEV), torch.tensor(LOG_SCALE))
            assert B.is_cuda and tuple(B.shape) == (c, c + k)
            xd = x.float().to(DEV)
            for n in ROWS:
                out = ops.ppt_head(xd[:n].contiguous(), B, bb, beta, s)
                assert tuple(out.shape) == (n, k) and out.dtype == torch.float32
                ok, what = check(f"K={k} C={c} D={d} cond={cond:g} bias={bias} n={n}", out, ref64[:n], ref32[:n])
                if not ok:
                    failed.append(what)
                assert torch.equal(ops.ppt_head(xd[:n].contiguous(), B, bb, beta, s), out)     # bitwise repeatable
    assert not failed, failed


def test_head_kernel_with_column_tiles_read_from_global_memory():
    """C = 128 with 256 classes: B exceeds the LDS budget, the last column tiles take their fragments from global memory"""
    from ptv3_hip import ops
    k, c, d = 256, 128, 512
    W, b, E, valid, x = head_inputs(k, c, d, 2.0, True)
    ref64 = R.head(x, W, b, E, valid, LOG_SCALE)
    ref32 = R.head(x.float().to(DEV), W.float().to(DEV), b.float().to(DEV), E.float().to(DEV), valid, LOG_SCALE)
    B, bb, beta, s = ops.ppt_head_collapse(W.float().to(DEV), b.float().to(DEV), E[list(valid)].float().to(DEV),
                                           torch.tensor(LOG_SCALE))
    for n in (129, 700):
        out = ops.ppt_head(x.float().to(DEV)[:n].contiguous(), B, bb, beta, s)
        ok, what = check(f"K={k} C={c} n={n}", out, ref64[:n], ref32[:n])
        assert ok, what


def test_zero_projection_gives_the_reference_nan():
    from ptv3_hip import ops
    W, b, E, valid, x = head_inputs(13, 64, 512, 2.0, False)
    B, bb, beta, s = ops.ppt_head_collapse(W.float().to(DEV), None, E[list(valid)].float().to(DEV), torch.tensor(LOG_SCALE))
    xd = x.float().to(DEV)[:17].contiguous()
    xd[5] = 0
    out = ops.ppt_head(xd, B, bb, beta, s)
    assert torch.isnan(out[5]).all() and not torch.isnan(out[:5]).any() and not torch.isnan(out[6:]).any()


def test_outside_the_limits_is_refused():
    from ptv3_hip import ops
    from ptv3_hip.lib import lib
    assert not ops.ppt_head_capable(20, 13) and not ops.ppt_head_capable(64, 0) and not ops.ppt_head_capable(64, 257)
    assert not ops.ppt_head_capable(144, 13) and ops.ppt_head_capable(128, 256) and ops.ppt_head_capable(16, 1)
    for c, k in [(20, 13), (64, 0), (64, 257)]:
        x = torch.randn(10, c, device=DEV)
        with pytest.raises(RuntimeError, match="outside the limits"):
            ops.ppt_head(x, torch.zeros(c, c + k, device=DEV), torch.zeros(c + k, device=DEV), 0.0, 1.0)
        assert b"outside the limits" in lib.load().ptv3_last_error()


# ---- PDNorm inside PT-v3m1 ------------------------------------------------------------------------------------------
_PDN_KEY = re.compile(r"\.norm\.(\d)\.(weight|bias|running_mean|running_var|num_batches_tracked)$")


def _plain_state_dict(sd, index):
    """state_dict of a PDNorm PT-v3m1 -> that of the plain PT-v3m1 that carries the norms of condition `index`"""
    out = {}
    for k, v in sd.items():
        m = _PDN_KEY.search(k)
        if m is None:
            out[k] = v.clone()
        elif int(m.group(1)) == index:
            out[k[: m.start()] + "." + m.group(2)] = v.clone()
    return out


def _backbones(index):
    from pointcept.models import build_model
    from make_golden_keypoint_oacnns import seeded_state_dict
    cfg = tiny_backbone(False)
    pd = build_model(cfg)
    pd.load_state_dict(seeded_state_dict(pd.state_dict()), strict=True)
    plain = build_model({k: v for k, v in cfg.items() if not k.startswith("pdnorm")})
    plain.load_state_dict(_plain_state_dict(pd.state_dict(), index), strict=True)
    plain.use_engine = False
    return pd.to(DEV), plain.to(DEV)


def _scene(cond):
    from make_golden_ppt import make_data
    data = batch_of(make_data(), cond)
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in data.items()}


@pytest.mark.parametrize("cond", ["A", "C"])
def test_pdnorm_backbone_equals_the_plain_backbone_with_the_active_norms(cond):
    index = CONDITIONS.index(cond)
    pd, plain = _backbones(index)
    pd.eval(), plain.eval()
    from ptv3_hip import engine
    assert not engine.eligible(pd)
    with torch.no_grad():
        torch.manual_seed(SEED)
        a = pd(_scene(cond)).feat
        torch.manual_seed(SEED)
        b = plain(_scene(cond)).feat
        torch.manual_seed(SEED)
        other = pd(_scene("B")).feat
    assert torch.equal(a, b)
    assert not torch.equal(a, other)


def test_pdnorm_training_step_moves_only_the_active_condition():
    from ptv3_hip.optim import FusedAdamW
    cond = "C"
    index = CONDITIONS.index(cond)
    pd, plain = _backbones(index)
    pd.train(), plain.train()
    before = {k: v.detach().clone() for k, v in pd.state_dict().items()}
    outs = []
    for model in (pd, plain):
        torch.manual_seed(SEED)
        feat = model(_scene(cond)).feat
        (feat * torch.linspace(-1, 1, feat.shape[1], device=DEV)).sum().backward()
        outs.append(feat.detach())
    assert torch.equal(outs[0], outs[1])
    plain_grads = {k: p.grad for k, p in plain.named_parameters()}
    mapped = _plain_state_dict({k: p.grad for k, p in pd.named_parameters() if p.grad is not None}, index)
    assert set(mapped) == set(plain_grads)
    for k, gr in plain_grads.items():
        assert torch.equal(mapped[k], gr), k
    for k, p in pd.named_parameters():
        m = _PDN_KEY.search(k)
        assert (p.grad is None) == (m is not None and int(m.group(1)) != index), k
    after = pd.state_dict()
    plain_after = plain.state_dict()
    moved = 0
    for k, v in after.items():
        m = _PDN_KEY.search(k)
        if m is None or not m.group(2).startswith(("running", "num")):
            continue
        if int(m.group(1)) == index:
            assert torch.equal(v, plain_after[k[: m.start()] + "." + m.group(2)]), k
            moved += int(not torch.equal(v, before[k]))
        else:
            assert torch.equal(v, before[k]), k
    assert moved > 0
    # a fused AdamW step leaves the inactive conditions' parameters bitwise unchanged and moves the active ones
    opt = FusedAdamW(pd.parameters(), lr=1e-2, weight_decay=0.05)
    opt.step()
    torch.cuda.synchronize()
    for k, p in pd.named_parameters():
        m = _PDN_KEY.search(k)
        if m is not None and int(m.group(1)) != index:
            assert torch.equal(p.detach(), before[k]), k
        elif m is not None:
            assert not torch.equal(p.detach(), before[k]), k


def test_pdnorm_without_affine_parameters_runs_composed():
    from pointcept.models import build_model
    from make_golden_keypoint_oacnns import seeded_state_dict
    model = build_model(dict(tiny_backbone(False), pdnorm_affine=False))
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    model = model.to(DEV).eval()
    with torch.no_grad():
        torch.manual_seed(SEED)
        feat = model(_scene("B")).feat
    assert torch.isfinite(feat).all()


# ---- the models against the reference's fixtures --------------------------------------------------------------------
_G = {}


def golden(golden_dir, run):
    if run not in _G:
        _G[run] = load_golden(golden_dir, run)
    return _G[run]


def _model(g, run, fused=True):
    from pointcept.models import build_model
    from pointcept.models.point_prompt_training import point_prompt_training_v1m1_language_guided as V
    V.CLIP_TEXT_WIDTH.setdefault("stub", WIDTH)          # the fixture's text encoder: width 40
    model = build_model(dict(type="PPT-v1m2" if run == "v1m2" else "PPT-v1m1", **tiny_kw(run)))
    ppt_state_dict(model, g.get("sd_class_embedding"), g.get("sd_logit_scale"))
    return model.to(DEV).set_fused(fused)


def _data(g, cond, with_segment=True):
    data = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("in_")}
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batch_of(data, cond, with_segment).items()}


def _close(name, got, want, gap, extra=0.0):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    floor = ULP * np.abs(want).max()
    print(f"{name}: err {err.max():.3e} gap {gap:.3e} floor {floor:.3e}")
    assert (err <= np.maximum(4 * gap, floor) + extra).all(), (name, err.max(), gap)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("run", ["v1m1", "v1m1_adaptive", "v1m2"])
def test_model_eval_matches_reference(golden_dir, run, fused):
    g = golden(golden_dir, run)
    model = _model(g, run, fused).eval()
    for cond in EVAL_CONDITIONS:
        with torch.no_grad():
            torch.manual_seed(SEED)
            out = model(_data(g, cond))
            torch.manual_seed(SEED)
            bare = model(_data(g, cond, with_segment=False))
        assert sorted(out) == ["loss", "seg_logits"] and sorted(bare) == ["seg_logits"]
        assert torch.equal(bare["seg_logits"], out["seg_logits"])
        assert tuple(out["seg_logits"].shape)[1] == len(VALID[CONDITIONS.index(cond)])
        _close(f"seg_logits {cond}", out["seg_logits"].cpu().numpy(), g[f"eval_seg_logits_{cond}"],
               float(g[f"gap_eval_seg_logits_{cond}"]))
        _close(f"loss {cond}", out["loss"].item(), g[f"eval_loss_{cond}"], float(g[f"gap_eval_loss_{cond}"]))


@pytest.mark.parametrize("run", ["v1m1", "v1m1_adaptive", "v1m2"])
def test_model_training_step_matches_reference(golden_dir, run):
    g = golden(golden_dir, run)
    model = _model(g, run).train()
    torch.manual_seed(SEED)
    out = model(_data(g, TRAIN_CONDITION))
    assert sorted(out) == ["loss"]
    out["loss"].backward()
    torch.cuda.synchronize()
    _close("loss", out["loss"].item(), g["train_loss"], float(g["gap_train_loss"]))
    nograd = set(g["nograd"].tolist())
    for name, p in model.named_parameters():
        assert (p.grad is None) == (name in nograd), name
        if p.grad is None:
            continue
        gmax = float(g["gmax_" + name])
        stored = g["grad_" + name].astype(np.float64) * gmax
        step = 2.0 ** -11 * np.abs(stored) + 2.0 ** -24 * gmax
        _close("grad " + name, p.grad.cpu().numpy(), stored, float(g["gap_grad_" + name]), step)
    for name, b in model.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            _close(name, b.cpu().numpy(), g["buf_" + name], float(g["gap_buf_" + name]))


def test_model_cache_follows_an_in_place_update_of_the_weights(golden_dir):
    g = golden(golden_dir, "v1m1")
    model = _model(g, "v1m1").eval()
    cond = EVAL_CONDITIONS[0]
    index = CONDITIONS.index(cond)
    feat = torch.from_numpy(g[f"eval_feat_{cond}"]).to(DEV)
    gap = float(g[f"gap_eval_seg_logits_{cond}"])
    with torch.no_grad():
        first = model.head(feat, index)
        assert model.collapsed(index) is model.collapsed(index)          # cached: same objects, nothing recomputed
        model.proj_head.weight.mul_(0.5).add_(0.01)
        second = model.head(feat, index)
        composed = model.set_fused(False).head(feat, index)
    assert not torch.equal(first, second)
    _close("after the update", second.cpu().numpy(), composed.cpu().numpy(), gap)


def test_model_kernel_form_matches_the_compositions(golden_dir, monkeypatch):
    """whatever `wired` selects at this size, all three forms of the eval head give the fixture's logits"""
    from pointcept.models.point_prompt_training import point_prompt_training_v1m1_language_guided as V
    g = golden(golden_dir, "v1m1")
    model = _model(g, "v1m1").eval()
    for cond in EVAL_CONDITIONS:
        index = CONDITIONS.index(cond)
        feat = torch.from_numpy(g[f"eval_feat_{cond}"]).to(DEV)
        for form in ("kernel", "collapsed", "reference"):
            monkeypatch.setattr(V, "wired", lambda k, c, n, form=form: form)
            with torch.no_grad():
                out = model.head(feat, index)
            _close(f"{form} {cond}", out.cpu().numpy(), g[f"eval_seg_logits_{cond}"],
                   float(g[f"gap_eval_seg_logits_{cond}"]) + float(g[f"gap_eval_feat_{cond}"]))
    handle = model.proj_head.register_forward_hook(lambda m, i, o: None)
    monkeypatch.setattr(V, "wired", lambda k, c, n: pytest.fail("a hooked proj_head composes the reference order"))
    with torch.no_grad():
        model.head(feat, index)
    handle.remove()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_model_under_autocast_runs_the_head_in_fp32(golden_dir, dtype):
    """inside torch.autocast the backbone computes in bfloat16, so there only dtypes and the head are pinned: the results
    are fp32, and the head alone on given features is bitwise the fp32 head, also when the features arrive in half
    precision; with the backbone held at fp32 the model under autocast is held to the fixture"""
    g = golden(golden_dir, "v1m1")
    model = _model(g, "v1m1").eval()
    cond = EVAL_CONDITIONS[0]
    index = CONDITIONS.index(cond)
    feat = torch.from_numpy(g[f"eval_feat_{cond}"]).to(DEV)
    with torch.no_grad():
        with torch.autocast("cuda", dtype=dtype):
            torch.manual_seed(SEED)
            got = model(_data(g, cond))
            half = model.head(feat.to(dtype), index)
        want = model.head(feat.to(dtype).float(), index)
    assert got["seg_logits"].dtype == torch.float32 and got["loss"].dtype == torch.float32
    assert torch.isfinite(got["seg_logits"]).all()
    assert half.dtype == torch.float32 and torch.equal(half, want)
    # with the backbone held at fp32 (its derived weights folded once outside autocast) the whole model under autocast
    # meets the fixture's tolerances
    model.backbone.compute_dtype = torch.float32
    with torch.no_grad():
        torch.manual_seed(SEED)
        model(_data(g, cond))
        with torch.autocast("cuda", dtype=dtype):
            torch.manual_seed(SEED)
            got = model(_data(g, cond))
    assert got["seg_logits"].dtype == torch.float32
    _close("autocast seg_logits", got["seg_logits"].cpu().numpy(), g[f"eval_seg_logits_{cond}"],
           float(g[f"gap_eval_seg_logits_{cond}"]))
    _close("autocast loss", got["loss"].item(), g[f"eval_loss_{cond}"], float(g[f"gap_eval_loss_{cond}"]))
    model.backbone.compute_dtype = None
    model.train()
    with torch.autocast("cuda", dtype=dtype):
        torch.manual_seed(SEED)
        out = model(_data(g, TRAIN_CONDITION))
    assert out["loss"].dtype == torch.float32
    out["loss"].backward()
    assert all(p.grad is None or p.grad.dtype == torch.float32 for p in model.parameters())
