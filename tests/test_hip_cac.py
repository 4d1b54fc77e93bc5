"""GPU tests of the context-aware classifier: the three kernels of csrc/cac.hip against tests/cac_ref.py in float64, and
the model "CAC-v1m1" against the reference's fixture (tests/golden/cac_tiny.npz).

Kernel tolerances follow the project's rule (DESIGN.md sections 13 - 15): the kernel's largest error against the float64
yardstick may be at most four times that of the SAME formula (cac_ref) evaluated by torch in float32 on the device, with a
floor of 8 float32 ulps of the tensor's largest entry.  Model tolerances are four times the fixture's stored
fp32-vs-float64 gap of the same tensor, with the rule's floor of one fp32 rounding at the tensor's scale (2^-23 of its
largest entry: the reference's pre_self_loss of 15.88 happens to lie 1.0e-7 from its float64 value, a ninth of the
spacing of fp32 numbers there, so four times that gap is below what fp32 can hold); a gradient, stored as float16 of
grad / max|grad|, is also allowed the float16 step of its stored value.  Where a confidence threshold is used, every row's largest softmax value is checked in float64
on the CPU to lie at least 1e-3 away from it, so that the mask is the same under any fp32 evaluation."""
import functools

import numpy as np
import pytest
import torch

import cac_ref as R
from make_golden_cac import load_golden, cac_state_dict, TINY_KW, TEMP, LOSSES, SIZES

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
KC = [(2, 48), (13, 96), (20, 96), (200, 48), (200, 96)]
SCENES = [1, 63, 64, 65, 700]
BIG = [2500, 2600]             # two chunks of 2048 rows per scene
DEV = "cuda:0"


def check(name, got, ref64, ref32):
    ref64 = ref64.detach().cpu().double()
    err_k = (got.detach().cpu().double() - ref64).abs().max().item()
    err_t = (ref32.detach().cpu().double() - ref64).abs().max().item()
    top = ref64.abs().max().item()
    bound = max(4.0 * err_t, 8.0 * ULP * top)
    print(f"{name}: kernel {err_k:.3e} torch-fp32 {err_t:.3e} max|ref| {top:.3e} bound {bound:.3e}")
    assert err_k <= bound, (name, err_k, err_t, top)


@functools.lru_cache(maxsize=None)
def inputs(k, c, sizes, conf):
    """x, logits (scene 2 without a confident row when conf > 0), labels, offset, dproto - float64 on the CPU"""
    g = torch.Generator().manual_seed(1000 * k + c + len(sizes))
    n = sum(sizes)
    x = torch.randn(n, c, generator=g, dtype=torch.float64)
    logits = torch.randn(n, k, generator=g, dtype=torch.float64) * 3.0
    offset = torch.tensor(np.cumsum(sizes))
    if conf > 0 and len(sizes) > 2:
        logits[offset[1]:offset[2]] *= 0.01
    if conf > 0:
        for _ in range(20):
            top = torch.softmax(logits.float().double(), 1).max(1)[0]
            near = (top - conf).abs() < 2e-3
            if not near.any():
                break
            logits[near] *= 1.5
        top = torch.softmax(logits.float().double(), 1).max(1)[0]
        assert ((top - conf).abs() >= 1e-3).all()
        if len(sizes) > 2:
            assert not (top[offset[1]:offset[2]] >= conf).any() and (top >= conf).any()
    labels = torch.randint(-1, k - 1, (n,), generator=g)           # class k - 1 absent, -1 ignored
    if k > 2:
        labels[labels == 0] = 1
        labels[n // 2] = 0                                           # a class of one point
    dproto = torch.randn(len(sizes), k, c, generator=g, dtype=torch.float64)
    return x.float().double(), logits.float().double(), labels, offset, dproto.float().double()


@functools.lru_cache(maxsize=None)
def proto_softmax_refs(k, c, sizes, conf):
    x, logits, _, offset, dproto = inputs(k, c, sizes, conf)
    out = []
    for dt, dev in ((torch.float64, "cpu"), (torch.float32, DEV)):
        xx = x.to(dev, dt).detach().clone().requires_grad_(True)
        proto, den = R.proto_softmax(xx, logits.to(dev, dt), offset, conf)
        (proto * dproto.to(dev, dt)).sum().backward()
        out.append((proto.detach(), den.detach(), xx.grad))
    return out


@pytest.mark.parametrize("conf", [0.0, 0.75])
@pytest.mark.parametrize("k,c", KC)
def test_proto_softmax(k, c, conf):
    from ptv3_hip import ops
    assert ops.cac_capable(k, c)
    sizes = tuple(SCENES)
    x, logits, _, offset, dproto = inputs(k, c, sizes, conf)
    (p64, d64, g64), (p32, d32, g32) = proto_softmax_refs(k, c, sizes, conf)
    xd, ld, od = x.float().to(DEV), logits.float().to(DEV), offset.to(DEV)
    proto, den, count = ops.cac_proto(xd, logits=ld, offset=od, conf_thresh=conf)
    assert count is None and tuple(proto.shape) == (len(sizes), k, c) and tuple(den.shape) == (len(sizes), k)
    check("proto", proto, p64, p32)
    check("den", den, d64, d32)
    if conf > 0:
        assert torch.equal(proto[2], torch.zeros_like(proto[2])) and not torch.isnan(proto).any()
    dx = ops.cac_proto_bwd(dproto.float().to(DEV), den, (x.shape[0], c), logits=ld, offset=od, conf_thresh=conf)
    check("dx", dx, g64, g32)
    again, den2, _ = ops.cac_proto(xd, logits=ld, offset=od, conf_thresh=conf)
    dx2 = ops.cac_proto_bwd(dproto.float().to(DEV), den2, (x.shape[0], c), logits=ld, offset=od, conf_thresh=conf)
    assert torch.equal(again, proto) and torch.equal(den2, den) and torch.equal(dx2, dx)


@pytest.mark.parametrize("k,c", [(13, 96), (200, 96)])
def test_proto_softmax_several_chunks_per_scene(k, c):
    from ptv3_hip import ops
    sizes = tuple(BIG)
    x, logits, _, offset, dproto = inputs(k, c, sizes, 0.75)
    (p64, d64, g64), (p32, d32, g32) = proto_softmax_refs(k, c, sizes, 0.75)
    xd, ld, od = x.float().to(DEV), logits.float().to(DEV), offset.to(DEV)
    proto, den, _ = ops.cac_proto(xd, logits=ld, offset=od, conf_thresh=0.75)
    check("proto", proto, p64, p32)
    check("den", den, d64, d32)
    dx = ops.cac_proto_bwd(dproto.float().to(DEV), den, (x.shape[0], c), logits=ld, offset=od, conf_thresh=0.75)
    check("dx", dx, g64, g32)
    again, _, _ = ops.cac_proto(xd, logits=ld, offset=od, conf_thresh=0.75)
    assert torch.equal(again, proto)


@pytest.mark.parametrize("sizes", [tuple(SCENES), tuple(BIG)])
@pytest.mark.parametrize("k,c", KC)
def test_proto_label(k, c, sizes):
    from ptv3_hip import ops
    x, _, labels, _, dproto = inputs(k, c, sizes, 0.0)
    refs = []
    for dt, dev in ((torch.float64, "cpu"), (torch.float32, DEV)):
        xx = x.to(dev, dt).detach().clone().requires_grad_(True)
        proto, cnt = R.proto_label(xx, labels.to(dev), k)
        (proto * dproto[0].to(dev, dt)).sum().backward()
        refs.append((proto.detach(), cnt, xx.grad))
    xd, lab = x.float().to(DEV), labels.to(DEV)
    proto, den, count = ops.cac_proto(xd, labels=lab, num_classes=k)
    assert tuple(proto.shape) == (k, c) and count.dtype == torch.int32
    assert torch.equal(count.cpu().long(), refs[0][1].long()) and torch.equal(den.cpu().double(), refs[0][1])
    assert count[k - 1] == 0 and torch.equal(proto[k - 1], torch.zeros_like(proto[k - 1]))
    if k > 2:
        assert count[0] == 1
    check("proto", proto, refs[0][0], refs[1][0])
    dx = ops.cac_proto_bwd(dproto[0].float().to(DEV).contiguous(), den, (x.shape[0], c), labels=lab)
    check("dx", dx, refs[0][2], refs[1][2])
    assert torch.equal(dx[labels == -1], torch.zeros_like(dx[labels == -1]))
    again, _, count2 = ops.cac_proto(xd, labels=lab, num_classes=k)
    assert torch.equal(again, proto) and torch.equal(count2, count)


def test_proto_label_all_ignored():
    from ptv3_hip import ops
    x = torch.randn(300, 48, device=DEV)
    labels = torch.full((300,), -1, dtype=torch.int64, device=DEV)
    proto, den, count = ops.cac_proto(x, labels=labels, num_classes=20)
    assert not proto.any() and not den.any() and not count.any()
    dx = ops.cac_proto_bwd(torch.randn(20, 48, device=DEV), den, (300, 48), labels=labels)
    assert not dx.any()


def test_autograd_functions_tape_the_kernels():
    from ptv3_hip import autograd as A
    k, c, sizes = 13, 96, tuple(SCENES)
    x, logits, labels, offset, dproto = inputs(k, c, sizes, 0.75)
    (p64, _, g64), (p32, _, g32) = proto_softmax_refs(k, c, sizes, 0.75)
    xd = x.float().to(DEV).requires_grad_(True)
    proto, den = A.cac_proto_softmax(xd, logits.float().to(DEV), offset.to(DEV), 0.75)
    (proto * dproto.float().to(DEV)).sum().backward()
    check("proto", proto, p64, p32)
    check("dx", xd.grad, g64, g32)
    xd.grad = None
    proto, den, count = A.cac_proto_label(xd, labels.to(DEV), k)
    proto.sum().backward()
    assert xd.grad is not None and not count.requires_grad and not den.requires_grad


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("k,c", KC)
def test_cos_logits(k, c, shared):
    from ptv3_hip import ops
    sizes = tuple(SCENES)
    y, _, _, offset, q = inputs(k, c, sizes, 0.0)
    q = q.clone()
    q[:, k // 2] = 0                                  # a zero prototype row: logits 0, not NaN
    if shared:
        q = q[0]
    r64 = R.cos_logits(y, q, offset, float(TEMP))
    r32 = R.cos_logits(y.float().to(DEV), q.float().to(DEV), offset, float(TEMP))
    out = ops.cac_cos_logits(y.float().to(DEV), q.float().to(DEV).contiguous(), None if shared else offset.to(DEV), TEMP)
    assert tuple(out.shape) == (y.shape[0], k) and not torch.isnan(out).any()
    assert torch.equal(out[:, k // 2], torch.zeros_like(out[:, k // 2]))
    check("cos_logits", out, r64, r32)
    assert torch.equal(ops.cac_cos_logits(y.float().to(DEV), q.float().to(DEV).contiguous(),
                                          None if shared else offset.to(DEV), TEMP), out)


@pytest.mark.parametrize("sizes", [tuple(SCENES), tuple(BIG)])
@pytest.mark.parametrize("k", [2, 13, 20, 200])
def test_distill(k, sizes):
    from ptv3_hip import ops
    _, pred, labels, _, _ = inputs(k, 48, sizes, 0.0)
    soft = inputs(k, 96, sizes, 0.0)[1]
    refs = []
    for dt, dev in ((torch.float64, "cpu"), (torch.float32, DEV)):
        pp = pred.to(dev, dt).detach().clone().requires_grad_(True)
        loss = R.distill_loss(pp, soft.to(dev, dt), labels.to(dev))
        (loss * 1.7).backward()
        refs.append((loss.detach().reshape(1), pp.grad))
    pd, sd, lab = pred.float().to(DEV), soft.float().to(DEV), labels.to(DEV)
    out, coef, count = ops.cac_distill(pd, sd, lab)
    valid = labels[labels >= 0]
    assert torch.equal(count[:k].cpu().long(), torch.bincount(valid, minlength=k))
    assert int(count[k]) == int((torch.bincount(valid, minlength=k) > 0).sum())
    check("loss", out, refs[0][0], refs[1][0])
    dpred = ops.cac_distill_bwd(torch.tensor([1.7], device=DEV), pd, sd, lab, coef)
    check("dpred", dpred, refs[0][1], refs[1][1])
    assert torch.equal(dpred[labels == -1], torch.zeros_like(dpred[labels == -1]))
    out2, coef2, _ = ops.cac_distill(pd, sd, lab)
    assert torch.equal(out2, out) and torch.equal(coef2, coef)
    assert torch.equal(ops.cac_distill_bwd(torch.tensor([1.7], device=DEV), pd, sd, lab, coef), dpred)


def test_distill_no_valid_label():
    from ptv3_hip import autograd as A
    pred = torch.randn(700, 20, device=DEV, requires_grad=True)
    soft = torch.randn(700, 20, device=DEV)
    loss = A.cac_distill(pred, soft, torch.full((700,), -1, dtype=torch.int64, device=DEV))
    loss.backward()
    assert loss.item() == 0.0 and not pred.grad.any()


def test_outside_the_limits_is_refused():
    from ptv3_hip import ops
    assert not ops.cac_capable(1, 48) and not ops.cac_capable(257, 48) and not ops.cac_capable(20, 129)
    assert not ops.cac_capable(256, 128)
    for k, c in [(20, 48), (100, 48), (200, 48), (20, 96), (100, 96), (200, 96)]:
        assert ops.cac_capable(k, c)
    with pytest.raises(RuntimeError, match="outside the limits"):
        ops.cac_proto(torch.randn(10, 129, device=DEV), labels=torch.zeros(10, dtype=torch.int64, device=DEV),
                      num_classes=20)


# ---- the model against the reference's fixture ------------------------------------------------------------------
_G = {}


def golden(golden_dir):
    if not _G:
        _G.update(load_golden(golden_dir))
    return _G


def _model(fused):
    from pointcept.models import build_model
    model = build_model(dict(type="CAC-v1m1", **TINY_KW))
    cac_state_dict(model)
    return model.to(DEV).set_fused(fused)


def _data(g, with_segment=True):
    keys = ["grid_coord", "feat", "offset", "coord"] + (["segment"] if with_segment else [])
    return {k: torch.from_numpy(g["in_" + k]).to(DEV) for k in keys}


def _close(name, got, want, gap, extra=0.0):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    floor = ULP * np.abs(want).max()             # one fp32 rounding at the tensor's scale: a stored gap can be less
    print(f"{name}: err {err.max():.3e} gap {gap:.3e} floor {floor:.3e}")
    assert (err <= np.maximum(4 * gap, floor) + extra).all(), (name, err.max(), gap)


@pytest.mark.parametrize("fused", [True, False])
def test_model_eval_matches_reference(golden_dir, fused):
    g = golden(golden_dir)
    model = _model(fused).eval()
    with torch.no_grad():
        out = model(_data(g))
        bare = model(_data(g, with_segment=False))
    assert sorted(out) == ["loss", "seg_logits"] and sorted(bare) == ["seg_logits"]
    assert torch.equal(bare["seg_logits"], out["seg_logits"])
    _close("seg_logits", out["seg_logits"].cpu().numpy(), g["eval_seg_logits"], float(g["gap_eval_seg_logits"]))
    _close("loss", out["loss"].item(), g["eval_loss"], float(g["gap_eval_loss"]))


@functools.lru_cache(maxsize=None)
def _train_step(fused):
    g = _G
    model = _model(fused).train()
    out = model(_data(g))
    out["loss"].backward()
    torch.cuda.synchronize()
    losses = {k: out[k].item() for k in out}
    grads = {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}
    bufs = {k: b.detach().cpu().numpy() for k, b in model.named_buffers() if k.startswith("feat_proj_layer.")}
    return losses, grads, bufs


def _grad_bound(g, name):
    stored = g["grad_" + name].astype(np.float64) * float(g["gmax_" + name])
    return stored, 2.0 ** -11 * np.abs(stored) + 2.0 ** -24 * float(g["gmax_" + name])


@pytest.mark.parametrize("fused", [True, False])
def test_model_training_step_matches_reference(golden_dir, fused):
    g = golden(golden_dir)
    losses, grads, bufs = _train_step(fused)
    assert sorted(losses) == sorted(LOSSES)
    for k in LOSSES:
        _close(k, losses[k], g["train_" + k], float(g["gap_train_" + k]))
    assert int(bufs["feat_proj_layer.1.num_batches_tracked"]) == len(SIZES) + 1
    for k in ("running_mean", "running_var"):
        name = "feat_proj_layer.1." + k
        _close(name, bufs[name], g["buf_" + name], float(g["gap_buf_" + name]))
    assert len(grads) == sum(1 for k in g if k.startswith("gmax_"))
    for name, got in grads.items():
        stored, step = _grad_bound(g, name)
        _close("grad " + name, got, stored, float(g["gap_grad_" + name]), step)


def test_model_fused_and_composed_agree(golden_dir):
    g = golden(golden_dir)
    (l1, g1, b1), (l0, g0, b0) = _train_step(True), _train_step(False)
    for k in LOSSES:
        _close(k, l1[k], l0[k], float(g["gap_train_" + k]))
    for name in g1:
        _close("grad " + name, g1[name], g0[name], float(g["gap_grad_" + name]))
    for name in b1:
        if name.endswith("num_batches_tracked"):
            assert b1[name] == b0[name]
        else:
            _close(name, b1[name], b0[name], float(g["gap_buf_" + name]))


def test_model_hook_or_undetached_logits_take_the_composed_path(golden_dir):
    g = golden(golden_dir)
    model = _model(True).eval()
    feat = torch.randn(8, 16, device=DEV)
    assert model._use_kernels(feat)
    handle = model.proj[0].register_forward_hook(lambda m, i, o: None)
    assert not model._use_kernels(feat)
    handle.remove()
    model.detach_pre_logits = False
    assert not model._use_kernels(feat)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_model_under_autocast_runs_the_head_in_fp32(golden_dir, dtype):
    """the configs train with enable_amp=True: inside torch.autocast one eval forward and one training step of the
    fused model give fp32 results, those of the run without autocast within the model tolerances (the head switches
    autocast off and the tiny SpUNet backbone has no op that autocast touches); the head alone, on given features, is
    bitwise the fp32 head, also when the features arrive in the autocast dtype"""
    g = golden(golden_dir)
    model = _model(True).eval()
    with torch.no_grad():
        want = model(_data(g))
        with torch.autocast("cuda", dtype=dtype):
            got = model(_data(g))
            feat = model.backbone(_data(g))
            feat = getattr(feat, "feat", feat)
            half = model.head(feat.to(dtype), _data(g))
        half_want = model.head(feat.to(dtype).float(), _data(g))
    assert got["seg_logits"].dtype == torch.float32 and got["loss"].dtype == torch.float32
    _close("autocast eval seg_logits", got["seg_logits"].cpu().numpy(), want["seg_logits"].cpu().numpy(),
           float(g["gap_eval_seg_logits"]))
    _close("autocast eval loss", got["loss"].item(), want["loss"].item(), float(g["gap_eval_loss"]))
    assert half["seg_logits"].dtype == torch.float32 and torch.equal(half["seg_logits"], half_want["seg_logits"])

    losses, grads, bufs = _train_step(True)
    model = _model(True).train()
    with torch.autocast("cuda", dtype=dtype):
        out = model(_data(g))
    assert all(out[k].dtype == torch.float32 for k in LOSSES)
    out["loss"].backward()
    torch.cuda.synchronize()
    for k in LOSSES:
        _close("autocast " + k, out[k].item(), losses[k], float(g["gap_train_" + k]))
    for name, p in model.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32
        _close("autocast grad " + name, p.grad.cpu().numpy(), grads[name], float(g["gap_grad_" + name]))
    for name, b in model.named_buffers():
        if name.startswith("feat_proj_layer.") and not name.endswith("num_batches_tracked"):
            _close("autocast " + name, b.cpu().numpy(), bufs[name], float(g["gap_buf_" + name]))
    assert int(model.feat_proj_layer[1].num_batches_tracked) == len(SIZES) + 1

