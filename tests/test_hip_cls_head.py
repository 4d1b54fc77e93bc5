"""The batch head kernels of csrc/cls_head.hip through ptv3_hip.ops, against the float64 restatement tests/cls_head_ref.py
(pinned to the reference by test_body_regressor_cpu.py).

Tolerance rule: a tensor's largest error against float64 may be at most 4 x the largest error of
the SAME function composed from torch float32 ops on the device, with a floor of 8 float32 ulps (8 * 2^-23) of the
tensor's largest entry.  The inputs keep every batch variance away from 0 (rows on separated levels, weight rows of
mostly one sign, every fourth unit of the opposite one), so that the composition is well-conditioned and the comparison is
not one of amplified noise.

Two kinds of gradient are exactly zero in exact arithmetic, and only they are treated differently: the two biases in
front of a BatchNorm at any b (the batch mean removes any shift), and, at b = 2, every gradient in front of a BatchNorm
(dg and the gradients of modules 0, 1, 4: the normalised rows are +-1 whatever the input).  There "the tensor's largest
entry" is a float64 rounding residue (about 1e-13 of the other gradients) and both sides hold only the rounding left
over by the BatchNorm backward, which subtracts from the arriving gradient its projections on the constant and on the
normalised column: noise of a few ulps of the terms that cancel, which are of the size of the gradients behind the
BatchNorm.  For these tensors alone the floor is 8 ulps of the largest entry of any gradient of the step; every other
tensor, at every b, has the floor of the rule, 8 ulps of its own largest entry."""
import numpy as np
import pytest
import torch

import cls_head_ref as R

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
TILE = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def test_row_tile_constant():
    from ptv3_hip import ops
    assert ops.CLS_HEAD_ROW_TILE == TILE


def _check(name, got, ref64, torch32, floor_scale=None):
    """the rule of the module docstring; prints each figure before it asserts"""
    ref64 = ref64.double().cpu()
    err_k = (got.double().cpu() - ref64).abs().max().item()
    err_t = (torch32.double().cpu() - ref64).abs().max().item()
    top = ref64.abs().max().item() if floor_scale is None else floor_scale
    bound = max(4.0 * err_t, 8.0 * ULP * top)
    print(f"{name}: kernel {err_k:.3e} torch-fp32 {err_t:.3e} max|ref| {top:.3e} bound {bound:.3e}")
    assert err_k <= bound, (name, err_k, err_t, top)


def _head_params(c, h1, h2, out, seed, dev):
    """fp32 state_dict of the head on `dev`: mostly positive weights (see the module docstring)"""
    g = torch.Generator().manual_seed(seed)

    def w(o, k):
        # a mostly positive row per unit, so that the unit separates the rows' levels; every fourth unit has the opposite
        # sign, so that the ReLU does not silence the same rows in every column (rows that are zero everywhere would be
        # near-equal rows - a small batch variance - in the next layer); a fourth and not a half, because two rows that
        # are active on equally many units give near-equal sums in the next layer at b = 2
        sign = (1.0 - 2.0 * (torch.arange(o) % 4 == 3).float()).view(o, 1)
        return sign * ((0.8 * torch.rand(o, k, generator=g) + 0.2 * torch.randn(o, k, generator=g)) * (2.0 / k ** 0.5))

    sd = {"0.weight": w(h1, c), "0.bias": 0.1 * torch.randn(h1, generator=g),
          "1.weight": 0.5 + torch.rand(h1, generator=g), "1.bias": 0.2 * torch.randn(h1, generator=g),
          "1.running_mean": 0.1 * torch.randn(h1, generator=g), "1.running_var": 0.5 + torch.rand(h1, generator=g),
          "4.weight": w(h2, h1), "4.bias": 0.1 * torch.randn(h2, generator=g),
          "5.weight": 0.5 + torch.rand(h2, generator=g), "5.bias": 0.2 * torch.randn(h2, generator=g),
          "5.running_mean": 0.1 * torch.randn(h2, generator=g), "5.running_var": 0.5 + torch.rand(h2, generator=g),
          "8.weight": w(out, h2) - 0.5 / h2 ** 0.5, "8.bias": 0.1 * torch.randn(out, generator=g)}
    return {k: v.to(dev).contiguous() for k, v in sd.items()}


def _scene_sizes(b):
    """an empty scene and a one-row scene wherever b allows, about 3000 rows in all"""
    if b == 1:
        return [3000]
    if b == 2:
        return [1, 2999]
    rest = b - 2
    sizes = [3000 // rest + 7 * i for i in range(rest)]
    return sizes[:1] + [0, 1] + sizes[1:]


def _fold(sd, i, eps=1e-5):
    s = sd[f"{i}.weight"] * torch.rsqrt(sd[f"{i}.running_var"] + eps)
    return s.contiguous(), (sd[f"{i}.bias"] - sd[f"{i}.running_mean"] * s).contiguous()


def _eval_call(ops, x, off, sd, target):
    (s1, t1), (s2, t2) = _fold(sd, 1), _fold(sd, 5)
    return ops.cls_head_eval(x, off, sd["0.weight"].t().contiguous(), sd["0.bias"], s1, t1,
                             sd["4.weight"].t().contiguous(), sd["4.bias"], s2, t2, sd["8.weight"].t().contiguous(),
                             sd["8.bias"], target, 0.7, 100.0)


def _pool(x, sizes, dtype):
    x = x.to(dtype)
    rows = [seg.mean(0) if seg.shape[0] else x.new_zeros(x.shape[1]) for seg in torch.split(x, sizes)]
    return torch.stack(rows)


EVAL_SHAPES = [(1, 8, 8, 8, 1), (2, 16, 24, 8, 7), (3, 64, 256, 128, 7), (5, 512, 256, 128, 40),
               (TILE + 1, 16, 40, 24, 7)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", EVAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eval_head_vs_float64(dev, shape, dtype):
    """ptv3_cls_head_eval with and without target: logits, loss and column errors against float64 on the stored-
    precision features; an empty scene pools to zeros; two runs bitwise equal; the logits do not depend on `target`."""
    from ptv3_hip import ops
    b, c, h1, h2, out = shape
    sizes = _scene_sizes(b)
    sd = _head_params(c, h1, h2, out, seed=b + c, dev=dev)
    gen = torch.Generator(device=dev).manual_seed(17 + b)
    x = (torch.randn(sum(sizes), c, device=dev, generator=gen) + 0.5).to(dtype)
    off = torch.tensor(np.cumsum(sizes), dtype=torch.int64, device=dev)
    target = torch.randn(b, out, device=dev, generator=gen)
    logits, stats = _eval_call(ops, x, off, sd, target)
    bare, none = _eval_call(ops, x, off, sd, None)
    assert none is None and torch.equal(bare, logits)
    again, stats2 = _eval_call(ops, x, off.int(), sd, target.reshape(-1))
    assert torch.equal(again, logits) and torch.equal(stats2, stats)
    sd64 = {k: v.double() for k, v in sd.items()}
    ref = R.head_eval(_pool(x, sizes, torch.float64), sd64)
    t32 = R.head_eval(_pool(x, sizes, torch.float32), sd)
    _check("logits", logits, ref, t32)
    _check("stats", stats, R.l1_stats(ref, target.double(), 0.7, 100.0), R.l1_stats(t32, target, 0.7, 100.0))


def _train_inputs(b, c, h1, h2, out, mask_kind, dev):
    sd = _head_params(c, h1, h2, out, seed=3 * b + out, dev=dev)
    gen = torch.Generator(device=dev).manual_seed(b)
    levels = torch.randperm(b, device=dev, generator=gen).float().view(b, 1) * 0.6
    g = (0.3 * torch.randn(b, c, device=dev, generator=gen) + levels).contiguous()
    if mask_kind == "half":
        keep = 0.5
        m1 = torch.empty(b, h1, device=dev).bernoulli_(keep, generator=gen)
        m2 = torch.empty(b, h2, device=dev).bernoulli_(keep, generator=gen)
    else:
        keep = 1.0 if mask_kind == "one" else 0.5
        m1, m2 = torch.ones(b, h1, device=dev), torch.ones(b, h2, device=dev)
        if mask_kind == "column":
            m1[:, h1 // 2] = 0.0
            m2[:, 0] = 0.0
    target = torch.randn(b, out, device=dev, generator=gen)
    dlogits = torch.randn(b, out, device=dev, generator=gen).contiguous()
    return sd, g, m1, m2, keep, target, dlogits


def _params(sd, momentum=0.1, eps=1e-5):
    return (sd["0.weight"], sd["0.bias"], sd["1.weight"], sd["1.bias"], sd["1.running_mean"], sd["1.running_var"],
            momentum, eps, sd["4.weight"], sd["4.bias"], sd["5.weight"], sd["5.bias"], sd["5.running_mean"],
            sd["5.running_var"], momentum, eps, sd["8.weight"], sd["8.bias"])


GRADS = ("d0.weight", "d0.bias", "d1.weight", "d1.bias", "d4.weight", "d4.bias", "d5.weight", "d5.bias", "d8.weight",
         "d8.bias")
DLOSS = 0.37


def _run_kernels(ops, sd, g, m1, m2, keep, target, dlogits, loss_weight=0.7):
    """one forward + backward through the entry points on a private copy of the running statistics"""
    sd = {k: (v.clone() if "running" in k else v) for k, v in sd.items()}
    l1 = dlogits is None
    logits, stats, save = ops.cls_head_train_fwd(g, _params(sd), m1, m2, keep, target if l1 else None, loss_weight, 100.0)
    if l1:
        dloss = torch.full((1,), DLOSS, device=g.device)
        dg, grads = ops.cls_head_train_bwd(g, _params(sd), save, keep, dloss=dloss, loss_weight=loss_weight)
    else:
        dg, grads = ops.cls_head_train_bwd(g, _params(sd), save, keep, dlogits=dlogits)
    out = {"logits": logits, "stats": stats, "dg": dg, "run": {k: v for k, v in sd.items() if "running" in k}}
    out.update(dict(zip(GRADS, grads)))
    return out


def _compare(got, ref, t32, l1, b):
    gmax = max(ref[k].abs().max().item() for k in GRADS + ("dg",))
    # exactly zero in exact arithmetic (module docstring): noise against the size of what cancels
    zero = ("d0.bias", "d4.bias")
    if b == 2:
        zero += ("dg", "d0.weight", "d1.weight", "d1.bias", "d4.weight")
    _check("logits", got["logits"], ref["logits"], t32["logits"])
    if l1:
        _check("stats", got["stats"], ref["stats"], t32["stats"])
    for k in ref["run"]:
        _check(k, got["run"][k], ref["run"][k], t32["run"][k])
    for k in ("dg",) + GRADS:
        _check(k, got[k], ref[k], t32[k], gmax if k in zero else None)


@pytest.mark.parametrize("mode", ["l1", "dlogits"])
@pytest.mark.parametrize("mask_kind", ["half", "one", "column"])
@pytest.mark.parametrize("b", [2, 3, 7, TILE + 1])
def test_train_head_vs_float64(dev, b, mask_kind, mode):
    """ptv3_cls_head_train_fwd / _bwd: every output, every gradient and both BatchNorms' running statistics, in the L1
    mode (dloss = 0.37 through a device scalar) and with dlogits given; two runs bitwise equal."""
    from ptv3_hip import ops
    c, h1, h2, out = (64, 256, 128, 7) if b != 3 else (24, 37, 19, 5)   # b = 3: odd widths, no 16-byte weight rows
    sd, g, m1, m2, keep, target, dlogits = _train_inputs(b, c, h1, h2, out, mask_kind, dev)
    l1 = mode == "l1"
    got = _run_kernels(ops, sd, g, m1, m2, keep, target, None if l1 else dlogits)
    twice = _run_kernels(ops, sd, g, m1, m2, keep, target, None if l1 else dlogits)
    for k in ("logits", "dg") + GRADS:
        assert torch.equal(got[k], twice[k]), k
    assert all(torch.equal(got["run"][k], twice["run"][k]) for k in got["run"])
    if l1:
        assert torch.equal(got["stats"], twice["stats"])
    else:
        assert got["stats"] is None
    kw = dict(target=target, loss_weight=0.7, dloss=DLOSS) if l1 else dict(dlogits=dlogits)
    ref = R.train_step(g.double(), {k: v.double() for k, v in sd.items()}, m1.double(), m2.double(), keep,
                       **{k: (v.double() if torch.is_tensor(v) else v) for k, v in kw.items()})
    t32 = R.train_step(g, sd, m1, m2, keep, **kw)
    _compare(got, ref, t32, l1, b)
    if mask_kind == "column":   # a unit dropped for every row passes no gradient to its weights
        assert torch.count_nonzero(got["d4.weight"][:, h1 // 2]).item() == 0
        assert torch.count_nonzero(got["d8.weight"][:, 0]).item() == 0


def test_sign_of_zero_difference(dev):
    """target[0, 0] := the kernel's own logit (bitwise repeatable, so the difference is exactly 0 in the second run): that
    element contributes nothing to any gradient, as torch's abs (sign(0) = 0); the references get the same treatment
    with their own logit."""
    from ptv3_hip import ops
    b, c, h1, h2, out = 4, 64, 256, 128, 7
    sd, g, m1, m2, keep, target, _ = _train_inputs(b, c, h1, h2, out, "half", dev)
    first = _run_kernels(ops, sd, g, m1, m2, keep, target, None)
    target = target.clone()
    target[0, 0] = first["logits"][0, 0]
    got = _run_kernels(ops, sd, g, m1, m2, keep, target, None)
    assert got["logits"][0, 0].item() == target[0, 0].item()
    # d8.bias[0] = coef * sum over rows of sign(logit - target): row 0 counts 0
    coef = np.float32(np.float32(DLOSS) * np.float32(0.7)) / (np.float32(b) * np.float32(out))
    want = np.float32(0.0)
    for s in torch.sign(got["logits"][:, 0] - target[:, 0]).cpu().numpy():
        want = np.float32(want + np.float32(coef * np.float32(s)))
    assert abs(got["d8.bias"][0].item() - float(want)) <= 2 * ULP * abs(float(want)) + 1e-12
    assert torch.sign(got["logits"][:, 0] - target[:, 0])[0].item() == 0.0

    def ref_run(g_, sd_, m1_, m2_, t_):
        probe = R.head_train(g_, sd_, m1_, m2_, keep)[0]
        t_ = t_.clone()
        t_[0, 0] = probe[0, 0]
        return R.train_step(g_, sd_, m1_, m2_, keep, target=t_, loss_weight=0.7, dloss=DLOSS)

    ref = ref_run(g.double(), {k: v.double() for k, v in sd.items()}, m1.double(), m2.double(), target.double())
    t32 = ref_run(g, sd, m1, m2, target)
    _compare(got, ref, t32, True, b)


def test_out_of_limit_shapes_are_refused(dev):
    """outside the limits every entry point returns an error with a message and launches nothing"""
    from ptv3_hip import ops
    assert ops.cls_head_capable(64, 256, 128, 7) and ops.cls_head_capable(512, 256, 128, 40)
    assert ops.cls_head_capable(1024, 512, 511, 512)
    for bad in ((12, 8, 8, 1), (1032, 8, 8, 1), (8, 513, 8, 1), (8, 8, 513, 1), (8, 8, 8, 513), (8, 8, 8, 0)):
        assert not ops.cls_head_capable(*bad), bad
    c, h1, h2, out = 8, 513, 8, 1
    sd = _head_params(c, h1, h2, out, seed=0, dev=dev)
    x = torch.randn(10, c, device=dev)
    off = torch.tensor([4, 10], device=dev)
    with pytest.raises(RuntimeError, match="unsupported"):
        _eval_call(ops, x, off, sd, None)
    g = torch.randn(2, c, device=dev)
    m1, m2 = torch.ones(2, h1, device=dev), torch.ones(2, h2, device=dev)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.cls_head_train_fwd(g, _params(sd), m1, m2, 1.0)
    ok = _head_params(8, 8, 8, 1, seed=0, dev=dev)
    with pytest.raises(RuntimeError, match="at least 2 rows"):
        ops.cls_head_train_fwd(g[:1].contiguous(), _params(ok), torch.ones(1, 8, device=dev),
                               torch.ones(1, 8, device=dev), 1.0)
    with pytest.raises(RuntimeError, match="c=12 unsupported"):
        _eval_call(ops, torch.randn(10, 12, device=dev), off, _head_params(12, 8, 8, 1, seed=0, dev=dev), None)
