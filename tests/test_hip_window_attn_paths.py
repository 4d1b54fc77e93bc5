"""GPU tests of the two paths of csrc/window_attn.hip no older test can fail on, and of csrc/attn_bwd.hip at the same
shapes, against tests/window_attn_ref.py:

A. the resident-window kernel under growing logits: the lazy softmax rescale (alpha = exp2(-d), d = max(d, 0) for the
   rows that did not grow, negm -= d, the row sums, probabilities up to 2^8 packed to bf16, lse after several rescales)
   only runs when a row maximum outgrows its reference by 8 log2 units, which randn qkv never does
   (tests/test_window_attn_reference_cpu.py).  Five input kinds, fp32 and bf16, head_dim 16 / 32 / 64, ragged windows;
   every launch configuration gives the bits of the default one.
B. the tiled kernel without dropout (windows whose K and V do not fit 160 KB of LDS): out, the training forward's lse,
   the dense bias branch, ragged windows, all three head_dim instantiations.
C. both backward entry points (statistics recomputed / taken from the forward) at B's shapes.
D. the tiled kernel with more than 64 KB of dynamic LDS (K = 8192, fp32, head_dim 64).

Each test names the kernel that ran with the launch profiler.

Tolerances.  Nothing here is within the project's usual 1e-4: the log2-domain scores reach 190 (416 in B).  For every
case the yardstick is E = max |attention_emulated - attention_f64| on the CPU (the same formula with the roundings the
kernel header documents; for gradients, autograd over both), and the kernel must stay within 4 E + floor, floor = one
unit in the last place of the output dtype at the reference's largest magnitude; 4 is the factor test_gva_vs_float64
uses for "same formula, another summation order".  bf16 cases round qkv (and dout) to bf16 first, so E holds the
kernel's roundings and not the input's.  Every check prints E, the kernel's error, err / E and err / bound.

A, B and dk, dv of C hold 4 E + floor as it stands.  Two checks were measured above it, each for a reason the emulation
cannot show, and get a term computed from the reference and the fp32 format (never from a kernel's output):
- D, forward out (_walk): the fp32 kernel adds all keys of a window into one accumulator, one rounded update per
  16x16x4 MFMA step, K / 4 = 2048 of them; torch sums in blocks.  Term: a random walk of sqrt(K / 4) half fp32 ulps at
  max |ref| (E = 6.6e-8 is 9 ulps there).
- C, backward dq: the kernels take delta = dO . O from the forward's output and recompute p from the scores, so the
  per-key rounding of a recomputed score (fp32 at magnitude 2^7: 1e-5) is not cancelled in sum_keys dS = 0 and is
  multiplied by the common component of k (150 for `every_tile`); autograd over one softmax cancels it exactly.
  Term: scale * ln2 * e * max over (query, head, channel) of sqrt(sum_keys (p |dP - delta| k)^2)
  (window_attn_ref.backward_score_sensitivity), e = sqrt(head_dim / 4) half fp32 ulps at the largest sum_d |q_d k_d|:
  one rounded update per MFMA step of the score.  The fp32 dq errors from before the attn_bwd.hip fix (below) are
  outside this bound at all three shapes.

Largest err / E per group on an MI355X (one run; the bound is 4 + (floor + term) / E):
  group  what      fp32                                          bf16
  A      out       2.06                                          1.47
  A      lse       1.25                                          1.09
  B      out       1.28 (dense bias 1.13)                        1.04 (dense bias 1.00)
  B      lse       1.03                                          1.05
  C      dq        14.45 (E 6.2e-5, err 9.0e-4, term 2.2e-3)     1.36
  C      dk        2.17                                          1.18
  C      dv        2.38                                          2.08
  D      out       4.98 (E 6.6e-8, err 3.3e-7, term 1.7e-7)      -
Before attn_bwd.hip recomputed its scores from the pre-scaled q as the forward does, C read: bf16 dk through
ptv3_window_attn_train_bwd 38.7 (err 6.6 at max |dk| 27.8: the forward's lse against differently rounded scores),
fp32 dq 129.8.
"""
import functools
import math
import os

import pytest
import torch

import window_attn_ref as R

pytestmark = pytest.mark.gpu

FULL = "window_attn_full_kernel"
TILED = "window_attn_kernel"
MARGIN = 4.0
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _kernels(fn):
    """run fn with the launch profiler on -> (fn's result, names of the kernels that ran)"""
    from ptv3_hip import ops
    ops.profile_enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
        names = set(ops.profile_collect_kernels())
        ops.profile_collect()          # resets the records
    finally:
        ops.profile_enable(False)
    return res, names


def _ulp(dtype, mag):
    """one unit in the last place of dtype at magnitude mag"""
    return 2.0 ** (math.floor(math.log2(max(mag, 1e-30))) - (23 if dtype == F32 else 7))


def _check(tag, got, ref, emu, out_dtype, extra=0.0):
    """got (kernel) and emu (emulation) against the float64 ref: err <= 4 E + one ulp of out_dtype at max |ref|
    (+ extra: a term derived from the reference and the number formats, see the module docstring)"""
    ref = ref.double()
    E = (emu.double() - ref).abs().max().item()
    err = (got.detach().double().cpu() - ref).abs().max().item()
    floor = _ulp(out_dtype, ref.abs().max().item())
    bound = MARGIN * E + floor + extra
    print(f"\nWAPATH {tag}: E {E:.3e} err {err:.3e} err/E {err / max(E, 1e-300):.2f} floor {floor:.3e} "
          f"extra {extra:.3e} err/bound {err / bound:.3f} max|ref| {ref.abs().max().item():.3e}", end="")
    assert math.isfinite(err) and err <= bound, f"{tag}: err {err:.3e} > 4 * {E:.3e} + {floor:.3e} + {extra:.3e}"


def _walk(K, ref):
    """group D (fp32) forward out: the kernel adds the keys of a window into ONE fp32 accumulator, one update per
    16x16x4 MFMA step = K / 4 updates, each rounding it by up to half an fp32 ulp: a random walk of sqrt(K / 4) half
    ulps at the reference's largest magnitude.  The blocked sums of the torch emulation do not walk."""
    return math.sqrt(K / 4.0) * 0.5 * _ulp(F32, ref.abs().max().item())


@functools.lru_cache(maxsize=None)
def _case(C, H, K, sizes, ragged, kind, dtype, with_bias=False, grads=False):
    """the CPU side of one case, computed once: plan, qkv, float64 reference and emulation (forward, and with grads
    the gradients of both under one dout)"""
    p = R.make_plan(list(sizes), K, seed=K)
    cu = p["cu"] if ragged else None
    scale = (C // H) ** -0.5
    qkv = R.ramp_qkv(p["n"], C, H, p["order"], p["pad"], K, kind, seed=C + K, cu=cu)
    g = torch.Generator().manual_seed(K + 1)
    dout = torch.randn(p["n"], C, generator=g)
    bias = 0.5 * torch.randn(p["pad"].shape[0] // K, H, K, K, generator=g) if with_bias else None
    if dtype == BF16:
        qkv, dout = qkv.bfloat16().float(), dout.bfloat16().float()
    maps = (p["order"], p["inverse"], p["pad"], p["unpad"], H, K, scale)
    c = dict(p=p, cu=cu, scale=scale, qkv=qkv, dout=dout, bias=bias)
    if grads:
        leaf = qkv.clone().requires_grad_(True)
        c["ref_out"], c["ref_lse"] = R.attention_f64(leaf, *maps, cu=cu, bias=bias)
        c["ref_out"].backward(dout.double())
        c["ref_grad"] = leaf.grad.double()
        leaf = qkv.clone().requires_grad_(True)
        c["emu_out"], c["emu_lse"] = R.attention_emulated(leaf, *maps, dtype, cu=cu, bias=bias)
        c["emu_out"].backward(dout)
        c["emu_grad"] = leaf.grad
        for k in ("ref_out", "ref_lse", "emu_out", "emu_lse"):
            c[k] = c[k].detach()
        c["sens"] = R.backward_score_sensitivity(qkv, dout, *maps, cu=cu)
    else:
        with torch.no_grad():
            c["ref_out"], c["ref_lse"] = R.attention_f64(qkv, *maps, cu=cu, bias=bias)
            c["emu_out"], c["emu_lse"] = R.attention_emulated(qkv, *maps, dtype, cu=cu, bias=bias)
    return c


def _maps(c, K, dev):
    """the window maps of the case on the GPU (ragged: with cu_seqlens), checked against the CPU pad plan"""
    from ptv3_hip import ops
    p = c["p"]
    order, inverse, off = p["order"][None].to(dev), p["inverse"][None].to(dev), p["off"].to(dev)
    if c["cu"] is not None:
        wo, wi, cu = ops.window_plan(order, inverse, off, p["off"].tolist(), K, with_cu=True)
        assert torch.equal(cu.cpu(), p["cu"])
    else:
        wo, wi = ops.window_plan(order, inverse, off, p["off"].tolist(), K)
        cu = None
    wo, wi = wo[0].contiguous(), wi[0].contiguous()
    assert torch.equal(wo.cpu().long(), p["order"][p["pad"]]) and torch.equal(wi.cpu().long(), p["unpad"][p["inverse"]])
    return wo, wi, cu


def _forward(qd, wo, wi, cu, H, K, scale, bias=None):
    from ptv3_hip import ops
    if cu is not None:
        return ops.window_attention_varlen(qd, wo, wi, cu, H, K, scale)
    return ops.window_attention(qd, wo, wi, H, K, scale, rpe_bias=bias)


def _forward_checks(tag, c, dtype, H, K, dev, kernel):
    """eval forward (the named kernel ran) and training forward: out and lse against float64, the two outs bitwise"""
    from ptv3_hip import ops
    wo, wi, cu = _maps(c, K, dev)
    qd = c["qkv"].to(dev, dtype)
    out, names = _kernels(lambda: _forward(qd, wo, wi, cu, H, K, c["scale"]))
    assert names == {kernel}, names
    (out_t, lse), names = _kernels(lambda: ops.window_attention_train(qd, wo, wi, H, K, c["scale"], cu_seqlens=cu))
    assert names == {kernel}, names
    assert torch.equal(out_t, out)
    _check(f"{tag} out", out, c["ref_out"], c["emu_out"], dtype)
    _check(f"{tag} lse", lse, c["ref_lse"], c["emu_lse"], F32)
    return qd, wo, wi, cu, out, lse


def _dt(dtype):
    return "fp32" if dtype == F32 else "bf16"


# ---- A: resident-window kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape", R.RESIDENT_SHAPES, ids=lambda s: f"C{s[0]}-K{s[2]}")
def test_resident_kernel_under_growing_logits(dev, shape, kind, dtype):
    C, H, K, sizes, ragged = shape
    assert not R.takes_tiled_kernel(4 if dtype == F32 else 2, C // H, K)
    c = _case(C, H, K, tuple(sizes), ragged, kind, dtype)
    _forward_checks(f"A {_dt(dtype)} C{C} K{K} {kind}", c, dtype, H, K, dev, FULL)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
@pytest.mark.parametrize("kind", ["every_tile", "mixed"])
def test_resident_kernel_rescales_alike_in_every_launch_config(dev, kind, dtype):
    """The rescale decision is taken per 16-query tile, so it does not depend on how tiles are dealt to waves: every
    (waves per workgroup, query tiles per wave) gives the bits of the configuration the cost model picks."""
    C, H, K, sizes, ragged = R.RESIDENT_SHAPES[0]
    c = _case(C, H, K, tuple(sizes), ragged, kind, dtype)
    wo, wi, cu = _maps(c, K, dev)
    qd = c["qkv"].to(dev, dtype)
    try:
        ref = _forward(qd, wo, wi, cu, H, K, c["scale"])
        for waves in (8, 4):
            for qt in (4, 2, 1):
                os.environ["PTV3_ATTN_WAVES"], os.environ["PTV3_ATTN_QT"] = str(waves), str(qt)
                out, names = _kernels(lambda: _forward(qd, wo, wi, cu, H, K, c["scale"]))
                assert names == {FULL}, names
                assert torch.equal(out, ref), (kind, waves, qt)
    finally:
        os.environ.pop("PTV3_ATTN_WAVES", None)
        os.environ.pop("PTV3_ATTN_QT", None)


# ---- B: tiled kernel without dropout ---------------------------------------------------------------------------------
def _tiled_id(s):
    return f"{'fp32' if s[0] == 4 else 'bf16'}-C{s[1]}-K{s[3]}"


def _tiled_case(shape, ragged, kind, **kw):
    esize, C, H, K, sizes = shape
    dtype = F32 if esize == 4 else BF16
    assert R.takes_tiled_kernel(esize, C // H, K)
    sizes = tuple(sizes) + ((R.RAGGED_EXTRA,) if ragged else ())
    return _case(C, H, K, sizes, ragged, kind, dtype, **kw), dtype


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("kind", ["randn", "every_tile"])
@pytest.mark.parametrize("shape", R.TILED_SHAPES, ids=_tiled_id)
def test_tiled_kernel_without_dropout(dev, shape, kind, ragged):
    _, C, H, K, _ = shape
    c, dtype = _tiled_case(shape, ragged, kind)
    _forward_checks(f"B {_dt(dtype)} C{C} K{K} {kind} {'ragged' if ragged else 'uniform'}", c, dtype, H, K, dev, TILED)


@pytest.mark.parametrize("kind", ["randn", "every_tile"])
@pytest.mark.parametrize("shape", [R.TILED_SHAPES[1], R.TILED_SHAPES[4]], ids=_tiled_id)
def test_tiled_kernel_dense_bias(dev, shape, kind):
    _, C, H, K, _ = shape
    c, dtype = _tiled_case(shape, False, kind, with_bias=True)
    wo, wi, _ = _maps(c, K, dev)
    qd, bias = c["qkv"].to(dev, dtype), c["bias"].to(dev)
    out, names = _kernels(lambda: _forward(qd, wo, wi, None, H, K, c["scale"], bias=bias))
    assert names == {TILED}, names
    _check(f"B-bias {_dt(dtype)} C{C} K{K} {kind} out", out, c["ref_out"], c["emu_out"], dtype)
    # the bias matters at this tolerance: the reference without it is further away than the bound allows
    plain, _ = _tiled_case(shape, False, kind)
    gap = (plain["ref_out"] - c["ref_out"]).abs().max().item()
    E = (c["emu_out"].double() - c["ref_out"]).abs().max().item()
    assert gap > 2 * (MARGIN * E + _ulp(dtype, c["ref_out"].abs().max().item())), (gap, E)


# ---- C: backward at the tiled shapes ---------------------------------------------------------------------------------
BWD_SHAPES = [(4, 64, 2, 650, [1430]), (2, 64, 2, 650, [1430]), (4, 128, 2, 330, [726]), (2, 128, 2, 330, [726]),
              (4, 32, 2, 1160, [2552])]


@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("kind", ["randn", "every_tile"])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=_tiled_id)
def test_backward_at_the_tiled_shapes(dev, shape, kind, ragged):
    """ptv3_window_attn_bwd / _varlen_bwd (statistics recomputed) and ptv3_window_attn_train_bwd (the forward's lse)
    against torch autograd over attention_f64 with the same dout; borrowed points receive the sum of their two slots."""
    from ptv3_hip import ops
    esize, C, H, K, sizes = shape
    dtype = F32 if esize == 4 else BF16
    sizes = tuple(sizes) + ((R.RAGGED_EXTRA,) if ragged else ())
    c = _case(C, H, K, sizes, ragged, kind, dtype, grads=True)
    assert (c["p"]["pad"].bincount() == 2).any()          # some points are borrowed
    wo, wi, cu = _maps(c, K, dev)
    qd, dd = c["qkv"].to(dev, dtype), c["dout"].to(dev, dtype)
    (out, lse), names = _kernels(lambda: ops.window_attention_train(qd, wo, wi, H, K, c["scale"], cu_seqlens=cu))
    assert names == {TILED if R.takes_tiled_kernel(esize, C // H, K) else FULL}, names   # bf16 K = 330 / 650: resident
    d0 = ops.window_attention_bwd(qd, out, dd, wo, wi, H, K, c["scale"], cu_seqlens=cu)
    d1 = ops.window_attention_train_bwd(qd, out, dd, lse, wo, wi, H, K, c["scale"], cu_seqlens=cu)
    tag = f"C {_dt(dtype)} C{C} K{K} {kind} {'ragged' if ragged else 'uniform'}"
    # dq: what the rounding of a recomputed score adds (R.backward_score_sensitivity).  A score is a head_dim-term fp32
    # dot product whose partial sums reach smax, rounded once per 16x16x4 MFMA step: a random walk of
    # sqrt(head_dim / 4) half ulps at smax, the model of _walk.  dk and dv need no such term: q has no large common
    # component, and dv has no cancellation.
    sens = c["sens"]
    e = math.sqrt((C // H) / 4.0) * 0.5 * _ulp(F32, sens["smax"])
    extra = dict(dq=c["scale"] * math.log(2.0) * e * sens["dq_walk"], dk=0.0, dv=0.0)
    for name, got in (("recompute", d0), ("train", d1)):
        for i, part in enumerate(("dq", "dk", "dv")):
            sl = slice(i * C, (i + 1) * C)
            _check(f"{tag} {name} {part}", got[:, sl], c["ref_grad"][:, sl], c["emu_grad"][:, sl], dtype,
                   extra=extra[part])


# ---- D: more than 64 KB of dynamic LDS -------------------------------------------------------------------------------
def test_tiled_kernel_with_more_than_64k_of_lds(dev):
    """fp32, head_dim 64, K = 8192: 34 816 bytes of K / V tiles + 32 768 bytes of slot indices = 67 584 bytes, above the
    64 KB a kernel may use without hipFuncAttributeMaxDynamicSharedMemorySize; the launcher raises the attribute."""
    esize, C, H, K, sizes = R.LARGE_SHAPE
    assert R.tiled_lds_bytes(esize, C // H, K) == 67584
    c = _case(C, H, K, tuple(sizes), False, "randn", F32)
    assert c["p"]["pad"].shape[0] == 2 * K
    wo, wi, _ = _maps(c, K, dev)
    qd = c["qkv"].to(dev)
    out, names = _kernels(lambda: _forward(qd, wo, wi, None, H, K, c["scale"]))
    assert names == {TILED}, names
    _check(f"D fp32 C{C} K{K} randn out", out, c["ref_out"], c["emu_out"], F32, extra=_walk(K, c["ref_out"]))
