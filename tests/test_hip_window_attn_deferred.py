"""GPU tests of the resident-window kernel's key walk without a running maximum (csrc/window_attn.hip), against
tests/window_attn_ref.py.

The first key tile pins every row's reference; the later tiles add exp2(score - reference) unscaled, and a 16-query tile
whose row sum reaches 2^64 (WA_DEFER_BOUND_BITS) or whose output is not finite is walked again with the lazy rescale.
What decides is, per row, U = lse - (row maximum over the first 64 keys), the log2 of the unscaled row sum; a CPU test
computes U from the float64 reference and asserts on which side of 64 the inputs lie:
  slow        U 48 .. 51: every query tile passes the check with probabilities up to 2^45 in its sums
  every_tile  U 183 .. 186: every query tile is walked twice
  edge        slow's ramp times 1.32, U 62 .. 65: the rows straddle the bound, so query tiles that are walked again sit
              next to tiles that are not, in the same wave and workgroup
  mixed       every third slot's logits fall: rows of both behaviours inside one 16-query tile
out and lse against float64, fp32 and bf16, eval and training forward bitwise alike; `edge` and `mixed` give the same
bits (out and lse) in every launch configuration.

The bound is the one of tests/test_hip_window_attn_paths.py: err <= 4 E + one ulp of the output dtype at max |ref|, E
measured on the CPU between the emulation and float64.  Each test names the kernel that ran with the launch profiler.
"""
import functools
import math
import os

import pytest
import torch

import window_attn_ref as R

gpu = pytest.mark.gpu

FULL = "window_attn_full_kernel"
MARGIN = 4.0
BOUND_LOG2 = 64.0      # WA_DEFER_BOUND_BITS: a row sum at or above 2^64 sends its query tile through the exact walk
F32, BF16 = torch.float32, torch.bfloat16
SHAPE = R.RESIDENT_SHAPES[0]            # (32, 2, 1024, [2100]): head_dim 16, three windows, the last one borrowing
EDGE_FACTOR = 1.32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _dt(dtype):
    return "fp32" if dtype == F32 else "bf16"


def _kernels(fn):
    """run fn with the launch profiler on -> (fn's result, names of the kernels that ran)"""
    from ptv3_hip import ops
    ops.profile_enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
        names = set(ops.profile_collect_kernels())
        ops.profile_collect()
    finally:
        ops.profile_enable(False)
    return res, names


def _ulp(dtype, mag):
    return 2.0 ** (math.floor(math.log2(max(mag, 1e-30))) - (23 if dtype == F32 else 7))


def _check(tag, got, ref, emu, out_dtype):
    """got (kernel) and emu (emulation) against the float64 ref: err <= 4 E + one ulp of out_dtype at max |ref|"""
    ref = ref.double()
    E = (emu.double() - ref).abs().max().item()
    err = (got.detach().double().cpu() - ref).abs().max().item()
    floor = _ulp(out_dtype, ref.abs().max().item())
    bound = MARGIN * E + floor
    print(f"\nWADEFER {tag}: E {E:.3e} err {err:.3e} err/E {err / max(E, 1e-300):.2f} floor {floor:.3e} "
          f"err/bound {err / bound:.3f} max|ref| {ref.abs().max().item():.3e}", end="")
    assert math.isfinite(err) and err <= bound, f"{tag}: err {err:.3e} > 4 * {E:.3e} + {floor:.3e}"


def _qkv(p, C, H, K, kind, cu):
    """ramp_qkv, and for `edge` slow's ramp stretched: the same randn (same seed), the key amplitude times EDGE_FACTOR"""
    if kind != "edge":
        return R.ramp_qkv(p["n"], C, H, p["order"], p["pad"], K, kind, seed=C + K, cu=cu)
    slow = R.ramp_qkv(p["n"], C, H, p["order"], p["pad"], K, "slow", seed=C + K, cu=cu)
    base = R.ramp_qkv(p["n"], C, H, p["order"], p["pad"], K, "randn", seed=C + K, cu=cu)
    D = C // H
    for h in range(H):
        col = C + h * D
        slow[:, col] = base[:, col] + (slow[:, col] - base[:, col]) * EDGE_FACTOR
    return slow


@functools.lru_cache(maxsize=None)
def _case(C, H, K, sizes, ragged, kind, dtype):
    """the CPU side of one case, computed once: plan, qkv, float64 reference and emulation"""
    p = R.make_plan(list(sizes), K, seed=K)
    cu = p["cu"] if ragged else None
    scale = (C // H) ** -0.5
    qkv = _qkv(p, C, H, K, kind, cu)
    if dtype == BF16:
        qkv = qkv.bfloat16().float()
    maps = (p["order"], p["inverse"], p["pad"], p["unpad"], H, K, scale)
    c = dict(p=p, cu=cu, scale=scale, qkv=qkv)
    with torch.no_grad():
        c["ref_out"], c["ref_lse"] = R.attention_f64(qkv, *maps, cu=cu)
        c["emu_out"], c["emu_lse"] = R.attention_emulated(qkv, *maps, dtype, cu=cu)
    return c


def _unscaled_log2(c, C, H, K):
    """per (query tile of 16 slots, head) of uniform windows: the largest U = lse - max over the first key tile of the
    row's log2-domain scores, from the float64 reference: log2 of the row sum the deferred walk accumulates"""
    p = c["p"]
    o = p["order"][p["pad"]]
    x = c["qkv"].double()[o]
    D = C // H
    W = o.shape[0] // K
    q, k, _ = x.reshape(W, K, 3, H, D).permute(2, 0, 3, 1, 4).unbind(0)                  # (W, H, K, D)
    s0 = (q * (c["scale"] * R.LOG2E)) @ k[:, :, :R.KEY_TILE].transpose(-2, -1)          # (W, H, K, 64)
    u = c["ref_lse"].reshape(W, K, H).permute(0, 2, 1) - s0.max(-1).values               # (W, H, K)
    return u.reshape(W, H, K // R.QUERY_TILE, R.QUERY_TILE).max(-1).values


def _maps(c, K, dev):
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


def _forward(qd, wo, wi, cu, H, K, scale):
    from ptv3_hip import ops
    return ops.window_attention_any(qd, wo, wi, H, K, scale, cu_seqlens=cu)


# ---- A: deferred against repeated walk -------------------------------------------------------------------------------
def test_inputs_lie_on_both_sides_of_the_bound():
    """no kernel: `slow` stays below 2^64 in every query tile, `every_tile` and `mixed` exceed it in every one, `edge`
    has query tiles on both sides, by more than 0.1 (the rounding of the sums moves U by 2^-8 at the most)"""
    C, H, K, sizes, _ = SHAPE
    for dtype in (F32, BF16):
        u = {kind: _unscaled_log2(_case(C, H, K, tuple(sizes), False, kind, dtype), C, H, K)
             for kind in ("slow", "every_tile", "mixed", "edge")}
        print(f"\nWADEFER U {_dt(dtype)}: " + ", ".join(f"{k} {v.min().item():.1f} .. {v.max().item():.1f}"
                                                       for k, v in u.items()), end="")
        assert u["slow"].max().item() < BOUND_LOG2 - 1 and u["slow"].max().item() > 2 * R.RESCALE_THR
        assert u["every_tile"].min().item() > BOUND_LOG2 + 1
        assert u["mixed"].min().item() > BOUND_LOG2 + 1
        below, above = (u["edge"] < BOUND_LOG2 - 0.1).sum().item(), (u["edge"] > BOUND_LOG2 + 0.1).sum().item()
        assert below >= 8 and above >= 8, (below, above)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
@pytest.mark.parametrize("kind", ["slow", "edge", "every_tile", "mixed"])
def test_deferred_and_repeated_walk_against_float64(dev, kind, dtype):
    from ptv3_hip import ops
    C, H, K, sizes, _ = SHAPE
    c = _case(C, H, K, tuple(sizes), False, kind, dtype)
    wo, wi, cu = _maps(c, K, dev)
    qd = c["qkv"].to(dev, dtype)
    out, names = _kernels(lambda: _forward(qd, wo, wi, cu, H, K, c["scale"]))
    assert names == {FULL}, names
    (out_t, lse), names = _kernels(lambda: ops.window_attention_train(qd, wo, wi, H, K, c["scale"]))
    assert names == {FULL}, names
    assert torch.equal(out_t, out)
    tag = f"A {_dt(dtype)} {kind}"
    _check(f"{tag} out", out, c["ref_out"], c["emu_out"], dtype)
    _check(f"{tag} lse", lse, c["ref_lse"], c["emu_lse"], F32)


@gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=_dt)
@pytest.mark.parametrize("kind", ["edge", "mixed"])
def test_repeat_decision_is_alike_in_every_launch_config(dev, kind, dtype):
    """The decision to walk again is taken per 16-query tile: whichever waves and workgroups the tiles are dealt to,
    the eval and the training forward give the bits of the default configuration."""
    from ptv3_hip import ops
    C, H, K, sizes, _ = SHAPE
    c = _case(C, H, K, tuple(sizes), False, kind, dtype)
    wo, wi, cu = _maps(c, K, dev)
    qd = c["qkv"].to(dev, dtype)
    try:
        ref = _forward(qd, wo, wi, cu, H, K, c["scale"])
        ref_t, ref_lse = ops.window_attention_train(qd, wo, wi, H, K, c["scale"])
        assert torch.equal(ref_t, ref)
        for waves in (8, 4):
            for qt in (4, 2, 1):
                os.environ["PTV3_ATTN_WAVES"], os.environ["PTV3_ATTN_QT"] = str(waves), str(qt)
                out, names = _kernels(lambda: _forward(qd, wo, wi, cu, H, K, c["scale"]))
                assert names == {FULL}, names
                assert torch.equal(out, ref), (kind, waves, qt)
                out_t, lse = ops.window_attention_train(qd, wo, wi, H, K, c["scale"])
                assert torch.equal(out_t, ref) and torch.equal(lse, ref_lse), (kind, waves, qt)
    finally:
        os.environ.pop("PTV3_ATTN_WAVES", None)
        os.environ.pop("PTV3_ATTN_QT", None)
