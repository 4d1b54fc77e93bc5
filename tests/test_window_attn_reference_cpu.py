"""CPU checks of tests/window_attn_ref.py, the reference of tests/test_hip_window_attn_paths.py:

- attention_f64 is the oracle's window attention (uniform windows) and a per-window loop (ragged windows);
- the inputs have the property they were made for: randn qkv never asks the resident-window kernel for a lazy
  rescale at any shape of the GPU file (why the older tests cannot see that path), `every_tile` asks in every later
  key tile, `slow`, `staircase` and `mixed` at least twice wherever a window has 3 key tiles or more;
- the restated launcher formula names the first window length that takes the tiled kernel."""
import math

import pytest
import torch

import window_attn_ref as R


def test_attention_f64_is_the_oracle_on_a_ragged_batch():
    from oracle import ptv3 as O
    C, H, K = 32, 2, 64
    p = R.make_plan([300, 200, 131], K, seed=1)
    qkv = R.ramp_qkv(p["n"], C, H, p["order"], p["pad"], K, "slow", seed=2)
    out, lse = R.attention_f64(qkv, p["order"], p["inverse"], p["pad"], p["unpad"], H, K, (C // H) ** -0.5)
    ref = O.window_attention_core(qkv.double(), p["order"], p["inverse"], p["pad"], p["unpad"], H, K)
    assert out.dtype == torch.float64 and tuple(lse.shape) == (p["pad"].shape[0], H)
    assert (out - ref).abs().max().item() < 1e-12
    # the ragged statement over the same (uniform) cu_seqlens gives the same numbers
    out2, lse2 = R.attention_f64(qkv, p["order"], p["inverse"], p["pad"], p["unpad"], H, K, (C // H) ** -0.5, cu=p["cu"])
    assert torch.equal(out, out2) and torch.equal(lse, lse2)


def test_attention_f64_is_a_per_window_loop_with_cu_seqlens():
    C, H, K = 64, 4, 128
    D = C // H
    scale = D ** -0.5
    p = R.make_plan([300, 40, 130], K, seed=3)
    cu = [int(v) for v in p["cu"]]
    assert sorted(set(b - a for a, b in zip(cu[:-1], cu[1:]))) == [40, 128]
    qkv = R.ramp_qkv(p["n"], C, H, p["order"], p["pad"], K, "every_tile", seed=4, cu=p["cu"])
    bias = None
    out, lse = R.attention_f64(qkv, p["order"], p["inverse"], p["pad"], p["unpad"], H, K, scale, cu=p["cu"], bias=bias)
    x = qkv.double()[p["order"][p["pad"]]]
    want = torch.zeros(x.shape[0], C, dtype=torch.float64)
    want_lse = torch.zeros(x.shape[0], H, dtype=torch.float64)
    for a, b in zip(cu[:-1], cu[1:]):
        for h in range(H):
            q = x[a:b, h * D:(h + 1) * D]
            k = x[a:b, C + h * D:C + (h + 1) * D]
            v = x[a:b, 2 * C + h * D:2 * C + (h + 1) * D]
            s = scale * q @ k.T
            want[a:b, h * D:(h + 1) * D] = torch.softmax(s, dim=-1) @ v
            want_lse[a:b, h] = torch.logsumexp(s, dim=-1) / math.log(2.0)
    assert (out - want[p["unpad"][p["inverse"]]]).abs().max().item() < 1e-12
    assert (lse - want_lse).abs().max().item() < 1e-10


def test_attention_f64_adds_a_dense_bias():
    C, H, K = 32, 2, 50
    scale = (C // H) ** -0.5
    p = R.make_plan([120], K, seed=5)
    g = torch.Generator().manual_seed(6)
    qkv = torch.randn(p["n"], 3 * C, generator=g)
    W = p["pad"].shape[0] // K
    bias = 0.5 * torch.randn(W, H, K, K, generator=g)
    out, _ = R.attention_f64(qkv, p["order"], p["inverse"], p["pad"], p["unpad"], H, K, scale, bias=bias)
    x = qkv.double()[p["order"][p["pad"]]].reshape(W, K, 3, H, C // H).permute(2, 0, 3, 1, 4)
    want = torch.softmax(scale * x[0] @ x[1].transpose(-2, -1) + bias.double(), dim=-1) @ x[2]
    want = want.transpose(1, 2).reshape(-1, C)[p["unpad"][p["inverse"]]]
    assert (out - want).abs().max().item() < 1e-12


def test_emulated_forms_stay_near_float64_and_are_differentiable():
    C, H, K = 32, 2, 64
    scale = (C // H) ** -0.5
    p = R.make_plan([150], K, seed=7)
    args = (p["order"], p["inverse"], p["pad"], p["unpad"], H, K, scale)
    qkv = R.ramp_qkv(p["n"], C, H, p["order"], p["pad"], K, "every_tile", seed=8).bfloat16().float()
    ref, ref_lse = R.attention_f64(qkv, *args)
    for dtype, tol in ((torch.float32, 1e-5), (torch.bfloat16, 0.1)):
        leaf = qkv.clone().requires_grad_(True)
        out, lse = R.attention_emulated(leaf, *args, dtype)
        assert out.dtype == torch.float32 and lse.dtype == torch.float32
        assert (out.double() - ref).abs().max().item() < tol * ref.abs().max().item()
        assert (lse.double() - ref_lse).abs().max().item() < tol * ref_lse.abs().max().item()
        out.sum().backward()
        assert torch.isfinite(leaf.grad).all() and leaf.grad.abs().max().item() > 0


def _all_shapes():
    """(C, H, K, sizes, ragged) of every case of the GPU file"""
    shapes = list(R.RESIDENT_SHAPES)
    for _, C, H, K, sizes in R.TILED_SHAPES:
        shapes.append((C, H, K, sizes, False))
        shapes.append((C, H, K, sizes + [R.RAGGED_EXTRA], True))
    _, C, H, K, sizes = R.LARGE_SHAPE
    shapes.append((C, H, K, sizes, False))
    return shapes


def _events(C, H, K, sizes, ragged, kind, bf16):
    p = R.make_plan(sizes, K, seed=K)
    cu = p["cu"] if ragged else None
    qkv = R.ramp_qkv(p["n"], C, H, p["order"], p["pad"], K, kind, seed=C + K, cu=cu)
    if bf16:
        qkv = qkv.bfloat16().float()
    return R.rescale_events(qkv, p["order"], p["pad"], H, K, (C // H) ** -0.5, cu=cu)


@pytest.mark.parametrize("shape", _all_shapes(), ids=lambda s: f"C{s[0]}-H{s[1]}-K{s[2]}-{'ragged' if s[4] else 'uniform'}")
def test_randn_never_asks_for_a_rescale(shape):
    """the documented reason the older attention tests miss the lazy-rescale path"""
    for bf16 in (False, True):
        events, later = _events(*shape, "randn", bf16)
        assert later.max().item() >= 1
        assert int(events.sum()) == 0


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", R.RESIDENT_SHAPES, ids=lambda s: f"C{s[0]}-K{s[2]}")
def test_every_tile_rescales_in_every_later_key_tile(shape, bf16):
    events, later = _events(*shape, "every_tile", bf16)
    assert later.max().item() == (shape[2] + R.KEY_TILE - 1) // R.KEY_TILE - 1
    assert torch.equal(events, later)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["slow", "staircase", "mixed"])
@pytest.mark.parametrize("shape", R.RESIDENT_SHAPES, ids=lambda s: f"C{s[0]}-K{s[2]}")
def test_other_ramps_rescale_at_least_twice_in_windows_of_three_key_tiles(shape, kind, bf16):
    events, later = _events(*shape, kind, bf16)
    long = later >= 2
    if shape[2] > 2 * R.KEY_TILE:
        assert long.any()
    assert (events[long] >= 2).all(), (events[long].min().item(), int((events[long] < 2).sum()))
    if kind == "slow" and shape[2] == 1024:
        # three units per tile: a rescale roughly every third tile, not every tile
        assert events.max().item() <= 8


def test_mixed_has_falling_rows_in_every_query_tile():
    """every third slot of `mixed` has its maximum in key tile 0 and shares a 16-row tile with growing rows"""
    C, H, K, sizes, _ = R.RESIDENT_SHAPES[0]
    p = R.make_plan(sizes, K, seed=K)
    qkv = R.ramp_qkv(p["n"], C, H, p["order"], p["pad"], K, "mixed", seed=C + K)
    D = C // H
    x = qkv.double()[p["order"][p["pad"]]].reshape(-1, K, 3, H, D).permute(2, 0, 3, 1, 4)
    s = (x[0] * D ** -0.5) @ x[1].transpose(-2, -1)                  # (W, H, K, K)
    arg = s.argmax(-1)
    falling = torch.arange(K) % 3 == 2
    # the last window holds borrowed points that keep the sign of their own slot: check the windows without them
    assert (arg[:-1, :, falling] < R.KEY_TILE).all()
    assert (arg[:-1, :, ~falling] >= K - R.KEY_TILE).all()


def test_first_window_that_takes_the_tiled_kernel():
    want = {(4, 64): 320, (4, 32): 640, (4, 16): 1152, (2, 64): 640, (2, 32): 1216, (2, 16): 2176}
    for (esize, d), K in want.items():
        assert R.first_tiled_window(esize, d) == K, (esize, d)
        assert not R.takes_tiled_kernel(esize, d, K - R.KEY_TILE)
    # the GPU file's shapes sit on the side they were chosen for
    for C, H, K, _, _ in R.RESIDENT_SHAPES:
        assert not R.takes_tiled_kernel(4, C // H, K) and not R.takes_tiled_kernel(2, C // H, K)
    for esize, C, H, K, _ in R.TILED_SHAPES + [R.LARGE_SHAPE]:
        assert R.takes_tiled_kernel(esize, C // H, K)
    for esize, C, H, K, _ in R.TILED_SHAPES:
        assert K % R.KEY_TILE
        assert K - R.first_tiled_window(esize, C // H) < R.KEY_TILE       # the first tiled window, plus a partial tile
    esize, C, H, K, _ = R.LARGE_SHAPE
    assert R.tiled_lds_bytes(esize, C // H, K) == 67584 > 64 * 1024
    # where the tiled kernel's dynamic LDS passes 64 KB
    assert R.tiled_lds_bytes(4, 64, 7680) <= 64 * 1024 < R.tiled_lds_bytes(4, 64, 7681)
    assert R.tiled_lds_bytes(4, 32, 11904) <= 64 * 1024 < R.tiled_lds_bytes(4, 32, 11905)
    for esize in (2, 4):
        for d in (16, 32, 64):
            assert R.tiled_lds_bytes(esize, d, 16384) > 64 * 1024
