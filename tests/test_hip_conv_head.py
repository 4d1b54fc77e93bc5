"""GPU: the halo-tile 3^3 conv fused with the block head (conv_head_halo_kernel in csrc/conv_head.hip), called through
ops.conv_head_halo with PTV3_CONV_HEAD=2.

The kernel must be the composition of the two kernels it replaces: f1 and qkv are compared with torch.equal against
ops.conv_halo (PTV3_CONV_HALO=2) followed by ops.block_head on the same inputs.  A float64 restatement of
conv -> + bias -> LayerNorm + shortcut -> LayerNorm -> qkv bounds both paths with one tolerance, and a forward of the
fork config through the executor shows the kernel running where the policy takes it.

Tables are built as in test_hip_halo_conv.py: in tile space (position p of row_order), so that the number of distinct
neighbour rows of a tile is chosen."""
import contextlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def shape():
    from ptv3_hip import ops
    return ops.halo_plan_shape()


@contextlib.contextmanager
def _env(values):
    os.environ.update(values)
    try:
        yield
    finally:
        for k in values:
            os.environ.pop(k, None)


# ---- tables ------------------------------------------------------------------------------------------------------
def _uniform_table(rng, m, present):
    nbr = rng.integers(0, m, size=(m, 27))
    nbr[rng.random((m, 27)) >= present] = -1
    return nbr.astype(np.int32)


def _tile_with(rng, pool, sites, present=0.7):
    """(sites, 27) entries drawn from `pool` so that every row of the pool appears at least once; tap 20 stays absent"""
    assert len(pool) <= sites * 26
    ent = rng.choice(pool, size=sites * 26)
    ent[rng.random(sites * 26) >= present] = -1
    ent[rng.permutation(sites * 26)[:len(pool)]] = pool
    return np.insert(ent.reshape(sites, 26), 20, -1, axis=1)


def _mixed_table(rng, T, CAP):
    """m = 4T + 9 in tile space: tile 0 exactly CAP distinct rows (the last fast tile), tile 1 CAP + 1 (the first slow
    one), tile 2 centre taps only, tile 3 a few rows shared among its sites, tile 4 a partial tile."""
    m = 4 * T + 9
    assert m > CAP + 1
    t = np.full((m, 27), -1, dtype=np.int64)
    t[0:T] = _tile_with(rng, rng.permutation(m)[:CAP], T)
    t[T:2 * T] = _tile_with(rng, rng.permutation(m)[:CAP + 1], T)
    t[2 * T:3 * T, 13] = np.arange(2 * T, 3 * T)
    t[3 * T:4 * T] = _tile_with(rng, rng.permutation(m)[:40], T, present=0.3)
    t[4 * T:] = _tile_with(rng, rng.permutation(m)[:30], m - 4 * T)
    return t.astype(np.int32)


def _to_rows(tile_space, order):
    if order is None:
        return tile_space
    out = np.empty_like(tile_space)
    out[order] = tile_space
    return out


# ---- inputs and the two paths ----------------------------------------------------------------------------------
def _case(dev, dtype, nbr, order, c, seed, same_shortcut=False):
    """a block's conv and head parameters and rows; LayerNorm gains in [0.5, 1.5]"""
    m = nbr.shape[0]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, c, generator=g).to(dev, dtype)
    p = dict(
        x=x, w=(torch.randn(c, 27 * c, generator=g) / (27 * c * 0.6) ** 0.5).to(dev, dtype),
        conv_bias=torch.randn(c, generator=g).to(dev),
        shortcut=x if same_shortcut else torch.randn(m, c, generator=g).to(dev, dtype),
        g0=(torch.rand(c, generator=g) + 0.5).to(dev), b0=(torch.randn(c, generator=g) * 0.2).to(dev),
        g1=(torch.rand(c, generator=g) + 0.5).to(dev), b1=(torch.randn(c, generator=g) * 0.2).to(dev),
        wqkv=(torch.randn(3 * c, c, generator=g) / c ** 0.5).to(dev, dtype), bqkv=torch.randn(3 * c, generator=g).to(dev),
        nbr=torch.from_numpy(nbr).to(dev),
        order=None if order is None else torch.from_numpy(order.astype(np.int32)).to(dev))
    return p


def _plan(p):
    from ptv3_hip import ops
    return ops.halo_plan(p["nbr"], p["order"])


def _two_kernels(p, plan):
    from ptv3_hip import ops
    with _env({"PTV3_CONV_HALO": "2"}):
        t = ops.conv_halo(p["x"], p["w"], p["nbr"], plan, bias=p["conv_bias"], row_order=p["order"])
    return ops.block_head(t, None, 0, None, p["shortcut"], p["g0"], p["b0"], p["g1"], p["b1"],
                          ops.chain_permute(p["wqkv"], p["x"].dtype), p["bqkv"], EPS)


def _fused(p, plan):
    from ptv3_hip import ops
    with _env({"PTV3_CONV_HEAD": "2"}):
        return ops.conv_head_halo(p["x"], p["w"], p["conv_bias"], p["nbr"], plan, p["shortcut"], p["g0"], p["b0"], p["g1"],
                                  p["b1"], ops.chain_permute(p["wqkv"], p["x"].dtype), p["bqkv"], EPS, row_order=p["order"])


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _check_composition(p, plan):
    f1, qkv = _fused(p, plan)
    f1_ref, qkv_ref = _two_kernels(p, plan)
    assert torch.isfinite(f1.float()).all() and torch.isfinite(qkv.float()).all()
    assert _same_bytes(f1, f1_ref), (f1.float() - f1_ref.float()).abs().max().item()
    assert _same_bytes(qkv, qkv_ref), (qkv.float() - qkv_ref.float()).abs().max().item()


# ---- bitwise composition -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("ordered", [False, True], ids=["identity", "row_order"])
def test_is_conv_halo_then_block_head_bitwise(dev, shape, dtype, c, ordered):
    """a partial wave, a partial tile, the tile edge, three tiles; the shortcut is x itself or another tensor"""
    T, CAP = shape
    assert T == 128
    for m in (1, 15, 127, 128, 129, 300):
        rng = np.random.default_rng(1000 * m + c)
        order = rng.permutation(m) if ordered else None
        nbr = _uniform_table(rng, m, 0.6)
        for same in (False, True):
            p = _case(dev, dtype, nbr, order, c, 7 * m + c, same_shortcut=same)
            plan, counts, _, _ = _plan(p)
            assert (counts <= CAP).all()
            _check_composition(p, plan)


# ---- the overflowing-tile path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [32, 64])
def test_every_tile_overflows(dev, shape, dtype, c):
    """neighbours drawn uniformly from all 5T rows, every tap present: ~5T distinct rows per tile"""
    T, CAP = shape
    rng = np.random.default_rng(5 + c)
    m = 5 * T
    nbr = _uniform_table(rng, m, 1.0)
    order = rng.permutation(m)
    p = _case(dev, dtype, nbr, order, c, 50 + c)
    plan, counts, _, _ = _plan(p)
    assert (counts.cpu().numpy() > CAP).all()
    _check_composition(p, plan)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("ordered", [False, True], ids=["identity", "row_order"])
def test_fast_and_slow_tiles_in_one_launch(dev, shape, dtype, c, ordered):
    T, CAP = shape
    rng = np.random.default_rng(77 + c)
    tile_space = _mixed_table(rng, T, CAP)
    m = tile_space.shape[0]
    order = rng.permutation(m) if ordered else None
    p = _case(dev, dtype, _to_rows(tile_space, order), order, c, 70 + c)
    plan, counts, _, _ = _plan(p)
    counts = counts.cpu().numpy()
    assert (counts <= CAP).any() and (counts > CAP).any(), counts
    _check_composition(p, plan)


# ---- against float64 ---------------------------------------------------------------------------------------------
def _ln64(v, g, b):
    mu = v.mean(1, keepdims=True)
    var = ((v - mu) ** 2).mean(1, keepdims=True)
    return (v - mu) / np.sqrt(var + EPS) * g + b


def _float64(p):
    d = lambda t: t.double().cpu().numpy()   # noqa: E731
    x, n, c = d(p["x"]), p["nbr"].cpu().numpy(), p["x"].shape[1]
    xp = np.concatenate([x, np.zeros((1, c))])
    conv = np.einsum("mdc,odc->mo", xp[np.where(n >= 0, n, len(n))], d(p["w"]).reshape(c, 27, c)) + d(p["conv_bias"])
    f1 = _ln64(conv, d(p["g0"]), d(p["b0"])) + d(p["shortcut"])
    qkv = _ln64(f1, d(p["g1"]), d(p["b1"])) @ d(p["wqkv"]).T + d(p["bqkv"])
    return f1, qkv


# bf16 bound, in units of 2^-8 * max(1, |ref|).  One rounding to bf16 is at most 2^-8 of the value (half an ulp of
# [2^k, 2^(k+1)) is 2^(k-8)).  The chain rounds x, f1, t3 = LN_1(f1) and the output.  A LayerNorm with gains <= 1.5
# passes an input error e on as at most 1.5 * 2 * e * rstd (the direct term and the mean / variance terms), and
# e * rstd for e = 2^-8 |v| is 2^-8 of the normalised value, itself at most the output scale: a factor 3 per LayerNorm.
#   f1:  3 (x through LN_cpe) + 1 (its own rounding) = 4
#   qkv: 3 * 4 (f1 through LN_1) + 1 (t3) = 13 on the product's input; the product maps a relative error of its input
#        to the same relative error of its output scale; + 1 for the stored output = 14; fp32 accumulation is below 1e-4.
# 16 covers both.  The two-kernel path is held to the same bound in the same test.
BF16_UNITS = 16


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [32, 64])
def test_random_floats_against_float64(dev, dtype, c):
    m = 300
    rng = np.random.default_rng(900 + c)
    order = rng.permutation(m)
    p = _case(dev, dtype, _uniform_table(rng, m, 0.6), order, c, 900 + c)
    plan = _plan(p)[0]
    ref = _float64(p)
    for name, path in (("conv_halo + block_head", _two_kernels), ("conv_head_halo", _fused)):
        got = path(p, plan)
        for what, g, r in (("f1", got[0], ref[0]), ("qkv", got[1], ref[1])):
            scale = max(1.0, float(np.abs(r).max()))
            tol = (1e-4 if dtype == torch.float32 else BF16_UNITS * 2.0 ** -8) * scale
            err = float(np.abs(g.double().cpu().numpy() - r).max())
            print(f"{name} c={c} {dtype} {what}: max err {err:.3e}, bound {tol:.3e}")
            assert err < tol, (name, what, err, tol)


# ---- the executor ------------------------------------------------------------------------------------------------
KERNEL = "conv_head_halo_kernel (sparse conv + block head)"


def _fork_model():
    from pointcept.models import build_model
    from ptv3_hip.configs import FORK_CFG
    torch.manual_seed(0)
    return build_model(dict(type="OffsetKeypointPTv3", num_keypoints=6,
                            backbone_conf=dict(type="PT-v3m1", **FORK_CFG))).eval()


def _forwards(model, datad, min_rows):
    """bf16 eval forwards with PTV3_CONV_HEAD = 0 and 1: predictions, launches of the fused kernel, level sizes"""
    from ptv3_hip import ops
    preds, ran = {}, {}
    for mode in ("0", "1"):
        with _env({"PTV3_CONV_HEAD": mode, "PTV3_CONV_HEAD_MIN_ROWS": str(min_rows)}):
            ops.profile_enable(True)
            try:
                with torch.no_grad():
                    torch.manual_seed(3)
                    levels = model.backbone(datad, _head=model.head)["_stage_points"]
                    torch.manual_seed(3)
                    preds[mode] = model(datad)["pred"].clone()
                torch.cuda.synchronize()
                kernels = ops.profile_collect_kernels()
                ops.profile_collect()
            finally:
                ops.profile_enable(False)
        ran[mode] = kernels.get(KERNEL, dict(launches=0))["launches"] // 2      # two forwards per mode
    return preds, ran, levels


def _fused_blocks(levels, min_rows):
    """(blocks the executor fuses, whether the old conv of any of them splits over K): every block of a width and row
    count the policy takes, but the first block of an encoder level"""
    from ptv3_hip import ops
    from ptv3_hip.configs import FORK_CFG as F
    want, split = 0, False
    for st, n in enumerate(levels):
        blocks = [(F["enc_channels"][st], F["enc_depths"][st] - 1)]
        if st < len(F["dec_channels"]):
            blocks.append((F["dec_channels"][st], F["dec_depths"][st]))
        for c, count in blocks:
            with _env({"PTV3_CONV_HEAD_MIN_ROWS": str(min_rows)}):
                taken = ops.conv_head_halo_policy(n, c, torch.bfloat16)
            if taken and count > 0 and ops.block_fusable(c, 4 * c, torch.bfloat16, n) == 1:
                want += count
                split = split or ops.gemm_splits(n, c, c, 27, torch.bfloat16) > 1
    return want, split


def test_forward_through_the_executor_levels_0_and_1(dev):
    """The fork config at 6000 points in bf16 with the row bound lowered to 1: the 64-channel blocks of levels 0 and 1
    take the fused kernel, against PTV3_CONV_HEAD=0.  The old conv splits over K at these sizes (ops.gemm_splits), so the conv's summation
    order differs and the predictions are not compared with each other: each is held to the bf16 bound of
    test_fork_config_at_bench_scene_vs_oracle against the oracle."""
    from oracle import ptv3 as O
    from ptv3_hip.configs import FORK_CFG
    import ptv3_scenes as S
    model = _fork_model()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    data = S.make_batch([6000], in_channels=4, extent=None, seed=21, with_target=6)
    torch.manual_seed(3)
    with torch.no_grad():
        ref = O.OffsetKeypointOracle(FORK_CFG, sd).forward(data)
    model = model.to(dev)
    model.backbone.compute_dtype = torch.bfloat16
    preds, ran, levels = _forwards(model, {k: v.to(dev) for k, v in data.items()}, 1)
    want, split = _fused_blocks(levels, 1)
    assert want == 5, (want, levels)                          # C = 64: encoder 1 one block; decoder 0 and 1 two each
    assert ran == {"0": 0, "1": want}, (ran, want, levels)
    assert torch.isfinite(preds["1"].float()).all()
    if not split:
        assert _same_bytes(preds["0"], preds["1"])
    scale = max(1.0, ref["logits"].abs().max().item())
    for mode in ("0", "1"):
        err = (preds[mode].float().cpu() - ref["pred"]).abs()
        print(f"PTV3_CONV_HEAD={mode}: split {split}, max err {err.max().item():.3e}, mean {err.mean().item():.3e} "
              f"(scale {scale:.3f}), fused launches {ran[mode]}")
        assert err.max().item() < 64 * 2.0 ** -8 * scale, (mode, err.max().item(), scale)
        assert err.mean().item() < 8 * 2.0 ** -8 * scale, (mode, err.mean().item(), scale)


def test_forward_is_byte_equal_where_the_old_conv_does_not_split(dev):
    """33 000 points: level 0 holds more than the 32 768 rows from which a 64-channel conv runs in a single pass.  With the
    row bound at level 0's size the fused kernel replaces single-pass convs only, and the prediction keeps its bytes."""
    import ptv3_scenes as S
    model = _fork_model().to(dev)
    model.backbone.compute_dtype = torch.bfloat16
    datad = {k: v.to(dev) for k, v in S.make_batch([33000], in_channels=4, extent=160, seed=21).items()}
    with torch.no_grad():
        n0 = model.backbone(datad, _head=model.head)["_stage_points"][0]
    preds, ran, levels = _forwards(model, datad, n0)
    want, split = _fused_blocks(levels, n0)
    assert want == 2 and not split, (want, split, levels)     # decoder 0 (C = 64): two blocks
    assert ran == {"0": 0, "1": want}, (ran, want, levels)
    assert torch.isfinite(preds["1"].float()).all()
    assert _same_bytes(preds["0"], preds["1"])
