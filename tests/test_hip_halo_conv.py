"""GPU: the halo tile of the narrow 3^3 convolutions (ptv3_halo_plan_build in csrc/sparse.hip, conv_halo_kernel in
csrc/gemm.hip), called through ops.halo_plan / ops.conv_halo with PTV3_CONV_HALO=2.

Two references: the existing single-pass path (PTV3_CONV_HALO=0, PTV3_CONV_TILE=0, PTV3_GEMM_BIG=0, PTV3_GEMM_SPLITK=0),
which the new kernel must match with torch.equal, and an int64 computation on the CPU over integer inputs in [-3, 3]
(|sum| <= 27 * 64 * 9 < 2^24: every partial sum is exact in fp32 whatever the order), which does not depend on the code
under test.  In those cases the output tensor starts NaN-filled, so a skipped store shows.

Tiles are runs of T consecutive entries of row_order; (T, CAP) come from ops.halo_plan_shape().  Synthetic tables are
built in tile space (position p of row_order) so that the number of distinct neighbour rows of a tile is chosen."""
import contextlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OLD_PATH = {"PTV3_CONV_HALO": "0", "PTV3_CONV_TILE": "0", "PTV3_GEMM_BIG": "0", "PTV3_GEMM_SPLITK": "0"}
NEW_PATH = {"PTV3_CONV_HALO": "2"}
DTYPES = [torch.float32, torch.bfloat16]
ABSENT = -1          # 0xFFFF seen as int16


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


def _old(x, w, nbr, order, **epi):
    from ptv3_hip import ops
    with _env(OLD_PATH):
        return ops.gemm(x, w, nbr=nbr, kvol=27, row_order=order, **epi)


def _new(x, w, nbr, order, plan=None, **epi):
    from ptv3_hip import ops
    with _env(NEW_PATH):
        if plan is None:
            plan = ops.halo_plan(nbr, order)[0]
        return ops.conv_halo(x, w, nbr, plan, row_order=order, **epi)


# ---- tables --------------------------------------------------------------------------------------------------
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
    """m = 5T + 9, in tile space: tile 0 exactly CAP distinct rows (the last fast tile), tile 1 CAP + 1 (the first slow
    one), tile 2 centre taps only, tile 3 one row that is a neighbour of every site, tile 4 neighbours from other
    tiles' ranges only, tile 5 a partial tile; tap 20 absent everywhere."""
    m = 5 * T + 9
    assert m > CAP + 1
    t = np.full((m, 27), -1, dtype=np.int64)
    t[0:T] = _tile_with(rng, rng.permutation(m)[:CAP], T)
    t[T:2 * T] = _tile_with(rng, rng.permutation(m)[:CAP + 1], T)
    t[2 * T:3 * T, 13] = np.arange(2 * T, 3 * T)
    t[3 * T:4 * T] = _tile_with(rng, rng.permutation(m)[:40], T, present=0.3)
    t[3 * T:4 * T, 5] = 7
    outside = np.concatenate([np.arange(0, 4 * T), np.arange(5 * T, m)])
    t[4 * T:5 * T] = _tile_with(rng, rng.choice(outside, 200, replace=False), T)
    t[5 * T:] = _tile_with(rng, rng.permutation(m)[:30], m - 5 * T)
    return t.astype(np.int32)


def _to_rows(tile_space, order):
    """table in tile space (row p = site order[p]; its VALUES are rows of x already) -> table indexed by row"""
    if order is None:
        return tile_space
    out = np.empty_like(tile_space)
    out[order] = tile_space
    return out


def _exact(x, w, nbr, bias):
    """int64 statement of the convolution: x (m, c), w (c, 27, c), nbr (m, 27), bias (c)"""
    xp = np.concatenate([x.astype(np.int64), np.zeros((1, x.shape[1]), np.int64)])
    g = xp[np.where(nbr >= 0, nbr, len(x))]                       # (m, 27, c)
    return np.einsum("mdc,odc->mo", g, w.astype(np.int64)) + bias.astype(np.int64)


def _int_case(rng, m, c):
    x = rng.integers(-3, 4, size=(m, c))
    w = rng.integers(-3, 4, size=(c, 27, c))
    bias = rng.integers(-3, 4, size=c)
    return x, w, bias


def _check_exact(dev, dtype, nbr, order, c, rng, expect_counts=None):
    from ptv3_hip import ops
    m = nbr.shape[0]
    x, w, bias = _int_case(rng, m, c)
    want = torch.from_numpy(_exact(x, w, nbr, bias)).float().to(dtype)       # bf16: one rounding of the exact value
    xd = torch.from_numpy(x).to(dev, dtype)
    wd = torch.from_numpy(w).to(dev, dtype).reshape(c, -1).contiguous()
    bd = torch.from_numpy(bias).float().to(dev)
    nd = torch.from_numpy(nbr).to(dev)
    od = None if order is None else torch.from_numpy(order.astype(np.int32)).to(dev)
    with _env(NEW_PATH):
        plan, counts, rows, slots = ops.halo_plan(nd, od)
    if expect_counts is not None:
        expect_counts(counts.cpu().numpy())
    got = _new(xd, wd, nd, od, plan=plan, bias=bd, out=torch.full((m, c), float("nan"), dtype=dtype, device=dev))
    assert not torch.isnan(got.float()).any()
    assert torch.equal(got.cpu(), want), (got.cpu().float() - want.float()).abs().max().item()
    assert torch.equal(got, _old(xd, wd, nd, od, bias=bd))
    return counts, rows, slots


# ---- sizes: a tile of one site, partial last tiles, more than one tile ----------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("ordered", [False, True], ids=["identity", "row_order"])
def test_sizes_around_the_tile(dev, shape, dtype, c, ordered):
    T, CAP = shape
    for m in (1, T - 1, T, T + 1, 2 * T + 37):
        rng = np.random.default_rng(1000 * m + c)
        order = rng.permutation(m) if ordered else None
        nbr = _uniform_table(rng, m, 0.6)

        def none_overflows(counts, m=m):
            assert len(counts) == -(-m // T) and (counts <= CAP).all()      # m <= 293 rows: every tile is fast
        _check_exact(dev, dtype, nbr, order, c, rng, none_overflows)


# ---- CAP, CAP + 1 and the special tiles, fast and slow tiles in one launch ------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("ordered", [False, True], ids=["identity", "row_order"])
def test_fast_and_slow_tiles_in_one_launch(dev, shape, dtype, c, ordered):
    T, CAP = shape
    rng = np.random.default_rng(77 + c)
    tile_space = _mixed_table(rng, T, CAP)
    m = tile_space.shape[0]
    order = rng.permutation(m) if ordered else None
    nbr = _to_rows(tile_space, order)

    def counts_as_built(counts):
        assert counts[0] == CAP and counts[1] == CAP + 1 and counts[2] == T
        assert (counts[[0, 2, 3, 4, 5]] <= CAP).all()
    counts, rows, slots = _check_exact(dev, dtype, nbr, order, c, rng, counts_as_built)
    # plan invariants of the special tiles
    slots, rows = slots.cpu().numpy(), rows.cpu().numpy()
    assert (slots[:, :, 20].reshape(-1)[:m] == ABSENT).all()                  # the tap nobody has
    assert (slots[2, :, 13] != ABSENT).all() and (np.delete(slots[2], 13, axis=1) == ABSENT).all()
    assert len(set(slots[3, :, 5])) == 1 and rows[3, slots[3, 0, 5]] == 7     # one row shared by the whole tile
    assert (slots.reshape(-1, 27)[m:] == ABSENT).all()                        # sites past m


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [32, 64])
def test_every_tile_overflows(dev, shape, dtype, c):
    """neighbours drawn uniformly from all 5T rows, every tap present: ~5T distinct rows per tile"""
    T, CAP = shape
    rng = np.random.default_rng(5 + c)
    m = 5 * T
    nbr = _uniform_table(rng, m, 1.0)
    order = rng.permutation(m)

    def all_slow(counts):
        assert (counts > CAP).all()
        want = [len(np.unique(nbr[order[t:t + T]])) for t in range(0, m, T)]
        assert counts.tolist() == want
    _check_exact(dev, dtype, nbr, order, c, rng, all_slow)


# ---- epilogues, random floats ----------------------------------------------------------------------------------
def _float_case(dev, dtype, c, T, CAP, seed):
    rng = np.random.default_rng(seed)
    tile_space = _mixed_table(rng, T, CAP)
    m = tile_space.shape[0]
    order = rng.permutation(m)
    nbr = _to_rows(tile_space, order)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, c, generator=g).to(dev, dtype)
    w = (torch.randn(c, 27, c, generator=g) / (27 * c) ** 0.5).to(dev, dtype)
    vec = [torch.randn(c, generator=g).to(dev), (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)]
    res = torch.randn(m, c, generator=g).to(dev, dtype)
    pool = torch.randn(50, c, generator=g).to(dev, dtype)
    ridx = torch.randint(0, 50, (m,), generator=g).int().to(dev)
    return (x, w.reshape(c, -1).contiguous(), torch.from_numpy(nbr).to(dev), torch.from_numpy(order.astype(np.int32)).to(dev),
            vec, res, pool, ridx)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [32, 64])
def test_epilogues_match_the_existing_path_bitwise(dev, shape, dtype, c):
    """The executor calls these convs with a plain bias (Run::block); the entry point takes ptv3_gemm's whole epilogue,
    so every form is held to the existing kernel: none, bias, bias + folded BN + GELU / ReLU, residual, indexed
    residual, and both outputs (out2)."""
    from ptv3_hip import ops
    T, CAP = shape
    x, w, nbr, order, (bias, scale, shift), res, pool, ridx = _float_case(dev, dtype, c, T, CAP, 300 + c)
    with _env(NEW_PATH):
        plan = ops.halo_plan(nbr, order)[0]
    forms = [dict(), dict(bias=bias), dict(bias=bias, bn_scale=scale, bn_shift=shift, act=ops.ACT_GELU),
             dict(bn_scale=scale, bn_shift=shift, act=ops.ACT_RELU), dict(bias=bias, res=res),
             dict(bias=bias, act=ops.ACT_RELU, res=pool, res_index=ridx),
             dict(bias=bias, bn_scale=scale, bn_shift=shift, act=ops.ACT_GELU, res=res, dual=True)]
    for epi in forms:
        new, old = _new(x, w, nbr, order, plan=plan, **epi), _old(x, w, nbr, order, **epi)
        if epi.get("dual"):
            assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1]), sorted(epi)
        else:
            assert torch.equal(new, old), sorted(epi)
    for o in (None,):                                   # and without row_order (a plan of its own)
        assert torch.equal(_new(x, w, nbr, o, bias=bias), _old(x, w, nbr, o, bias=bias))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [32, 64])
def test_random_floats_against_float64(dev, shape, dtype, c):
    """fp32: 1e-4 of the output scale.  bf16: the inputs are exact in float64, the fp32 accumulation stays inside the
    same 1e-4, and the stored output adds one rounding to bf16's 8 significant bits: half an ulp, which is at most
    2^-8 of the value (an ulp of [2^k, 2^(k+1)) is 2^(k-7))."""
    T, CAP = shape
    x, w, nbr, order, (bias, _, _), _, _, _ = _float_case(dev, dtype, c, T, CAP, 900 + c)
    first = _new(x, w, nbr, order, bias=bias)
    second = _new(x, w, nbr, order, bias=bias)
    assert torch.equal(first, second)
    n = nbr.cpu().numpy()
    xp = np.concatenate([x.double().cpu().numpy(), np.zeros((1, c))])
    ref = np.einsum("mdc,odc->mo", xp[np.where(n >= 0, n, len(n))], w.double().cpu().numpy().reshape(c, 27, c))
    ref += bias.double().cpu().numpy()
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(first.double().cpu().numpy() - ref).max())
    tol = (1e-4 if dtype == torch.float32 else 1e-4 + 2.0 ** -8) * scale
    print(f"halo conv c={c} {dtype}: max err {err:.3e}, bound {tol:.3e}")
    assert err < tol


# ---- a real scene ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_scene(dev):
    """4000 occupied voxels of a densely sampled surface (the benchmark's kind of scene), its 27-tap table and its
    z-order, all through ops"""
    from ptv3_hip import ops
    import ptv3_scenes as S
    n = 4000
    grid = torch.from_numpy(S.make_scene(n, 4, None, 4000, "surface")["grid_coord"])
    idx = torch.cat([torch.zeros(n, 1, dtype=torch.int32), grid.int()], 1).contiguous().to(dev)
    nbr, _ = ops.subm_neighbors_blocks(idx, 3)
    depth = int(grid.max()).bit_length()
    code = ops.sfc_encode(grid.to(dev), torch.zeros(n, dtype=torch.int64, device=dev), depth, ["z"])
    order = ops.argsort_codes(code, 3 * depth)[0][0].int().contiguous()
    return nbr, order


def test_real_scene_plan_invariants_and_fast_share(dev, shape, real_scene):
    from ptv3_hip import ops
    T, CAP = shape
    nbr, order = real_scene
    with _env(NEW_PATH):
        _, counts, rows, slots = ops.halo_plan(nbr, order)
    n, o = nbr.cpu().numpy(), order.cpu().numpy()
    counts, rows, slots = counts.cpu().numpy(), rows.cpu().numpy(), slots.cpu().numpy()
    m = len(n)
    assert len(counts) == -(-m // T)
    for t in range(len(counts)):
        tab = n[o[t * T:(t + 1) * T]]                                   # (sites, 27) of this tile
        present = np.unique(tab[tab >= 0])
        assert counts[t] == len(present)                                # counts match a CPU unique
        k = min(counts[t], CAP)
        assert len(set(rows[t, :k])) == k and set(rows[t, :k]) <= set(present)   # every listed row is in the table
        sl = slots[t, :len(tab)].astype(np.int64)
        assert ((sl == ABSENT) == (tab < 0)).all()
        if counts[t] <= CAP:
            assert (rows[t][sl[tab >= 0]] == tab[tab >= 0]).all()       # every present (site, tap) -> slot of its row
        assert (slots[t, len(tab):] == ABSENT).all()
    fast = float((counts <= CAP).mean())
    print(f"real scene: {len(counts)} tiles, distinct rows mean {counts.mean():.0f} max {counts.max()}, fast {fast:.3f}")
    assert fast >= 0.95


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [32, 64])
def test_real_scene_matches_the_existing_path_bitwise(dev, real_scene, dtype, c):
    nbr, order = real_scene
    g = torch.Generator().manual_seed(c)
    x = torch.randn(nbr.shape[0], c, generator=g).to(dev, dtype)
    w = (torch.randn(c, 27 * c, generator=g) / (27 * c) ** 0.5).to(dev, dtype)
    bias = torch.randn(c, generator=g).to(dev)
    assert torch.equal(_new(x, w, nbr, order, bias=bias), _old(x, w, nbr, order, bias=bias))


# ---- the executor ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,points", [(torch.bfloat16, 6000), (torch.float32, 33000)], ids=["bf16", "f32"])
def test_forward_through_the_executor_is_bitwise_unchanged(dev, dtype, points):
    """One eval forward of the fork config: PTV3_CONV_HALO=2 (every single-pass 32 / 64-channel 3^3 conv through the halo
    tile) against PTV3_CONV_HALO=0.  The executor leaves split-K shapes on their slab path whatever the switch says (a
    split changes the summation order), and fp32 splits its 27 x 32-channel K below 32 768 rows: 6000 points in bf16,
    33 000 in fp32 are the smallest scenes whose level-0 convs are single-pass.  The profiler names the kernel, so the
    test sees that it ran."""
    from pointcept.models import build_model
    from ptv3_hip import ops
    from ptv3_hip.configs import FORK_CFG
    import ptv3_scenes as S
    torch.manual_seed(0)
    model = build_model(dict(type="OffsetKeypointPTv3", num_keypoints=6,
                             backbone_conf=dict(type="PT-v3m1", **FORK_CFG))).to(dev).eval()
    model.backbone.compute_dtype = dtype
    data = {k: v.to(dev) for k, v in S.make_batch([points], in_channels=4, extent=None if points < 10000 else 160,
                                                  seed=21).items()}
    preds = {}
    for mode in ("0", "2"):
        with _env({"PTV3_CONV_HALO": mode}):
            ops.profile_enable(True)
            try:
                torch.manual_seed(3)
                with torch.no_grad():
                    preds[mode] = model(data)["pred"].clone()
                torch.cuda.synchronize()
                kernels = ops.profile_collect_kernels()
                ops.profile_collect()
            finally:
                ops.profile_enable(False)
        ran = kernels.get("conv_halo_kernel (sparse conv)", dict(launches=0))["launches"]
        assert (ran > 0) == (mode == "2"), (mode, sorted(kernels))
    assert torch.isfinite(preds["2"].float()).all()
    assert torch.equal(preds["0"], preds["2"])
