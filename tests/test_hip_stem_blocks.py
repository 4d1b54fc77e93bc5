"""GPU: the k^3 stem convolution straight from the block table (ptv3_stem_conv_blocks, csrc/conv_stem.hip).

Every case expects the bytes of ops.gemm(x, w, nbr=subm_neighbors_blocks(idx, k), kvol=k^3, ...) - the path the module
model keeps - in fp32 (cin = 4) and bf16 (cin padded to 8), cout = 32.  The output tensor is pre-filled with NaN, so a
row the kernel skips (a duplicate coordinate, a row past a tile's end) shows.  Sizes sit around the 64-site tile; site sets
are the ones in which a tap can go wrong: all taps present, a plane, a lone site, the coordinate bounds, duplicate
coordinates, equal coordinates in three scenes.  ptv3_gemm splits K at every size up to 24 576 rows and the kernel
must reproduce the slab sums; one case past that size runs the single pass."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

COUT = 32
DTYPES = {"fp32": (torch.float32, 4), "bf16": (torch.bfloat16, 8)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _with_batch(xyz, batch=0):
    xyz = np.asarray(xyz, dtype=np.int64).reshape(-1, 3)
    return torch.from_numpy(np.concatenate([np.full((len(xyz), 1), batch), xyz], 1).astype(np.int32))


def _random_sites(n, seed, origin=3):
    """n distinct voxels of the smallest cube with twice as many cells, in random order: most taps have a neighbour"""
    extent = max(2, int(np.ceil((2 * n) ** (1 / 3))))
    flat = np.random.default_rng(seed).choice(extent ** 3, size=n, replace=False)
    return _with_batch(np.stack([flat // (extent * extent), (flat // extent) % extent, flat % extent], 1) + origin)


def _cube():
    g = np.arange(12)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + 6
    return _with_batch(xyz[np.random.default_rng(1).permutation(len(xyz))])


def _plane():
    g = np.arange(20)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    xyz = np.concatenate([xy + 1, np.full((len(xy), 1), 7)], 1)
    return _with_batch(xyz[np.random.default_rng(2).permutation(len(xyz))])


def _bounds():
    m = 65535
    return _with_batch([(0, 0, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1), (0, 0, 1), (m, m, m), (m - 1, m, m), (m, m - 1, m - 1),
                        (m - 1, m - 1, m - 1), (m, 0, 1), (0, m, m - 1), (1, m - 1, 0)])


def _duplicate_pairs():
    base = _random_sites(90, 3)
    rows = torch.cat([base, base[:45]])
    return rows[torch.from_numpy(np.random.default_rng(4).permutation(len(rows)))]


def _three_scenes():
    a = _random_sites(70, 5)
    return torch.cat([torch.cat([torch.full((70, 1), b, dtype=torch.int32), a[:, 1:]], 1) for b in (0, 1, 2)])


SITE_SETS = {
    "cube_12": _cube,
    "plane": _plane,
    "lone": lambda: _with_batch([(9, 10, 11)]),
    "bounds": _bounds,
    "duplicate_pairs": _duplicate_pairs,
    "three_scenes": _three_scenes,
}


def _operands(idx, dtype_name, k, seed, dev):
    dtype, cin = DTYPES[dtype_name]
    n = idx.shape[0]
    gen = torch.Generator().manual_seed(seed)
    x = torch.zeros(n, cin)
    x[:, :4] = torch.randn(n, 4, generator=gen)
    w = torch.randn(COUT, k ** 3, cin, generator=gen) * 0.1
    scale = torch.rand(COUT, generator=gen) + 0.5
    shift = torch.randn(COUT, generator=gen) * 0.1
    order = torch.randperm(n, generator=gen).to(torch.int32)
    return (x.to(dtype).to(dev), w.to(dtype).to(dev).contiguous(), scale.to(dev), shift.to(dev), order.to(dev))


def _check(idx, dtype_name, k, epilogue, ordered, dev, seed=0):
    """stem_conv_blocks against gemm over the block table's neighbour table: the same bytes, every row written"""
    from ptv3_hip import ops
    idx = idx.contiguous().to(dev)
    x, w, scale, shift, order = _operands(idx, dtype_name, k, seed, dev)
    kw = dict(row_order=order if ordered else None)
    if epilogue:
        kw.update(bn_scale=scale, bn_shift=shift, act=ops.ACT_GELU)
    nbr, table = ops.subm_neighbors_blocks(idx, k)
    ref = ops.gemm(x, w, nbr=nbr, kvol=k ** 3, **kw)
    out = torch.full_like(ref, float("nan"))
    ops.stem_conv_blocks(x, w, idx, table, ksize=k, out=out, **kw)
    assert not torch.isnan(out.float()).any()
    assert torch.equal(out.view(torch.uint8), ref.view(torch.uint8))
    return nbr


@pytest.mark.parametrize("ordered", [False, True], ids=["natural", "row_order"])
@pytest.mark.parametrize("epilogue", [False, True], ids=["plain", "bn_gelu"])
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 4097])
def test_sizes_around_the_tile(dev, n, dtype_name, epilogue, ordered):
    _check(_random_sites(n, 10 + n), dtype_name, 5, epilogue, ordered, dev, seed=n)


@pytest.mark.parametrize("epilogue,ordered", [(False, False), (True, True), (True, False), (False, True)],
                         ids=["plain-natural", "bn_gelu-row_order", "bn_gelu-natural", "plain-row_order"])
@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("sites", list(SITE_SETS))
def test_site_sets(dev, sites, dtype_name, epilogue, ordered):
    idx = SITE_SETS[sites]()
    nbr = _check(idx, dtype_name, 5, epilogue, ordered, dev, seed=7).cpu()
    n = idx.shape[0]
    present = (nbr >= 0).sum(1)
    # the reference table has the property the set was built for
    if sites == "cube_12":
        assert (present == 125).sum().item() == 8 ** 3
    elif sites == "plane":
        assert present.max().item() == 25
    elif sites == "lone":
        assert nbr[0].tolist() == [-1] * 62 + [0] + [-1] * 62
    elif sites == "bounds":
        assert present.max().item() < 27
    elif sites == "duplicate_pairs":
        keys = [tuple(r) for r in idx.tolist()]
        first = {}
        for i, key in enumerate(keys):
            first.setdefault(key, i)
        others = torch.cat([nbr[:, :62], nbr[:, 63:]], 1)
        assert set(others[others >= 0].tolist()) <= set(first.values())     # the smallest row is the neighbour
        assert torch.equal(nbr[:, 62], torch.arange(n, dtype=torch.int32))   # and every duplicate is its own centre
    elif sites == "three_scenes":
        scene = torch.arange(n).div(70, rounding_mode="floor")
        hit = nbr >= 0
        assert torch.equal(nbr.clamp(min=0).div(70, rounding_mode="floor")[hit], scene[:, None].expand_as(nbr)[hit])


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_k3_against_the_27_tap_table(dev, dtype_name):
    _check(_random_sites(130, 21), dtype_name, 3, True, True, dev, seed=3)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_single_pass_beside_the_split_sizes(dev, dtype_name):
    """ptv3_gemm sums four K slabs up to 24 576 rows at this shape and runs one pass above: both forms are covered"""
    from ptv3_hip import ops
    dtype, cin = DTYPES[dtype_name]
    assert ops.gemm_splits(4097, cin, COUT, 125, dtype) > 1
    n = 24700
    assert ops.gemm_splits(n, cin, COUT, 125, dtype) == 1
    _check(_random_sites(n, 22), dtype_name, 5, True, False, dev, seed=5)
