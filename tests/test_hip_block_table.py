"""GPU: neighbour tables from the 4x4x4 block table (ptv3_subm_build_block_table + ptv3_subm_neighbors_blocks).

Whole tables, bitwise (torch.equal), against two independent references:
  * a Python dictionary over the sites in which the first (smallest) row of a coordinate wins and the centre tap is
    the row itself,
  * the full-probing kernel of the per-voxel table (ops.subm_neighbors under PTV3_NBR_SYMMETRIC=0).
The cases are the smallest that can still go wrong: block borders, the coordinate bounds, a full block (mask bit 63,
rank 63), batch ids, duplicate coordinates, dense / sparse / near-full tables; each at k = 1, 3, 5, 7."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = (1, 3, 5, 7)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _sites(rows):
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)


def _random_sites(n, extent, seed, batch=0, origin=0):
    """n distinct voxels of an extent^3 cube, in random order"""
    rng = np.random.default_rng(seed)
    flat = rng.choice(extent ** 3, size=n, replace=False)
    xyz = np.stack([flat // (extent * extent), (flat // extent) % extent, flat % extent], 1) + origin
    return torch.from_numpy(np.concatenate([np.full((n, 1), batch), xyz], 1).astype(np.int32))


def _full_blocks(origins, seed):
    rows = [(0, ox + a, oy + b, oz + c) for ox, oy, oz in origins for a in range(4) for b in range(4) for c in range(4)]
    perm = np.random.default_rng(seed).permutation(len(rows))
    return _sites(rows)[torch.from_numpy(perm)]


def _pair(axis):
    a, b = [5, 5, 5], [5, 5, 5]
    a[axis], b[axis] = 3, 4      # the neighbour sits in the next block
    return _sites([[0] + a, [0] + b])


def _upper():
    m = 65535
    return _sites([(0, m, 10, 10), (0, m - 1, 10, 10), (0, 10, m, 10), (0, 10, m - 2, 10), (0, 10, 10, m),
                   (0, 10, 11, m - 1), (0, m, m, m), (0, m - 1, m - 1, m - 1)])


def _two_batches():
    a = _random_sites(400, 12, 3, batch=0)
    b = a.clone()
    b[:, 0] = 1
    return torch.cat([a, b[torch.from_numpy(np.random.default_rng(4).permutation(400))]])


def _duplicates():
    base = _random_sites(200, 10, 5, origin=2)
    rng = np.random.default_rng(6)
    rows = torch.cat([base, base[torch.from_numpy(rng.integers(0, 200, 100))]])
    return rows[torch.from_numpy(rng.permutation(300))]


def _duplicated_block():
    blk = _full_blocks([(4, 8, 12)], 7)
    rows = torch.cat([blk, blk])
    return rows[torch.from_numpy(np.random.default_rng(8).permutation(128))]


def _one_site_per_block():
    """5000 sites in 5000 distinct blocks of a 20^3 lattice of blocks: the block count equals n (the fullest table the
    layout allows), with neighbours across block borders"""
    rng = np.random.default_rng(9)
    blocks = rng.choice(20 ** 3, size=5000, replace=False)
    xyz = np.stack([blocks // 400, (blocks // 20) % 20, blocks % 20], 1) * 4 + rng.integers(0, 4, (5000, 3))
    return torch.from_numpy(np.concatenate([np.zeros((5000, 1)), xyz], 1).astype(np.int32))


CASES = {
    "n0": lambda: torch.zeros(0, 4, dtype=torch.int32),
    "n1": lambda: _sites([(0, 5, 6, 7)]),
    "pair_x": lambda: _pair(0),
    "pair_y": lambda: _pair(1),
    "pair_z": lambda: _pair(2),
    "origin": lambda: _sites([(0, 0, 0, 0), (0, 1, 0, 0), (0, 0, 2, 0), (0, 0, 0, 3), (0, 1, 1, 1)]),
    "upper": _upper,
    "full_block": lambda: _full_blocks([(8, 8, 8)], 1),
    "two_full_blocks": lambda: _full_blocks([(8, 8, 8), (8, 12, 8)], 2),
    "two_batches": _two_batches,
    "duplicates": _duplicates,
    "duplicated_block": _duplicated_block,
    "dense_3000_in_24": lambda: _random_sites(3000, 24, 10),
    "sparse_2000_in_200": lambda: _random_sites(2000, 200, 11),
    "one_site_per_block_5000": _one_site_per_block,
}
_IDX = {}


def _case(name):
    if name not in _IDX:
        _IDX[name] = CASES[name]().contiguous()
    return _IDX[name]


def _encode(b, x, y, z):
    return ((b * 65536 + x) * 65536 + y) * 65536 + z


_DICT = {}


def dictionary_table(case, k):
    """the dictionary reference of a case, computed once and left unchanged"""
    if (case, k) not in _DICT:
        _DICT[case, k] = _dictionary_table(_case(case), k)
    return _DICT[case, k]


def _dictionary_table(idx, k):
    """nbr (n, k^3) from a dictionary coordinate -> first row; the centre tap is the row itself"""
    a = idx.numpy().astype(np.int64)
    n, kvol, h = len(a), k ** 3, k // 2
    first = {}
    for i, key in enumerate(_encode(a[:, 0], a[:, 1], a[:, 2], a[:, 3]).tolist()):
        first.setdefault(key, i)
    d = np.arange(kvol)
    off = np.stack([d // (k * k) - h, (d // k) % k - h, d % k - h], 1)            # (kvol, 3)
    q = a[:, None, 1:] + off[None]                                                # (n, kvol, 3)
    inside = ((q >= 0) & (q < 65536)).all(-1)
    keys = _encode(a[:, None, 0], q[..., 0], q[..., 1], q[..., 2])
    out = np.array([first.get(key, -1) for key in keys.reshape(-1).tolist()], dtype=np.int32).reshape(n, kvol)
    out[~inside] = -1
    out[:, kvol // 2] = np.arange(n)
    return torch.from_numpy(out)


def full_probing_table(idx, k):
    from ptv3_hip import ops
    os.environ["PTV3_NBR_SYMMETRIC"] = "0"
    try:
        full, _ = ops.subm_neighbors(idx, k)
    finally:
        os.environ.pop("PTV3_NBR_SYMMETRIC", None)
    return full


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", list(CASES))
def test_block_table_equals_dictionary_and_full_probing(dev, case, k):
    from ptv3_hip import ops
    idx = _case(case)
    nbr, _ = ops.subm_neighbors_blocks(idx.to(dev), k)
    assert nbr.shape == (idx.shape[0], k ** 3) and nbr.dtype == torch.int32
    assert torch.equal(nbr.cpu(), dictionary_table(case, k))
    assert torch.equal(nbr, full_probing_table(idx.to(dev), k))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", ["duplicates", "duplicated_block"])
def test_duplicate_coordinates_give_the_same_table_twice(dev, case, k):
    """the smallest row of a coordinate wins whatever order the atomics land in: two builds, identical tables"""
    from ptv3_hip import ops
    idx = _case(case).to(dev)
    first, _ = ops.subm_neighbors_blocks(idx, k)
    second, _ = ops.subm_neighbors_blocks(idx, k)
    assert torch.equal(first, second)


def test_one_table_serves_k5_then_k3(dev):
    from ptv3_hip import ops
    idx = _case("dense_3000_in_24")
    nbr5, table = ops.subm_neighbors_blocks(idx.to(dev), 5)
    nbr3, same = ops.subm_neighbors_blocks(idx.to(dev), 3, table)
    assert same is table
    assert torch.equal(nbr5.cpu(), dictionary_table("dense_3000_in_24", 5))
    assert torch.equal(nbr3.cpu(), dictionary_table("dense_3000_in_24", 3))


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", ["n1", "upper", "duplicates", "sparse_2000_in_200", "one_site_per_block_5000"])
def test_every_entry_is_written_and_no_table_filler_leaks(dev, case, k):
    """nbr starts as a sentinel and none may survive (there is no pre-fill to rely on); every entry is -1 or a row,
    never a slot index or the table's filler"""
    from ptv3_hip import ops
    from ptv3_hip.lib import lib
    idx = _case(case).to(dev)
    n = idx.shape[0]
    _, table = ops.subm_neighbors_blocks(idx, 1)
    sentinel = -123456789
    nbr = torch.full((n, k ** 3), sentinel, dtype=torch.int32, device=dev)
    lib.check(lib.ptv3_subm_neighbors_blocks(idx.data_ptr(), n, table.data_ptr(), table.numel(), k, nbr.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "ptv3_subm_neighbors_blocks")
    assert not (nbr == sentinel).any()
    assert ((nbr >= -1) & (nbr < n)).all()
    assert torch.equal(nbr.cpu(), dictionary_table(case, k))
