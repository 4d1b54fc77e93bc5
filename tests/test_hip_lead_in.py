"""The serial lead-in of a forward, up to the stem conv: the radix sort with batched counter / key / value loads (and
its executor form that also writes row_order), the one-pass coordinate maximum that is its own read-back, the table build whose zero fill rides on the site conversion, and the executor's new
order on its geometry stream.  Everything here is integers: results are compared exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from make_golden_cfg import ORDERS, TINY_CFG  # noqa: E402

TILE = 2048          # keys per radix workgroup (RS_TILE)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _scan_batch():
    from ptv3_hip.lib import lib
    return int(lib.ptv3_argsort_scan_batch())


def _sort_sizes():
    # B = counters a scatter workgroup loads per round trip: one trip, exactly one, one and a slot, two and a bit; the
    # level-0 size of the benchmark scene (49 blocks); the last size with the fused scan and the first without it
    B = 32
    return [1, TILE - 1, TILE, TILE + 1, B * TILE, B * TILE + 1, (B + 1) * TILE + 5, 49 * TILE - 3, 128 * TILE,
            128 * TILE + 1]


def test_sort_sizes_follow_the_kernel_batch():
    assert _scan_batch() == 32, "the sizes of _sort_sizes() are written for a batch of 32 counters"


def _key_sets(k, n, end_bit, gen):
    """(name, (k, n) int64 keys with every set bit below end_bit)"""
    top = 1 << end_bit
    pool = torch.randint(0, top, (37,), generator=gen, dtype=torch.int64)
    dup = pool[torch.randint(0, 37, (k, n), generator=gen)]                      # 37 distinct keys: heavy duplication
    rnd = torch.randint(0, top, (k, n), generator=gen, dtype=torch.int64)
    same = (rnd & ~torch.tensor(255, dtype=torch.int64)) | (0xA5 & (top - 1))    # the first sorted digit equal everywhere
    hole = torch.where((rnd & 255) == 7, rnd ^ 15, rnd)                          # digit value 7 never occurs (7 -> 8)
    return [("duplicates", dup), ("equal digit", same), ("absent digit", hole)]


def _reference(code):
    order = torch.sort(code, dim=1, stable=True).indices
    inverse = torch.empty_like(order)
    inverse.scatter_(1, order, torch.arange(code.shape[1], device=code.device).expand_as(order).contiguous())
    return order, inverse


@pytest.mark.parametrize("n", _sort_sizes())
def test_radix_sort_matches_stable_torch_sort(dev, n):
    """ops.argsort_codes and the executor's variant (row_order beside order and inverse) against
    torch.sort(stable=True), exactly: k in {1, 4}, end_bit in {8, 9, 24, 40}, three key sets."""
    from ptv3_hip import ops
    gen = torch.Generator().manual_seed(1000 + n % 9973)
    for k in (1, 4):
        for end_bit in (8, 9, 24, 40):
            for name, keys in _key_sets(k, n, end_bit, gen):
                code = keys.to(dev)
                ref_order, ref_inverse = _reference(code)
                what = (k, end_bit, name)
                order, inverse = ops.argsort_codes(code, end_bit)
                assert torch.equal(order, ref_order), what
                assert torch.equal(inverse, ref_inverse), what
                order, inverse, row_order = ops.argsort_codes_rows(code, end_bit)
                assert torch.equal(order, ref_order), what
                assert torch.equal(inverse, ref_inverse), what
                assert row_order.dtype == torch.int32 and torch.equal(row_order.long(), ref_order[0]), what


@pytest.mark.parametrize("n", [1, 2049, 49 * TILE - 3])
def test_sort_of_curve_codes_with_row_order(dev, n):
    """The executor's level-0 call: codes of k curves from coordinates with many duplicates, sorted with row_order."""
    from ptv3_hip import ops
    gen = torch.Generator().manual_seed(77 + n)
    depth = 6
    grid = torch.randint(0, 1 << depth, (n, 3), generator=gen).to(dev)
    batch = torch.sort(torch.randint(0, 3, (n,), generator=gen)).values.to(dev)
    for orders in (ORDERS[:1], ORDERS):
        code = ops.sfc_encode(grid, batch, depth, orders)
        ref_order, ref_inverse = _reference(code)
        order, inverse, row_order = ops.argsort_codes_rows(code, 3 * depth + 2)
        assert torch.equal(order, ref_order) and torch.equal(inverse, ref_inverse)
        assert torch.equal(row_order.long(), ref_order[0])


@pytest.mark.parametrize("n", [1, 255, 8 * 256 + 1, 70001])
@pytest.mark.parametrize("coord_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_coordinate_maximum(dev, n, coord_dtype):
    """One pass, a fixed batch of loads per thread: the maximum at the first element, at the last one and inside the
    final partial batch (a thread's eight values are 256 apart; a workgroup takes 2048), values on both sides of a
    power of two.  (The executor's depth = bit_length(max + 1), structure.py:73, is compared with the module path's in
    test_executor_order_matches_the_module_path and at 17 in test_depth_17_is_refused_and_the_next_call_is_right.)"""
    from ptv3_hip import ops
    n3 = 3 * n
    last_batch = (n3 - 1) // 2048 * 2048
    places = sorted({0, n3 - 1, (last_batch + n3 - 1) // 2})
    gen = torch.Generator().manual_seed(5 + n)
    state = torch.zeros(2, dtype=torch.int32, device=dev)      # reused: the kernel leaves it zero for the next launch
    for d in (1, 7, 15):
        for top in (0, (1 << d) - 1, 1 << d):
            for at in places:
                flat = torch.randint(0, top + 1, (n3,), generator=gen)
                flat[flat == top] = max(top - 1, 0)             # the maximum occurs once, where it is placed
                flat[at] = top
                grid = flat.view(n, 3).to(coord_dtype).to(dev)
                assert int(ops.coord_max(grid, state).item()) == top, (d, top, at)
    assert state.tolist() == [0, 0]


def _tiny_model(dev):
    from pointcept.models import build_model
    torch.manual_seed(3)
    return build_model(dict(type="OffsetKeypointPTv3", num_keypoints=6, hidden_dim=32,
                            backbone_conf=dict(type="PT-v3m1", **TINY_CFG))).to(dev).eval()


def _scenes(dev, sizes_list, seed):
    import ptv3_scenes as S
    return [{k: v.to(dev) for k, v in S.make_batch(sz, in_channels=4, extent=64, seed=seed + i).items()}
            for i, sz in enumerate(sizes_list)]


def _module_path(model, scene):
    model.backbone.use_engine = False
    torch.manual_seed(9)
    with torch.no_grad():
        pred = model(scene)["pred"].clone()
        torch.manual_seed(9)
        pt = model.backbone(scene)
    out = dict(pred=pred, feat=pt.feat.clone(), code=pt.serialized_code.clone(), order=pt.serialized_order.clone(),
               inverse=pt.serialized_inverse.clone(), depth=int(pt.serialized_depth))
    torch.cuda.synchronize()
    model.backbone.use_engine = True
    return out


@pytest.mark.parametrize("resident,overlap", [(False, False), (True, False), (True, True)],
                         ids=["stream-ordered", "resident", "overlap"])
def test_executor_order_matches_the_module_path(dev, resident, overlap):
    """fp32, two scenes per call, three consecutive calls with different point counts (both geometry arenas are used,
    and the second is reused): prediction, features, codes, orders and inverses are bitwise the module path's.  The
    executor queues the sites, the block table and the 5^3 table before it has read depth and offsets back, encodes
    and sorts afterwards, and takes row_order from the sort."""
    model = _tiny_model(dev)
    scenes = _scenes(dev, [[4000, 2500], [1500, 900], [5000, 1000]], seed=60)
    want = [_module_path(model, sc) for sc in scenes]
    model.backbone.inputs_resident, model.backbone.overlap_calls = resident, overlap
    preds, points = [], []
    for sc in scenes:
        torch.manual_seed(9)
        with torch.no_grad():
            preds.append(model(sc)["pred"])
    for sc in scenes:
        torch.manual_seed(9)
        with torch.no_grad():
            pt = model.backbone(sc)
        points.append(dict(feat=pt.feat.clone(), code=pt.serialized_code.clone(), order=pt.serialized_order.clone(),
                           inverse=pt.serialized_inverse.clone(), depth=int(pt.serialized_depth)))
    torch.cuda.synchronize()
    for i, w in enumerate(want):
        assert torch.equal(preds[i], w["pred"]), i
        assert points[i]["depth"] == w["depth"], i
        for key in ("feat", "code", "order", "inverse"):
            assert torch.equal(points[i][key], w[key]), (i, key)


def test_depth_17_is_refused_and_the_next_call_is_right(dev):
    """A coordinate of 65 535 makes depth 17: the executor returns its error with the depth-independent kernels of
    level 0 already queued (they stay inside the call's arena for any int32 coordinates); the valid call straight
    after it gives the module path's result."""
    model = _tiny_model(dev)
    good, other = _scenes(dev, [[3000, 2000], [2500, 700]], seed=80)
    want = _module_path(model, good)
    bad = dict(other)
    bad["grid_coord"] = other["grid_coord"].clone()
    bad["grid_coord"][-1, 2] = 65535
    for resident in (False, True):
        model.backbone.inputs_resident = resident
        with pytest.raises(RuntimeError, match=r"serialization depth 17 outside \[1,16\]"):
            torch.manual_seed(9)
            with torch.no_grad():
                model(bad)
        torch.manual_seed(9)
        with torch.no_grad():
            got = model(good)["pred"]
        torch.cuda.synchronize()
        assert torch.equal(got, want["pred"]), resident


@pytest.mark.parametrize("n,duplicates", [(1, False), (300, False), (300, True), (5000, False)])
@pytest.mark.parametrize("coord_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
def test_table_with_folded_zero_fill_gives_the_same_neighbours(dev, n, duplicates, coord_dtype):
    """ptv3_subm_sites (site conversion + zero fill in one launch) + ptv3_subm_build_block_table_zeroed against
    ptv3_subm_build_block_table: the 3^3 and 5^3 tables are bitwise equal, so are the sites and the int64 coordinates.
    The table memory is filled with ones first: a fill that missed a byte would leave a slot that looks occupied."""
    from ptv3_hip import ops
    gen = torch.Generator().manual_seed(11 + n)
    cells = torch.randperm(24 ** 3, generator=gen)[:n]
    grid = torch.stack([cells // 576, (cells // 24) % 24, cells % 24], dim=1)
    if duplicates:
        grid[n // 2:n // 2 + 20] = grid[:20]                     # twenty coordinates occur twice
    batch = torch.sort(torch.randint(0, 2, (n,), generator=gen)).values
    if duplicates:
        batch[n // 2:n // 2 + 20] = batch[:20]
    grid_d, batch_d = grid.to(coord_dtype).to(dev), batch.to(dev)
    ref_idx = torch.cat([batch_d[:, None], grid_d.long()], dim=1).int().contiguous()
    for rep in range(2):                                          # the second round reuses freed (dirty) table memory
        dirty = torch.full((int(ops.lib.ptv3_subm_block_table_bytes(n)),), 0xFF, dtype=torch.uint8, device=dev)
        del dirty
        indices, grid64, table = ops.subm_sites_table(batch_d, grid_d)
        assert torch.equal(indices, ref_idx)
        assert torch.equal(grid64, grid_d.long())
        for ksize in (3, 5):
            want, _ = ops.subm_neighbors_blocks(ref_idx, ksize)
            got, _ = ops.subm_neighbors_blocks(indices, ksize, table=table)
            assert torch.equal(got, want), (ksize, rep)
