"""GPU parity of the serialized pooling family, kernel by kernel: ptv3_pool_segments, ptv3_pool_reduce (feature half
and geometry half), ptv3_pool_max_bwd and ptv3_segment_sum against the float64 restatement of oracle/pooling.py
(itself held to torch.unique / segment_reduce / scatter_reduce by tests/test_pooling_reference_cpu.py).

Inputs are built directly (oracle.pooling.synth_codes): sorted keys with prescribed run lengths behind a random
permutation, the scene id in the top bits.  Integer outputs and selections (max, arg-max routing) are compared bit
for bit; sums, means and the BN + activation epilogue against bounds derived next to each check.  NaN inputs are
out of scope: the kernels' fmaxf drops a NaN where torch's amax keeps it."""
import functools
import math
import time

import numpy as np
import pytest
import torch

from oracle import pooling as P

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4        # the project's fp32 parity budget (BASELINE.json)
DTYPES = [torch.float32, torch.bfloat16]
NOUTS = (1, 3, 63, 257, 2001)   # none but 1 is a multiple of pool_feat_kernel's rows per workgroup (4 ... 256)
WIDTHS = (4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 256, 260, 512)   # LPR 1 ... 64; idle lanes (12), loops (260, 512)
TILE = 1024            # PS_TILE of csrc/pool.hip


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _np64(t):
    return t.detach().float().cpu().double().numpy()


# ------------------------------------------------------------------------------------------------
# A. pool_segments
# ------------------------------------------------------------------------------------------------
def _mixed(n, rng, hi=9):
    """run lengths 1 ... hi-1 summing to n exactly"""
    lens = rng.integers(1, hi, size=n)
    lens = lens[: int((lens.cumsum() <= n).sum())]
    rest = n - int(lens.sum())
    return np.concatenate([lens, [rest]]) if rest else lens


def _runs(shape, n, rng):
    if shape == "equal":
        return np.array([n])
    if shape == "distinct":
        return np.ones(n, dtype=np.int64)
    return _mixed(n, rng)


def _check_segments(dev, run_len, shift, rng, scene_of_run=None, num_scenes=0, twin=None):
    from ptv3_hip import ops
    code0, order0, batch = P.synth_codes(run_len, shift, rng, scene_of_run, twin)
    n = code0.size
    ref = P.pool_segments(code0, order0, shift, batch, num_scenes)
    assert ref[2] == len(run_len)
    code_d, order_d = _t(code0, dev), _t(order0, dev)
    cluster, seg_start, n_out = ops.pool_segments(code_d, order_d, shift)
    forms = [(cluster, seg_start, n_out)]
    if batch is not None:
        got = ops.pool_segments(code_d, order_d, shift, _t(batch, dev), num_scenes)
        forms.append(got[:3])
        assert got[4] == ref[3].tolist(), f"pooled offset (host) {got[4]} vs {ref[3].tolist()}"
        assert got[3].dtype == torch.int64 and np.array_equal(got[3].cpu().numpy(), ref[3])
    for cluster, seg_start, n_out in forms:
        assert n_out == ref[2]
        assert cluster.dtype == torch.int64 and np.array_equal(cluster.cpu().numpy(), ref[0])
        assert seg_start.dtype == torch.int32 and seg_start.shape[0] == n_out + 1
        assert int(seg_start[-1]) == n
        assert np.array_equal(seg_start.cpu().numpy(), ref[1])
    return code0, order0


@pytest.mark.parametrize("shape", ["equal", "distinct", "mixed"])
@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 4097, 20011])
def test_pool_segments_sizes_and_run_shapes(dev, n, shape):
    for shift in (0, 3, 6, 9):
        rng = np.random.default_rng(n * 16 + shift)
        run_len = _runs(shape, n, rng)
        _check_segments(dev, run_len, shift, rng)
        _check_segments(dev, run_len, shift, rng, np.zeros(len(run_len), dtype=np.int64), 1)


@pytest.mark.parametrize("shift", [0, 3, 6, 9])
def test_pool_segments_run_spanning_whole_tiles(dev, shift):
    """a run of 3000 points from position 500: tiles 1 and 2 hold no run start (block sums of zero)"""
    rng = np.random.default_rng(shift)
    run_len = np.concatenate([np.ones(500, dtype=np.int64), [3000], _mixed(2500, rng)])
    assert run_len[:500].sum() == 500 and 500 + 3000 >= 3 * TILE
    _check_segments(dev, run_len, shift, rng)
    _check_segments(dev, run_len, shift, rng, np.repeat([0, 1], [400, len(run_len) - 400]), 2)


@pytest.mark.parametrize("shift", [0, 3, 6, 9])
def test_pool_segments_run_boundary_on_tile_boundary(dev, shift):
    rng = np.random.default_rng(100 + shift)
    run_len = np.concatenate([_mixed(TILE, rng), _mixed(4097 - TILE, rng)])
    assert TILE in np.cumsum(run_len).tolist()        # a run starts exactly at position 1024
    _check_segments(dev, run_len, shift, rng)


def _scene_split(run_len, scenes, rng):
    """contiguous scenes over the runs.  scenes >= 2: scenes 0 and 1 are twins (their last / first key differ in
    the scene bits only).  scenes >= 5: scene 2 is a single point."""
    run_len = run_len.copy()
    R = len(run_len)
    cuts = np.sort(rng.choice(np.arange(10, R - 10), size=scenes - 1, replace=False)) if scenes > 1 else np.array([], int)
    twin = None
    if scenes >= 5:
        cuts[2] = cuts[1] + 1
        run_len[cuts[1]] = 1
        assert cuts[3] > cuts[2]
    if scenes >= 2:
        run_len[cuts[0] - 1] = run_len[cuts[0]] = 1
        twin = 0
    scene_of_run = np.searchsorted(cuts, np.arange(R), side="right")
    return run_len, scene_of_run, twin


@pytest.mark.parametrize("scenes", [1, 2, 5, 64])
@pytest.mark.parametrize("shift", [0, 3, 6, 9])
def test_pool_segments_batched(dev, scenes, shift):
    rng = np.random.default_rng(scenes * 16 + shift)
    run_len, scene_of_run, twin = _scene_split(_mixed(20011, rng), scenes, rng)
    assert scene_of_run.max() == scenes - 1
    code0, order0 = _check_segments(dev, run_len, shift, rng, scene_of_run, scenes, twin)
    if twin is not None:
        keys = code0[order0]
        e = int(run_len[scene_of_run == 0].sum())
        assert keys[e - 1] ^ keys[e] == 1 << P.BATCH_SHIFT
    if scenes >= 5:
        assert run_len[scene_of_run == 2].tolist() == [1]


@pytest.mark.parametrize("present", [(0, 2, 3), (0, 1, 2), (1, 2, 3)], ids=["scene1_empty", "last_empty", "first_empty"])
def test_pool_segments_empty_scenes(dev, present):
    """A scene without points: its pooled offset repeats its predecessor (0 when it leads) and n_out is the true
    count.  The kernel writes an entry from the scene's last point only; ops.pool_segments fills the rest."""
    rng = np.random.default_rng(sum(present))
    run_len = _mixed(4097, rng)
    scene_of_run = np.sort(rng.choice(present, size=len(run_len)))
    assert set(scene_of_run.tolist()) == set(present)
    _check_segments(dev, run_len, 3, rng, scene_of_run, 4)


def test_pool_segments_scan_carry(dev):
    """1026 tiles: pool_block_scan_kernel takes a second pass of 1024 block sums and must carry the first's total"""
    rng = np.random.default_rng(5)
    n = 1_050_000
    run_len = _mixed(n, rng, hi=5)
    assert -(-n // TILE) == 1026
    cuts = (len(run_len) // 3, 2 * len(run_len) // 3)
    scene_of_run = np.searchsorted(cuts, np.arange(len(run_len)), side="right")
    t0 = time.perf_counter()
    _check_segments(dev, run_len, 3, rng, scene_of_run, 3)
    print(f"scan carry: n {n}, n_out {len(run_len)}, reference + device + compare {time.perf_counter() - t0:.2f} s")


# ------------------------------------------------------------------------------------------------
# shared segment layouts of B ... E: lengths 1 ... 8 mixed plus one segment of 700 members
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layout(n_out):
    rng = np.random.default_rng(1000 + n_out)
    seg_len = rng.integers(1, 9, size=n_out)
    seg_len[n_out // 2] = 700
    n = int(seg_len.sum())
    order0 = rng.permutation(n).astype(np.int64)
    cluster = np.empty(n, dtype=np.int64)
    cluster[order0] = np.repeat(np.arange(n_out), seg_len)
    base = rng.standard_normal((n, 512)).astype(np.float32)       # finite; the widths take column slices of it
    minus_inf = rng.random((n, 512)) < 0.03
    minus_inf[order0[: seg_len[0]]] = n_out > 1                   # segment 0 holds -inf only: its max is -inf
    return dict(n=n, n_out=n_out, seg_len=seg_len, seg_start=P.starts_of(seg_len), order0=order0, cluster=cluster,
                base=base, minus_inf=minus_inf)


def _feat(L, c, dtype, with_inf):
    f = torch.from_numpy(L["base"][:, :c].copy())
    if with_inf:
        f[torch.from_numpy(L["minus_inf"][:, :c].copy())] = -math.inf
    return f.to(dtype)


def _geometry(n, k, rng, coord_kind="unit"):
    coord = rng.uniform(-1, 1, size=(n, 3)) if coord_kind == "unit" else 1000.0 + 10.0 * rng.uniform(-1, 1, size=(n, 3))
    return (coord.astype(np.float32), rng.integers(0, 1 << 16, size=(n, 3)), rng.integers(0, 7, size=n),
            rng.integers(0, 1 << 45, size=(k, n)))


# ------------------------------------------------------------------------------------------------
# B. pool_reduce, feature half
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", WIDTHS)
def test_pool_max_every_width_bit_for_bit(dev, c, dtype):
    """max is a selection: no tolerance, in either dtype.  -inf is an ordinary member."""
    from ptv3_hip import ops
    for n_out in NOUTS:
        L = _layout(n_out)
        feat = _feat(L, c, dtype, with_inf=True)
        ref = torch.full((n_out, c), -math.inf).scatter_reduce(
            0, torch.from_numpy(L["cluster"])[:, None].expand(-1, c), feat.float(), "amax")
        assert np.array_equal(ref.double().numpy(), P.segment_max(feat, L["order0"], L["seg_start"]))
        order_d, seg_d = _t(L["order0"], dev), _t(L["seg_start"], dev)
        got = ops.pool_max(feat.to(dev), order_d, seg_d, n_out)
        assert got.dtype == dtype and torch.equal(got.float().cpu(), ref), f"pool_max c={c} n_out={n_out}"
        coord, grid, batch, code = _geometry(L["n"], 2, np.random.default_rng(c))
        got2 = ops.pool_reduce(feat.to(dev), _t(coord, dev), _t(grid, dev), _t(batch, dev), _t(code, dev), order_d,
                               seg_d, n_out, 1)[0]
        assert got2.dtype == dtype and torch.equal(got2.float().cpu(), ref), f"pool_reduce c={c} n_out={n_out}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", [16, 48, 260])
def test_pool_max_repeated_members(dev, c, dtype):
    """the eval layout of GridKNNDownsample: fixed segments of 16 neighbour ids drawn with replacement"""
    from ptv3_hip import ops
    g = torch.Generator().manual_seed(c)
    m, nsrc = 500, 3000
    y = torch.randn(nsrc, c, generator=g).to(dtype)
    idx = torch.randint(0, nsrc, (m, 16), generator=g)
    assert any(len(set(row.tolist())) < 16 for row in idx[:200]) and idx.unique().numel() < nsrc
    starts = torch.arange(0, 16 * (m + 1), 16, dtype=torch.int32)
    got = ops.pool_max(y.to(dev), idx.reshape(-1).contiguous().to(dev), starts.to(dev), m)
    assert torch.equal(got.cpu(), y[idx].max(1).values)


EPILOGUES = [("scale", P.ACT_NONE), ("scale", P.ACT_RELU), ("scale", P.ACT_GELU), (None, P.ACT_RELU), (None, P.ACT_GELU)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("scale,act", EPILOGUES, ids=["bn", "bn_relu", "bn_gelu", "relu", "gelu"])
@pytest.mark.parametrize("c", [16, 64, 260])
def test_pool_reduce_epilogue(dev, c, scale, act, dtype):
    """act(max * bn_scale + bn_shift) against float64 with the exact erf.  fp32: the parity budget FP32_TOL scaled by
    max(1, |ref|).  bf16: one bf16 step (2**-8 relative) for the single final rounding on top of that budget."""
    from ptv3_hip import ops
    L = _layout(257)
    n_out = L["n_out"]
    rng = np.random.default_rng(c)
    feat = _feat(L, c, dtype, with_inf=False)
    bn_scale = bn_shift = None
    if scale:
        bn_scale = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(np.float32)   # distinct per channel
        bn_shift = rng.standard_normal(c).astype(np.float32)
        assert len(set(bn_scale.tolist())) == c and len(set(bn_shift.tolist())) == c
    ref = P.pool_feat(feat, L["order0"], L["seg_start"], bn_scale, bn_shift, act)
    coord, grid, batch, code = _geometry(L["n"], 1, rng)
    got = ops.pool_reduce(feat.to(dev), None, _t(grid, dev), _t(batch, dev), _t(code, dev), _t(L["order0"], dev),
                          _t(L["seg_start"], dev), n_out, 0, None if bn_scale is None else _t(bn_scale, dev),
                          None if bn_shift is None else _t(bn_shift, dev), act)[0]
    assert got.dtype == dtype
    err = np.abs(_np64(got) - ref)
    if dtype == torch.float32:
        bound = FP32_TOL * np.maximum(1.0, np.abs(ref))
    else:
        bound = 2.0 ** -8 * np.abs(ref) + FP32_TOL
    print(f"epilogue c={c} scale={bool(scale)} act={act} {dtype}: max err {err.max():.3e}, "
          f"max err/bound {(err / bound).max():.3e}")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------
# C. pool_reduce, geometry half
# ------------------------------------------------------------------------------------------------
PERMS = {1: [0], 2: [1, 0], 4: [2, 0, 3, 1], 8: [5, 2, 7, 0, 3, 6, 1, 4]}


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
@pytest.mark.parametrize("k", [1, 2, 4, 8])
def test_pool_geometry_heads_codes_and_permutation(dev, k, depth):
    from ptv3_hip import ops
    L = _layout(257)
    n_out = L["n_out"]
    coord, grid, batch, code = _geometry(L["n"], k, np.random.default_rng(8 * k + depth))
    feat = _feat(L, 8, torch.float32, with_inf=False).to(dev)
    d = [_t(a, dev) for a in (coord, grid, batch, code, L["order0"], L["seg_start"])]
    for perm in (None, list(range(k)), PERMS[k]):
        ref = P.pool_geometry(coord, grid, batch, code, L["order0"], L["seg_start"], depth, perm)
        geo = ops.pool_geometry(*d, n_out, depth, perm)
        full = ops.pool_reduce(feat, *d, n_out, depth, row_perm=perm)[1:]
        nocoord = ops.pool_geometry(None, *d[1:], n_out, depth, perm)
        assert nocoord[0] is None
        for got in (geo, full, nocoord):
            assert np.array_equal(got[1].cpu().numpy(), ref[1]), "grid_out"
            assert np.array_equal(got[2].cpu().numpy(), ref[2]), "batch_out"
            assert got[3].shape == (k, n_out) and np.array_equal(got[3].cpu().numpy(), ref[3]), f"code_out perm={perm}"
        assert torch.equal(geo[0], full[0])                    # the two entry points run the same kernel
        assert np.abs(_np64(geo[0]) - ref[0]).max() < 1e-4     # the tight bound is test_pool_mean_coord's
    if k > 1:   # the head's code rows really differ, so a permutation is visible
        assert not np.array_equal(ref[3], P.pool_geometry(None, grid, batch, code, L["order0"], L["seg_start"], depth)[3])


@pytest.mark.parametrize("k", [1, 4, 8])
def test_pool_reduce_refuses_bad_row_permutation(dev, k):
    """a host-side argument check: nothing is launched"""
    from ptv3_hip import ops
    L = _layout(3)
    coord, grid, batch, code = _geometry(L["n"], k, np.random.default_rng(k))
    d = [_t(a, dev) for a in (coord, grid, batch, code, L["order0"], L["seg_start"])]
    for bad in (k, -1):
        perm = list(range(k))
        perm[-1] = bad
        with pytest.raises(RuntimeError, match="bad row permutation"):
            ops.pool_geometry(*d, L["n_out"], 1, perm)
        with pytest.raises(RuntimeError, match="bad row permutation"):
            ops.pool_reduce(_feat(L, 4, torch.float32, False).to(dev), *d, L["n_out"], 1, row_perm=perm)


@pytest.mark.parametrize("coord_kind", ["unit", "offset1000"])
@pytest.mark.parametrize("n_out", [3, 257, 2001])
def test_pool_mean_coord(dev, n_out, coord_kind):
    """coord_out against the float64 mean.  The kernel sums a segment's cnt members sequentially in fp32 (cnt - 1
    roundings, each at most 2**-24 of a partial sum <= cnt * max|coord|), then multiplies by a rounded reciprocal
    (two more roundings of at most 2**-24 * max|coord|): |err| <= (cnt + 1) * 2**-24 * max|coord| <=
    cnt * 2**-23 * max|coord|, the maximum taken over the segment's members per axis."""
    from ptv3_hip import ops
    L = _layout(n_out)
    coord, grid, batch, code = _geometry(L["n"], 2, np.random.default_rng(n_out), coord_kind)
    ref = P.segment_mean(coord, L["order0"], L["seg_start"])
    amax = np.maximum.reduceat(np.abs(coord.astype(np.float64))[L["order0"]], L["seg_start"][:-1].astype(np.int64), axis=0)
    bound = L["seg_len"][:, None] * 2.0 ** -23 * amax
    got = ops.pool_geometry(*[_t(a, dev) for a in (coord, grid, batch, code, L["order0"], L["seg_start"])], n_out, 1)[0]
    assert got.dtype == torch.float32 and got.shape == (n_out, 3)
    err = np.abs(_np64(got) - ref)
    j = n_out // 2
    print(f"mean coord n_out={n_out} {coord_kind}: max err {err.max():.3e}, max err/bound {(err / bound).max():.3e}, "
          f"700-member segment err {err[j].max():.3e} (bound {bound[j].min():.3e})")
    assert L["seg_len"][j] == 700 and (err <= bound).all()


# ------------------------------------------------------------------------------------------------
# D. pool_max_bwd / A.segment_max
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("data", ["coarse", "continuous"])
@pytest.mark.parametrize("c", [4, 7, 48, 260])   # 7: segment_bwd_kernel needs no multiple of 4 (the forward does)
def test_pool_max_bwd_first_maximum_takes_the_gradient(dev, c, data, dtype):
    """Per (segment, channel) dy goes to the first member, in serialized order, holding the maximum; every other
    member gets exactly 0.  Bit for bit in both dtypes; on the coarse grid most segments hold ties."""
    from ptv3_hip import autograd as A
    from ptv3_hip import ops
    for n_out in (3, 257, 2001):
        L = _layout(n_out)
        n, order0, seg_start = L["n"], L["order0"], L["seg_start"]
        rng = np.random.default_rng(31 * c + n_out)
        if data == "coarse":
            feat = torch.from_numpy(rng.integers(-2, 3, size=(n, c)).astype(np.float32))
        else:
            feat = torch.from_numpy(rng.standard_normal((n, c)).astype(np.float32))
        feat[torch.from_numpy(order0[seg_start[1]:seg_start[2]])] = -math.inf      # a segment of -inf only
        feat = feat.to(dtype)
        dy = torch.from_numpy(rng.standard_normal((n_out, c)).astype(np.float32)).to(dtype)
        assert (dy != 0).all()
        ref = P.max_bwd(feat, dy, order0, seg_start)
        if data == "coarse":   # ties are the rule here, not the exception
            mx = P.segment_max(feat, order0, seg_start)
            holders = P.segment_sum((_np64(feat) == mx[L["cluster"]]).astype(np.float64), order0, seg_start)
            assert (holders > 1).mean() > 0.3
        order_d, seg_d = _t(order0, dev), _t(seg_start, dev)
        got = _np64(ops.pool_max_bwd(feat.to(dev), dy.to(dev), order_d, seg_d))
        # the whole of dfeat is written (it starts as torch.empty) and equals the reference everywhere
        assert np.array_equal(got, ref), f"dfeat c={c} n_out={n_out}"
        assert np.array_equal(got[order0[seg_start[1]]], _np64(dy)[1])              # all -inf: the first member
        assert np.array_equal(P.segment_sum(got, order0, seg_start), _np64(dy))     # a valid gradient: sums to dy
        assert ((got != 0).reshape(n, c)[order0].cumsum(0)[seg_start[1:] - 1] ==
                np.arange(1, n_out + 1)[:, None]).all()                             # exactly one taker each
        if c % 4 == 0:
            fd = feat.to(dev).requires_grad_(True)
            out = A.segment_max(fd, order_d, seg_d, n_out)
            out.backward(dy.to(dev))
            assert np.array_equal(_np64(out), P.segment_max(feat, order0, seg_start))
            assert fd.grad.dtype == dtype and np.array_equal(_np64(fd.grad), ref)


# ------------------------------------------------------------------------------------------------
# E. segment_sum / A.cluster_gather backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("c", [4, 48, 260])
def test_segment_sum_and_cluster_gather_backward(dev, c, dtype):
    """Float64 segment sums.  fp32: a sequential sum of cnt terms makes cnt - 1 roundings of at most 2**-24 of a
    partial sum <= sum|dy|, so |err| <= cnt * 2**-24 * sum|dy|.  bf16 adds the final rounding, 2**-8 * |ref|."""
    from ptv3_hip import autograd as A
    from ptv3_hip import ops
    worst = 0.0
    for n_out in NOUTS:
        L = _layout(n_out)
        n, order0, seg_start = L["n"], L["order0"], L["seg_start"]
        dy = _feat(L, c, dtype, with_inf=False)
        ref = P.segment_sum(dy, order0, seg_start)
        bound = L["seg_len"][:, None] * 2.0 ** -24 * P.segment_sum(dy.float().abs(), order0, seg_start)
        if dtype == torch.bfloat16:
            bound = bound + 2.0 ** -8 * np.abs(ref)
        order_d, seg_d = _t(order0, dev), _t(seg_start, dev)
        got = ops.segment_sum(dy.to(dev), order_d, seg_d, n_out)
        assert got.dtype == dtype and got.shape == (n_out, c)
        err = np.abs(_np64(got) - ref)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), f"segment_sum c={c} n_out={n_out}: {(err / bound).max():.3f} of the bound"
        parent = torch.from_numpy(L["base"][:n_out, :c].copy()).to(dtype).to(dev).requires_grad_(True)
        cluster_d = _t(L["cluster"], dev)
        out = A.cluster_gather(parent, cluster_d, order_d, seg_d)
        assert torch.equal(out.detach(), parent.detach()[cluster_d])
        out.backward(dy.to(dev))
        assert torch.equal(parent.grad, got)
    print(f"segment_sum c={c} {dtype}: max err/bound {worst:.3e}")
