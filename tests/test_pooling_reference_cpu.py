"""CPU checks of oracle/pooling.py, the float64 reference that tests/test_hip_pooling.py holds the pooling kernels
to: against torch.unique, oracle.ptv3.segment_reduce, scatter_reduce("amax") and literal Python loops."""
import math

import numpy as np
import pytest
import torch

from oracle import pooling as P
from oracle import ptv3 as O


def _layout(seed, n_runs=300, with_long=True):
    rng = np.random.default_rng(seed)
    seg_len = rng.integers(1, 9, size=n_runs)
    if with_long:
        seg_len[n_runs // 2] = 700
    n = int(seg_len.sum())
    return rng, seg_len, P.starts_of(seg_len), rng.permutation(n), n


@pytest.mark.parametrize("shift", [0, 3, 9])
@pytest.mark.parametrize("scenes", [None, 1, 5])
def test_segments_match_torch_unique(shift, scenes):
    rng = np.random.default_rng(7 + shift)
    run_len = rng.integers(1, 9, size=400)
    scene_of_run = None if scenes is None else np.sort(rng.integers(0, scenes, size=400))
    code0, order0, batch = P.synth_codes(run_len, shift, rng, scene_of_run)
    assert (np.diff(code0[order0]) >= 0).all()                      # order0 serializes code0
    res = P.pool_segments(code0, order0, shift, batch, scenes or 0)
    cluster, seg_start, n_out = res[:3]
    uniq, inv = torch.unique(torch.from_numpy(code0) >> shift, sorted=True, return_inverse=True)
    assert n_out == uniq.numel() == run_len.size                    # the runs are the ones asked for
    assert np.array_equal(cluster, inv.numpy())
    assert np.array_equal(seg_start, P.starts_of(run_len))
    if scenes is not None:
        assert (np.diff(batch[order0]) >= 0).all()                  # scenes are contiguous along order0
        per_scene = [len(set((code0[batch == b] >> shift).tolist())) for b in range(scenes)]
        assert np.array_equal(res[3], np.cumsum(per_scene))


def test_segments_empty_scenes_repeat_their_predecessor():
    rng = np.random.default_rng(0)
    run_len = rng.integers(1, 5, size=30)
    scene_of_run = np.repeat([1, 3], 15)          # scenes 0, 2 and 4 of five hold no point
    code0, order0, batch = P.synth_codes(run_len, 3, rng, scene_of_run)
    assert P.pool_segments(code0, order0, 3, batch, 5)[3].tolist() == [0, 15, 15, 30, 30]


def test_twin_scenes_differ_in_the_scene_bits_only():
    rng = np.random.default_rng(1)
    run_len = np.array([3, 2, 1, 1, 4, 2])
    code0, order0, batch = P.synth_codes(run_len, 6, rng, np.array([0, 0, 0, 1, 1, 1]), twin_scenes=0)
    keys = code0[order0]
    assert keys[5] ^ keys[6] == 1 << P.BATCH_SHIFT
    assert P.pool_segments(code0, order0, 6, batch, 2)[3].tolist() == [3, 6]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_segment_max_matches_segment_reduce_and_scatter_amax(dtype):
    rng, seg_len, seg_start, order0, n = _layout(2)
    feat = torch.from_numpy(rng.standard_normal((n, 12)).astype(np.float32)).to(dtype)
    feat[torch.from_numpy(rng.random((n, 12)) < 0.05)] = -math.inf
    got = P.segment_max(feat, order0, seg_start)
    ref = O.segment_reduce(feat.float()[torch.from_numpy(order0)], torch.from_numpy(seg_start).long(), "max")
    assert np.array_equal(got, ref.double().numpy())
    cluster = torch.empty(n, dtype=torch.long)
    cluster[torch.from_numpy(order0)] = torch.repeat_interleave(torch.arange(seg_len.size), torch.from_numpy(seg_len))
    amax = torch.full((seg_len.size, 12), -math.inf).scatter_reduce(
        0, cluster[:, None].expand(-1, 12), feat.float(), "amax")
    assert np.array_equal(got, amax.double().numpy())
    assert np.array_equal(got, P.pool_feat(feat, order0, seg_start))


def test_epilogue_matches_torch_float64():
    rng, seg_len, seg_start, order0, n = _layout(3, with_long=False)
    feat = rng.standard_normal((n, 8))
    scale, shift = rng.uniform(0.5, 1.5, 8), rng.standard_normal(8)
    mx = torch.from_numpy(P.segment_max(feat, order0, seg_start))
    z = mx * torch.from_numpy(scale) + torch.from_numpy(shift)
    F = torch.nn.functional
    for act, fn in ((P.ACT_NONE, lambda t: t), (P.ACT_RELU, F.relu), (P.ACT_GELU, F.gelu)):
        got = P.pool_feat(feat, order0, seg_start, scale, shift, act)
        assert np.abs(got - fn(z).numpy()).max() < 1e-14
        assert np.abs(P.pool_feat(feat, order0, seg_start, act=act) - fn(mx).numpy()).max() < 1e-14
    assert abs(float(P.gelu(np.array([1.0]))[0]) - 0.5 * (1.0 + math.erf(math.sqrt(0.5)))) < 1e-15


def test_max_bwd_tie_rule_is_first_member():
    rng, seg_len, seg_start, order0, n = _layout(4, n_runs=120, with_long=False)
    feat = rng.integers(-2, 3, size=(n, 5)).astype(np.float64)      # coarse grid: most segments hold ties
    feat[order0[seg_start[7]:seg_start[8]]] = -math.inf             # a segment of -inf only
    dy = rng.standard_normal((seg_len.size, 5))
    got = P.max_bwd(feat, dy, order0, seg_start)
    ref = np.zeros_like(feat)
    ties = 0
    for j in range(seg_len.size):
        for ch in range(5):
            members = [int(r) for r in order0[seg_start[j]:seg_start[j + 1]]]
            best = members[0]
            for r in members[1:]:
                if feat[r, ch] > feat[best, ch]:                    # strict: an equal later member never wins
                    best = r
            ref[best, ch] = dy[j, ch]
            ties += sum(feat[r, ch] == feat[best, ch] for r in members) > 1
    assert ties > seg_len.size                                      # the rule is really exercised
    assert np.array_equal(got, ref)
    assert np.array_equal(got[order0[seg_start[7]]], dy[7])         # all -inf: the first member takes it
    assert np.array_equal(P.segment_sum(got, order0, seg_start), dy)


def test_max_bwd_without_ties_matches_torch_autograd():
    rng, seg_len, seg_start, order0, n = _layout(5, n_runs=100, with_long=False)
    feat = torch.from_numpy(rng.standard_normal((n, 6))).requires_grad_(True)
    dy = rng.standard_normal((seg_len.size, 6))
    torch.segment_reduce(feat[torch.from_numpy(order0)], "max", lengths=torch.from_numpy(seg_len), axis=0).backward(
        torch.from_numpy(dy))
    assert np.array_equal(P.max_bwd(feat, dy, order0, seg_start), feat.grad.numpy())


def test_segment_sum_and_mean_match_segment_reduce():
    rng, seg_len, seg_start, order0, n = _layout(6)
    x = torch.from_numpy(rng.standard_normal((n, 7)))
    ptr = torch.from_numpy(seg_start).long()
    xs = x[torch.from_numpy(order0)]
    assert np.abs(P.segment_sum(x, order0, seg_start) - O.segment_reduce(xs, ptr, "sum").numpy()).max() < 1e-12
    assert np.abs(P.segment_mean(x, order0, seg_start) - O.segment_reduce(xs, ptr, "mean").numpy()).max() < 1e-13


def test_geometry_takes_the_head_member():
    rng, seg_len, seg_start, order0, n = _layout(8, n_runs=50, with_long=False)
    coord = rng.standard_normal((n, 3))
    grid = rng.integers(0, 1 << 16, size=(n, 3))
    batch = rng.integers(0, 4, size=n)
    code = rng.integers(0, 1 << 40, size=(4, n))
    perm = [2, 0, 3, 1]
    coord_out, grid_out, batch_out, code_out = P.pool_geometry(coord, grid, batch, code, order0, seg_start, 2, perm)
    for j in (0, 17, 49):
        members = order0[seg_start[j]:seg_start[j + 1]]
        head = members[0]
        assert np.allclose(coord_out[j], coord[members].mean(0), rtol=0, atol=1e-14)
        assert grid_out[j].tolist() == [int(v) >> 2 for v in grid[head]]
        assert batch_out[j] == batch[head]
        assert [int(code_out[r, j]) for r in range(4)] == [int(code[perm[r], head]) >> 6 for r in range(4)]
    assert P.pool_geometry(None, grid, batch, code, order0, seg_start, 0)[0] is None
    assert np.array_equal(P.pool_geometry(None, grid, batch, code, order0, seg_start, 0)[3], code[:, order0[seg_start[:-1]]])
