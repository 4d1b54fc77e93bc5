"""Oracle (test infrastructure): float64 restatement of the serialized pooling family - ptv3_pool_segments,
ptv3_pool_reduce (feature half and geometry half), ptv3_pool_max_bwd and ptv3_segment_sum - in plain numpy / torch.

The layout all of them share: `order0` (n) lists source rows in serialized order, `seg_start` (n_out + 1) cuts that
list into non-empty runs, pooled row j has the members order0[seg_start[j] : seg_start[j + 1]].  A member list may
name a source row more than once (the fixed 16-neighbour segments of GridKNNDownsample).

NaN is out of scope everywhere here: the kernels' fmaxf drops a NaN, numpy's maximum keeps it.

tests/test_pooling_reference_cpu.py holds this file to torch.unique, oracle.ptv3.segment_reduce,
scatter_reduce("amax") and a literal loop; tests/test_hip_pooling.py holds the kernels to this file."""
import math

import numpy as np
import torch

ACT_NONE, ACT_GELU, ACT_RELU = 0, 1, 2   # PTV3_ACT_* of include/ptv3_hip.h

BATCH_SHIFT = 48   # synth_codes puts the scene id here, above every parent and low bit it draws


# ----------------------------------------------------------------------------
# input construction
# ----------------------------------------------------------------------------
def synth_codes(run_len, shift, rng, scene_of_run=None, twin_scenes=None):
    """Serialized codes with prescribed runs.  run_len (R) ints: run r has run_len[r] points that share
    `code >> shift`; consecutive runs differ in it.  scene_of_run (R) non-decreasing ints puts the scene id in the
    top bits of the key, as the real codes carry it, so scenes are contiguous along order0.  twin_scenes = b makes
    the last key of scene b and the first key of scene b + 1 differ in the scene bits only (both runs must have
    one point).  Returns code0 (n) int64, order0 (n) int64 (a random permutation; code0[order0] is sorted) and
    batch (n) int64 or None."""
    run_len = np.asarray(run_len, dtype=np.int64)
    R = run_len.size
    scene = np.zeros(R, dtype=np.int64) if scene_of_run is None else np.asarray(scene_of_run, dtype=np.int64)
    assert scene.size == R and (np.diff(scene) >= 0).all() and (run_len >= 1).all()
    parent = np.empty(R, dtype=np.int64)
    for b in np.unique(scene):          # strictly increasing parents inside a scene, restarting in each
        m = scene == b
        parent[m] = np.cumsum(rng.integers(1, 4, size=int(m.sum())))
    if twin_scenes is not None:
        last = int(np.nonzero(scene == twin_scenes)[0][-1])
        nxt = scene == twin_scenes + 1
        first = int(np.nonzero(nxt)[0][0])
        assert first == last + 1 and run_len[last] == 1 and run_len[first] == 1
        parent[nxt] += parent[last] - parent[first]
    assert parent.max() < (1 << (BATCH_SHIFT - shift - 1))
    n = int(run_len.sum())
    run_of = np.repeat(np.arange(R), run_len)
    low = rng.integers(0, 1 << shift, size=n) if shift else np.zeros(n, dtype=np.int64)
    if twin_scenes is not None:
        s = int(run_len[:last].sum())
        low[s] = low[s + 1] = 0
    keys = (scene[run_of] << BATCH_SHIFT) | (parent[run_of] << shift) | low
    keys = np.sort(keys)                # the low bits sort inside a run; (scene, parent) already ascend
    order0 = rng.permutation(n)
    code0 = np.empty(n, dtype=np.int64)
    code0[order0] = keys
    batch = None
    if scene_of_run is not None:
        batch = np.empty(n, dtype=np.int64)
        batch[order0] = scene[run_of]
    return code0, order0.astype(np.int64), batch


def starts_of(seg_len):
    """seg_start (n_out + 1) int32 of the given run lengths."""
    return np.concatenate([[0], np.cumsum(np.asarray(seg_len, dtype=np.int64))]).astype(np.int32)


# ----------------------------------------------------------------------------
# ptv3_pool_segments
# ----------------------------------------------------------------------------
def pool_segments(code0, order0, shift, batch=None, num_scenes=0):
    """cluster (n) int64, seg_start (n_out + 1) int32, n_out, and with batch the pooled cumulative offsets
    (num_scenes) int64: the running count of clusters up to and including each scene, so a scene without points
    repeats its predecessor (0 for a leading one)."""
    code0, order0 = torch.as_tensor(code0), torch.as_tensor(order0)
    n = code0.numel()
    _, inv, counts = torch.unique_consecutive(code0[order0] >> shift, return_inverse=True, return_counts=True)
    cluster = torch.empty(n, dtype=torch.int64)
    cluster[order0] = inv
    seg_start = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).int()
    n_out = counts.numel()
    if batch is None:
        return cluster.numpy(), seg_start.numpy(), n_out
    head_scene = torch.as_tensor(batch)[order0[seg_start[:-1].long()]]
    pooled_offset = torch.bincount(head_scene, minlength=num_scenes).cumsum(0)
    return cluster.numpy(), seg_start.numpy(), n_out, pooled_offset.numpy()


# ----------------------------------------------------------------------------
# ptv3_pool_reduce
# ----------------------------------------------------------------------------
def _f64(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().double().numpy()
    return np.asarray(x, dtype=np.float64)


def _cuts(seg_start):
    s = np.asarray(seg_start, dtype=np.int64)
    assert (np.diff(s) >= 1).all(), "segments are non-empty"
    return s[:-1]


def segment_max(feat, order0, seg_start):
    """(n_out, c) float64: max over the members.  A selection: exact for fp32 / bf16 inputs."""
    return np.maximum.reduceat(_f64(feat)[np.asarray(order0)], _cuts(seg_start), axis=0)


def gelu(x):
    """exact-erf GELU in float64."""
    x = np.asarray(x, dtype=np.float64)
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x * math.sqrt(0.5)))).numpy())


def pool_feat(feat, order0, seg_start, bn_scale=None, bn_shift=None, act=ACT_NONE):
    """(n_out, c) float64: act(max_members(feat) * bn_scale + bn_shift)."""
    y = segment_max(feat, order0, seg_start)
    if bn_scale is not None:
        y = y * _f64(bn_scale)[None, :] + _f64(bn_shift)[None, :]
    if act == ACT_GELU:
        y = gelu(y)
    elif act == ACT_RELU:
        y = np.maximum(y, 0.0)
    return y


def segment_mean(x, order0, seg_start):
    """(n_out, d) float64 mean over the members."""
    s = np.asarray(seg_start, dtype=np.int64)
    return np.add.reduceat(_f64(x)[np.asarray(order0)], _cuts(s), axis=0) / np.diff(s)[:, None]


def pool_geometry(coord, grid_coord, batch, code, order0, seg_start, pooling_depth, row_perm=None):
    """coord_out (n_out, 3) float64 mean (None without coord); from the head member (the first of the run):
    grid_out = grid_coord[head] >> depth, batch_out = batch[head], code_out[r] = code[row_perm[r]][head] >> 3 * depth."""
    order0 = np.asarray(order0)
    head = order0[_cuts(seg_start)]
    code = np.asarray(code)
    perm = np.arange(code.shape[0]) if row_perm is None else np.asarray(row_perm, dtype=np.int64)
    coord_out = None if coord is None else segment_mean(coord, order0, seg_start)
    return (coord_out, np.asarray(grid_coord)[head] >> pooling_depth, np.asarray(batch)[head],
            code[perm][:, head] >> (3 * pooling_depth))


# ----------------------------------------------------------------------------
# ptv3_pool_max_bwd, ptv3_segment_sum
# ----------------------------------------------------------------------------
def max_bwd(feat, dy, order0, seg_start):
    """(n, c) float64: per (segment, channel) dy goes to the FIRST member, in order0 order, that holds the maximum
    (the strict > of segment_csr's arg-max); every other member gets exactly 0.  Each source row must be the
    member of exactly one segment."""
    f, g, order0 = _f64(feat), _f64(dy), np.asarray(order0)
    s = np.asarray(seg_start, dtype=np.int64)
    out = np.zeros_like(f)
    cols = np.arange(f.shape[1])
    for j in range(s.size - 1):
        rows = order0[s[j]:s[j + 1]]
        out[rows[np.argmax(f[rows], axis=0)], cols] = g[j]
    return out


def segment_sum(x, order0, seg_start):
    """(n_out, c) float64 sum over the members."""
    return np.add.reduceat(_f64(x)[np.asarray(order0)], _cuts(seg_start), axis=0)
