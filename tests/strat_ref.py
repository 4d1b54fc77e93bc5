"""CPU restatement of what the Stratified Transformer path computes: the pointops2 functions the reference model calls
(libs/pointops2/functions/pointops.py; kernels in libs/pointops2/src/{attention_v2,rpe_v2,knnquery,sampling}), the group
plan that replaces BasicLayer.forward's edge list, the partial_dense ball query and the group form of the attention.
Plain torch / numpy in the dtype of the inputs (float64 inputs give the float64 reference); differentiable where the
reference is.  Used by the tests and, as the `pointops2.pointops` stand-in, by tests/golden/make_golden_keypoint_strat.py.
"""
import numpy as np
import torch


# ---- the three attention functions on the edge list (index_0 sorted, index_0_offsets (n + 1) its run starts) --------
def _index_0(index_0_offsets, m):
    counts = (index_0_offsets[1:] - index_0_offsets[:-1]).long()
    return torch.repeat_interleave(torch.arange(counts.shape[0], device=counts.device), counts, output_size=m)


def attention_step1_v2(q, k, index_1, index_0_offsets, n_max):
    """(M, h): q[index_0[e]] . k[index_1[e]] per head (attention_step1_forward_cuda_kernel_v2)."""
    i0 = _index_0(index_0_offsets, index_1.shape[0])
    return (q[i0] * k[index_1.long()]).sum(-1)


def _table_rows(table, rel_idx):
    """(M, h, d): sum over the three axes a of table[rel_idx[e, a], :, :, a]."""
    r = rel_idx.long()
    return table[r[:, 0], :, :, 0] + table[r[:, 1], :, :, 1] + table[r[:, 2], :, :, 2]


def dot_prod_with_idx_v3(q, index_q_offsets, n_max, k, index_k, table_q, table_k, rel_idx):
    """(M, h): q[index_0] . sum_a table_q[rel_idx[:, a], :, :, a] + k[index_1] . sum_a table_k[...]
    (dot_prod_with_idx_forward_cuda_kernel_v3)."""
    i0 = _index_0(index_q_offsets, index_k.shape[0])
    return (q[i0] * _table_rows(table_q, rel_idx)).sum(-1) + (k[index_k.long()] * _table_rows(table_k, rel_idx)).sum(-1)


def attention_step2_with_rel_pos_value_v2(attn, v, index_0_offsets, n_max, index_1, table, rel_idx):
    """(n, h, d): out[i] = sum over i's edges of attn[e] (v[index_1[e]] + sum_a table[rel_idx[e, a], :, :, a])."""
    i0 = _index_0(index_0_offsets, index_1.shape[0])
    n = index_0_offsets.shape[0] - 1
    rows = attn.unsqueeze(-1) * (v[index_1.long()] + _table_rows(table, rel_idx))
    return torch.zeros((n,) + tuple(v.shape[1:]), dtype=rows.dtype, device=rows.device).index_add_(0, i0, rows)


def scatter_softmax(src, index, dim=0):
    """torch_scatter.scatter_softmax along dim 0 for a sorted or unsorted index."""
    assert dim == 0
    n = int(index.max()) + 1
    idx = index.long().view(-1, *([1] * (src.dim() - 1))).expand_as(src)
    mx = torch.full((n,) + tuple(src.shape[1:]), -float("inf"), dtype=src.dtype).scatter_reduce(
        0, idx, src.detach(), "amax", include_self=True)
    e = torch.exp(src - mx.gather(0, idx))
    return e / torch.zeros_like(mx).scatter_add(0, idx, e).gather(0, idx)


def rel_index(coord, index_0, index_1, window, quant):
    """relative_position_index of WindowAttention.forward (:163-169), torch's own kernels in coord's dtype."""
    rel = coord[index_0.long()] - coord[index_1.long()]
    rel = torch.round(rel * 100000) / 100000
    return torch.div(rel + 2 * window - 1e-4, quant, rounding_mode="trunc")


def edge_attention(q, k, v, coord, index_0, index_1, tq, tk, tv, scale, window, quant, rel=None):
    """WindowAttention.forward between qkv and proj (:157-220) over an edge list sorted by index_0: (n, h, d)."""
    n = q.shape[0]
    counts = torch.bincount(index_0.long(), minlength=n)
    offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    if rel is None:
        rel = rel_index(coord, index_0, index_1, window, quant)
    qs = q * scale
    attn = attention_step1_v2(qs, k, index_1, offsets, None) + dot_prod_with_idx_v3(qs, offsets, None, k, index_1, tq, tk,
                                                                                   rel)
    attn = scatter_softmax(attn, index_0, 0)
    return attention_step2_with_rel_pos_value_v2(attn, v, offsets, None, index_1, tv, rel)


def group_attention(q, k, v, coord, groups, tq, tk, tv, scale, window, quant, rel_coord=None):
    """The group formula: per (query rows, key rows) group a dense softmax.  rel_coord: the coordinates r_a is computed
    from (default coord; pass the fp32 ones with float64 q / k / v so that the float64 reference uses the fp32 index,
    which is part of the input's definition, not of the arithmetic under test)."""
    out = torch.zeros_like(q)
    rc = coord if rel_coord is None else rel_coord
    for qr, kr in groups:
        qr, kr = torch.as_tensor(qr).long(), torch.as_tensor(kr).long()
        i0, i1 = qr.repeat_interleave(len(kr)), kr.repeat(len(qr))
        r = rel_index(rc, i0, i1, window, quant).long().view(len(qr), len(kr), 3)
        qs = q[qr] * scale                                                   # (nq, h, d)
        e = torch.einsum("ihd,jhd->ijh", qs, k[kr])
        tv_rows = 0
        for a in range(3):
            e = e + torch.einsum("ihd,ijhd->ijh", qs, tq[r[..., a], :, :, a]) + \
                torch.einsum("jhd,ijhd->ijh", k[kr], tk[r[..., a], :, :, a])
            tv_rows = tv_rows + tv[r[..., a], :, :, a]                       # (nq, nk, h, d)
        p = torch.softmax(e, dim=1)
        out[qr] = torch.einsum("ijh,ijhd->ihd", p, v[kr].unsqueeze(0) + tv_rows)
    return out


# ---- the plan --------------------------------------------------------------------------------------------------
def cells(coord, cmin, window, shifted, large):
    """(n, 3) int64 window cells exactly as voxel_grid evaluates them in coord's dtype: ((x + s) - min) / size, s = half
    the size in shifted blocks (BasicLayer.forward :372-385)."""
    coord = torch.as_tensor(coord)
    size = torch.tensor([window] * 3, dtype=coord.dtype) * (2 if large else 1)
    pos = coord + size * 1 / 2 if shifted else coord
    return ((pos - torch.as_tensor(cmin, dtype=coord.dtype)) / size).long()


def group_plan(coord, ends, down_idx, window, shifted):
    """[(query rows, key rows)] as numpy int64 arrays: one group per (scene, small cell, large cell), in sorted key
    order (in shifted blocks a small cell straddles large cells, so the pair is the group); keys = ALL rows of the small
    cell, then the sampled rows of the large cell whose small cell differs (the device plan promises no order inside a
    part: compare as sets)."""
    coord = torch.as_tensor(coord, dtype=torch.float32)
    cmin = coord.min(0).values
    small = cells(coord, cmin, window, shifted, False).numpy()
    large = cells(coord, cmin, window, shifted, True).numpy()
    ends = np.asarray(ends, dtype=np.int64)
    batch = np.repeat(np.arange(len(ends)), np.diff(np.concatenate([[0], ends])))
    sampled = np.zeros(len(coord), dtype=bool)
    sampled[np.asarray(down_idx, dtype=np.int64)] = True
    groups, windows, smalls = {}, {}, {}
    for i in range(len(coord)):
        wk, sk = (batch[i],) + tuple(large[i]), (batch[i],) + tuple(small[i])
        groups.setdefault(sk + wk[1:], []).append(i)
        smalls.setdefault(sk, []).append(i)
        if sampled[i]:
            windows.setdefault(wk, []).append(i)
    out = []
    for key in sorted(groups):
        sk, wk = key[:4], (key[0],) + key[4:]
        sparse = [j for j in windows.get(wk, []) if tuple(small[j]) != sk[1:]]
        out.append((np.asarray(groups[key], dtype=np.int64), np.asarray(smalls[sk] + sparse, dtype=np.int64)))
    return out


def keys_per_query(groups, n):
    """[sorted key rows of query i] for i < n from a list of groups."""
    out = [None] * n
    for qr, kr in groups:
        ks = np.sort(np.asarray(kr, dtype=np.int64))
        for i in np.asarray(qr):
            assert out[i] is None, f"row {i} is a query of two groups"
            out[i] = ks
    return out


def reference_edges(coord, ends, down_idx, window, shifted):
    """Literal numpy transcription of BasicLayer.forward's masks (:388-442) for one parity: (index_0, index_1), sorted
    by index_0 (stable).  The one deliberate difference from the reference is kept OUT of this function: the shifted
    small-window test below uses the reference's own expression (x - min + w/2) / w."""
    coord = torch.as_tensor(coord, dtype=torch.float32)
    n = len(coord)
    ends = np.asarray(ends, dtype=np.int64)
    batch = torch.from_numpy(np.repeat(np.arange(len(ends)), np.diff(np.concatenate([[0], ends]))))
    cmin = coord.min(0).values

    def grid_sample(size, shift):
        c = cells(coord, cmin, size, shift, False)
        pos = torch.cat([c, batch.view(-1, 1)], 1)
        extent = pos.max(0).values + 1
        stride = torch.cat([extent.new_ones(1), torch.cumprod(extent, 0)[:-1]])
        cluster = (pos * stride).sum(1)
        _, cluster, counts = torch.unique(cluster, sorted=True, return_inverse=True, return_counts=True)
        k = int(counts.max())
        p2v = cluster.new_zeros(len(counts), k)
        mask = torch.arange(k).unsqueeze(0) < counts.unsqueeze(-1)
        p2v[mask] = torch.argsort(cluster, stable=True)
        return p2v, counts

    w = torch.tensor([window] * 3, dtype=torch.float32)
    p2v, counts = grid_sample(window, shifted)
    new_p2v, new_counts = grid_sample(2 * window, shifted)
    k = p2v.shape[1]
    mask = torch.arange(k).unsqueeze(0) < counts.unsqueeze(-1)
    mm = mask.unsqueeze(-1) & mask.unsqueeze(-2)
    index_0 = p2v.unsqueeze(-1).expand(-1, -1, k)[mm]
    index_1 = p2v.unsqueeze(1).expand(-1, k, -1)[mm]
    down_mask = torch.zeros(n, dtype=torch.bool)
    down_mask[torch.as_tensor(np.asarray(down_idx)).long()] = True
    down_mask = down_mask[new_p2v]
    k = new_p2v.shape[1]
    mask = torch.arange(k).unsqueeze(0) < new_counts.unsqueeze(-1)
    down_mask = down_mask & mask
    mm = mask.unsqueeze(-1) & down_mask.unsqueeze(-2)
    if not shifted:
        wc = torch.div(coord[new_p2v] - cmin, w, rounding_mode="trunc")
    else:
        wc = torch.div(coord[new_p2v] - cmin + 1 / 2 * w, w, rounding_mode="trunc")
    prev = (wc.unsqueeze(2) != wc.unsqueeze(1)).any(-1)
    mm = mm & prev
    index_0 = torch.cat([index_0, new_p2v.unsqueeze(-1).expand(-1, -1, k)[mm]], 0)
    index_1 = torch.cat([index_1, new_p2v.unsqueeze(1).expand(-1, k, -1)[mm]], 0)
    index_0, order = torch.sort(index_0, stable=True)
    return index_0.numpy(), index_1[order].numpy()


# ---- sampling, neighbours, grouping, interpolation (pointops2 call signatures) ---------------------------------------
def fps_scene(xyz, count):
    """Rows of one scene's farthest point sampling in fp32 ((dx*dx + dy*dy) + dz*dz, first maximum) and the smallest
    relative lead of a winner over the runner-up, measured in float64."""
    x32 = np.asarray(xyz, dtype=np.float32)
    x64 = x32.astype(np.float64)
    d32 = np.full(len(x32), 1e10, dtype=np.float32)
    d64 = np.full(len(x32), 1e10, dtype=np.float64)
    rows, gap, old = [0], np.inf, 0
    for _ in range(1, count):
        e = x32 - x32[old]
        d32 = np.minimum(d32, (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        d64 = np.minimum(d64, ((x64 - x64[old]) ** 2).sum(1))
        old = int(np.argmax(d32))
        assert old == int(np.argmax(d64)), "fp32 and float64 disagree on a selection"
        if len(d64) > 1:
            top2 = np.partition(d64, -2)[-2:]
            gap = min(gap, (top2[1] - top2[0]) / top2[1])
        rows.append(old)
    return np.asarray(rows[:count], dtype=np.int64), gap


FPS_LOG = {"gap": np.inf, "samples": []}


def furthestsampling(xyz, offset, new_offset):
    pts = xyz.detach().float().numpy()
    ends, new_ends = [int(v) for v in offset.tolist()], [int(v) for v in new_offset.tolist()]
    taken = []
    for s, e, ms, me in zip([0] + ends[:-1], ends, [0] + new_ends[:-1], new_ends):
        rows, gap = fps_scene(pts[s:e], me - ms)
        FPS_LOG["gap"] = min(FPS_LOG["gap"], gap)
        taken.append(rows + s)
    taken = np.concatenate(taken)
    FPS_LOG["samples"].append(taken)
    return torch.from_numpy(taken.astype(np.int32))


def knnquery(nsample, xyz, new_xyz, offset, new_offset):
    """(idx (m, nsample) int32, dist (m, nsample)): the nsample nearest rows of the query's scene, ascending; a scene
    shorter than nsample pads with ITS FIRST ROW at squared distance 1e10 (knnquery_cuda_kernel.cu:86-91), unlike the -1
    of libs/pointops."""
    if new_xyz is None:
        new_xyz = xyz
    x, y = xyz.detach().double().numpy(), new_xyz.detach().double().numpy()
    ends, new_ends = [int(v) for v in offset.tolist()], [int(v) for v in new_offset.tolist()]
    idx = np.zeros((len(y), nsample), dtype=np.int32)
    d2 = np.full((len(y), nsample), 1e10, dtype=np.float64)
    for s, e, ms, me in zip([0] + ends[:-1], ends, [0] + new_ends[:-1], new_ends):
        if me == ms:
            continue
        dd = ((y[ms:me, None, :] - x[None, s:e, :]) ** 2).sum(-1)
        order = np.argsort(dd, axis=1, kind="stable")[:, :nsample]
        kk = order.shape[1]
        idx[ms:me] = s
        idx[ms:me, :kk] = order + s
        d2[ms:me, :kk] = np.take_along_axis(dd, order, 1)
    return torch.from_numpy(idx), torch.from_numpy(np.sqrt(d2)).to(xyz.dtype)


def queryandgroup(nsample, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=True, return_indx=False):
    if new_xyz is None:
        new_xyz = xyz
    if idx is None:
        idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)
    m, c = new_xyz.shape[0], feat.shape[1]
    grouped_xyz = xyz[idx.view(-1).long(), :].view(m, nsample, 3) - new_xyz.unsqueeze(1)
    grouped_feat = feat[idx.view(-1).long(), :].view(m, nsample, c)
    out = torch.cat((grouped_xyz, grouped_feat), -1) if use_xyz else grouped_feat
    return (out, idx) if return_indx else out


def interpolation(xyz, new_xyz, feat, offset, new_offset, k=3):
    idx, dist = knnquery(k, xyz, new_xyz, offset, new_offset)
    dist_recip = 1.0 / (dist + 1e-8)
    weight = dist_recip / torch.sum(dist_recip, dim=1, keepdim=True)
    new_feat = torch.zeros(new_xyz.shape[0], feat.shape[1], dtype=feat.dtype)
    for i in range(k):
        new_feat = new_feat + feat[idx[:, i].long(), :] * weight[:, i].unsqueeze(-1)
    return new_feat


def ball_query(radius, max_neighbor, xyz, ends):
    """(idx (n, max_neighbor) int64, smallest relative distance of a d^2 from radius^2 in float64): the partial_dense
    ball query of a cloud against itself - per row the first max_neighbor rows of its scene, in index order, with
    d^2 < radius^2 (the row itself included), then -1."""
    x = np.asarray(xyz, dtype=np.float64)
    n = len(x)
    idx = np.full((n, max_neighbor), -1, dtype=np.int64)
    margin = np.inf
    ends = [int(v) for v in ends]
    r2 = float(np.float32(radius) * np.float32(radius))
    for s, e in zip([0] + ends[:-1], ends):
        d2 = ((x[s:e, None, :] - x[None, s:e, :]) ** 2).sum(-1)
        margin = min(margin, np.abs(d2 / r2 - 1).min()) if e > s else margin
        for i in range(e - s):
            rows = np.nonzero(d2[i] < r2)[0][:max_neighbor]
            idx[s + i, :len(rows)] = rows + s
    return idx, margin
