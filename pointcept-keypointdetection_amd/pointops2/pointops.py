"""The part of the reference's libs/pointops2/functions/pointops.py that Stratified Transformer (ST-v1m2) calls.

    furthestsampling(xyz, offset, new_offset)                    ptv3_farthest_point_sampling
    knnquery(nsample, xyz, new_xyz, offset, new_offset)          ptv3_knn_query; (idx int32, dist = sqrt(d2))
    queryandgroup(nsample, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=True, return_indx=False)
    interpolation(xyz, new_xyz, feat, offset, new_offset, k=3)
    attention_step1_v2, dot_prod_with_idx_v3, attention_step2_with_rel_pos_value_v2

pointops2's kNN pads a scene shorter than nsample with the scene's FIRST ROW at squared distance 1e10
(src/knnquery/knnquery_cuda_kernel.cu:86-91), not with the -1 of libs/pointops; that is reproduced here.
The three attention functions are differentiable torch compositions over the edge list, with the argument lists of
libs/pointops2/functions/pointops.py:170-258, 632-755, 854-961: they serve training and the unfused eval path, the fused
eval path is ops.stratified_attention.  Every other name of the reference's module raises NotImplementedError.
"""
import torch

from pointops import functions as _po
from ptv3_hip import ops


def furthestsampling(xyz, offset, new_offset):
    return _po.farthest_point_sampling(xyz, offset, new_offset)


def _pad_first_row(idx, new_offset, offset):
    """-1 -> first row of the query's scene."""
    starts = torch.cat([offset.new_zeros(1), offset[:-1]]).to(torch.int32)
    sizes = torch.diff(new_offset.long(), prepend=new_offset.new_zeros(1).long())
    scene = torch.repeat_interleave(torch.arange(sizes.shape[0], device=idx.device), sizes, output_size=idx.shape[0])
    return torch.where(idx < 0, starts[scene].unsqueeze(1), idx)


@torch.no_grad()
def knnquery(nsample, xyz, new_xyz, offset, new_offset):
    if new_xyz is None:
        new_xyz, new_offset = xyz, offset
    idx, dist = _po.knn_query(nsample, xyz, offset, new_xyz, new_offset)
    return _pad_first_row(idx, new_offset, offset), dist


def queryandgroup(nsample, xyz, new_xyz, feat, idx, offset, new_offset, use_xyz=True, return_indx=False):
    """(m, nsample, [3 +] c): the neighbours' offsets from the query in front of their features (pointops.py:964-1001)."""
    if new_xyz is None:
        new_xyz = xyz
    if not (xyz.is_contiguous() and new_xyz.is_contiguous() and feat.is_contiguous()):
        raise AssertionError("queryandgroup: xyz / new_xyz / feat must be contiguous")
    if idx is None:
        idx, _ = knnquery(nsample, xyz, new_xyz, offset, new_offset)
    idx = idx.contiguous()
    out = _po.grouping2(feat, idx)
    if use_xyz:
        out = torch.cat((_po.grouping2(xyz, idx) - new_xyz.unsqueeze(1), out), -1)
    return (out, idx) if return_indx else out


def interpolation(xyz, new_xyz, feat, offset, new_offset, k=3):
    """pointops.py:1113-1127: normalised 1 / (dist + 1e-8) blend of the k nearest rows."""
    if not (xyz.is_contiguous() and new_xyz.is_contiguous() and feat.is_contiguous()):
        raise AssertionError("interpolation: xyz / new_xyz / feat must be contiguous")
    idx, dist = knnquery(k, xyz, new_xyz, offset, new_offset)
    w = torch.reciprocal(dist + 1e-8)
    w = (w / w.sum(dim=1, keepdim=True)).contiguous()
    return _po._KnnBlend.apply(feat, idx.contiguous(), w)


def _index_0(index_0_offsets, m):
    counts = (index_0_offsets[1:] - index_0_offsets[:-1]).long()
    return torch.repeat_interleave(torch.arange(counts.shape[0], device=counts.device), counts, output_size=m)


def _table_rows(table, rel_idx):
    r = rel_idx.long()
    return table[r[:, 0], :, :, 0] + table[r[:, 1], :, :, 1] + table[r[:, 2], :, :, 2]


def attention_step1_v2(q, k, index_1, index_0_offsets, n_max):
    """(M, h) = q[index_0] . k[index_1] per head; index_0 is given by its run starts index_0_offsets (n + 1)."""
    return (q[_index_0(index_0_offsets, index_1.shape[0])] * k[index_1.long()]).sum(-1)


def dot_prod_with_idx_v3(q, index_q_offsets, n_max, k, index_k, table_q, table_k, rel_idx):
    """(M, h) = q[index_0] . sum_a table_q[rel_idx[:, a], :, :, a] + k[index_k] . sum_a table_k[rel_idx[:, a], :, :, a]"""
    i0 = _index_0(index_q_offsets, index_k.shape[0])
    return (q[i0] * _table_rows(table_q, rel_idx)).sum(-1) + (k[index_k.long()] * _table_rows(table_k, rel_idx)).sum(-1)


def attention_step2_with_rel_pos_value_v2(attn, v, index_0_offsets, n_max, index_1, table, rel_idx):
    """(n, h, d): out[i] = sum over i's edges e of attn[e] (v[index_1[e]] + sum_a table[rel_idx[e, a], :, :, a])"""
    i0 = _index_0(index_0_offsets, index_1.shape[0])
    rows = attn.unsqueeze(-1) * (v[index_1.long()] + _table_rows(table, rel_idx))
    out = torch.zeros((index_0_offsets.shape[0] - 1,) + tuple(v.shape[1:]), dtype=rows.dtype, device=rows.device)
    return out.index_add_(0, i0, rows)


def relative_position_index(coord, index_0, index_1, window_size, quant_size, table_rows):
    """(M, 3) int32 of WindowAttention.forward (:163-169), torch's CPU fp32 values (ptv3_strat_rel_index)."""
    return ops.strat_rel_index(coord, index_0, index_1, window_size, quant_size, table_rows)


_ABSENT = ("grouping", "attention_step1", "attention_step2", "attention_step2_v2", "dot_prod_with_idx",
           "dot_prod_with_idx_v2", "attention_step2_with_rel_pos_value", "Divide2Patch", "subtraction", "aggregation",
           "interpolation_v2", "interpolation2")


def __getattr__(name):
    if name in _ABSENT:
        def absent(*args, **kwargs):
            raise NotImplementedError(f"pointops2.pointops.{name} is not built on the HIP path (ST-v1m2 does not call it)")
        absent.__name__ = name
        return absent
    raise AttributeError(name)
