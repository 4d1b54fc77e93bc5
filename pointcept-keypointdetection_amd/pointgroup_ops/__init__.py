"""pointgroup_ops on MI355X: the two functions of the reference's libs/pointgroup_ops (functions/functions.py) over
libptv3_hip.so (csrc/pointgroup.hip, csrc/pg_bfs_host.cpp).  The CUDA library cannot be built here: parity unpinned.

ballquery_batch_p(coords, batch_idxs, batch_offsets, radius, meanActive) -> (idx (nActive) int32, start_len (n, 2) int32)
    on the device.  meanActive only sized the reference's first guess (functions.py:26-35); the count pass here sizes
    idx exactly, so it is accepted and ignored.  `start` is the exclusive scan of the counts by point index, one of the
    orders the reference's atomicAdd can produce.
bfs_cluster(semantic_label, ball_query_idxs, start_len, threshold) -> (cluster_idxs (sum, 2) int32, cluster_offsets)
    on CPU tensors.  One deviation: the members of a cluster come in ascending index, not in the search's discovery
    order (no caller in the reference tree reads the inner order), so the list path and the on-device clustering of the
    model return the same tensors.
"""
import torch

from ptv3_hip import ops as _ops


def ballquery_batch_p(coords, batch_idxs, batch_offsets, radius, meanActive):
    assert coords.is_contiguous() and coords.is_cuda
    assert batch_idxs.is_contiguous() and batch_idxs.is_cuda
    assert batch_offsets.is_contiguous() and batch_offsets.is_cuda
    return _ops.pg_ballquery_batch_p(coords, batch_idxs, batch_offsets, radius)


def bfs_cluster(semantic_label, ball_query_idxs, start_len, threshold):
    assert semantic_label.is_contiguous() and ball_query_idxs.is_contiguous() and start_len.is_contiguous()
    idxs, offsets = _ops.pg_bfs_cluster_host(semantic_label, ball_query_idxs, start_len, threshold)
    return _ops.pg_sort_members(idxs), offsets


__all__ = ["ballquery_batch_p", "bfs_cluster"]
