"""numpy restatements of PointGroup's evaluation tail, written from the algorithm: the brute ball
query with its cap, the directed breadth-first search in discovery order, and the proposal filter with float64 scores.
Shared by tests/test_pointgroup_cpu.py, tests/test_hip_pointgroup.py and tests/golden/make_golden_pointgroup.py."""
import numpy as np

CAP = 1000


def ball_query(xyz, batch_idxs, batch_offsets, radius, cap=CAP):
    """(idx (nActive) int32, start_len (n, 2) int32).  Point i's list: the rows k of its scene with d2 < radius^2 in
    ascending k, the first `cap` of them; d2 = ((xi-xk)^2 + (yi-yk)^2) + (zi-zk)^2 in float32, one rounding per operation;
    radius^2 in float32; start = the exclusive scan of the counts by point index."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    n = xyz.shape[0]
    r2 = np.float32(radius) * np.float32(radius)
    lists, start_len = [], np.zeros((n, 2), dtype=np.int32)
    at = 0
    for i in range(n):
        s = int(batch_idxs[i])
        lo, hi = int(batch_offsets[s]), int(batch_offsets[s + 1])
        d = xyz[i][None, :] - xyz[lo:hi]
        sq = d * d
        d2 = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
        hits = (np.nonzero(d2 < r2)[0][:cap] + lo).astype(np.int32)
        lists.append(hits)
        start_len[i] = (at, hits.shape[0])
        at += hits.shape[0]
    idx = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int32)
    return idx.astype(np.int32), start_len


def neighbour_counts(xyz, batch_idxs, batch_offsets, radius):
    """true (uncapped) neighbour count of every point"""
    return ball_query(xyz, batch_idxs, batch_offsets, radius, cap=1 << 30)[1][:, 1]


def bfs_cluster(label, idx, start_len, threshold):
    """(cluster_idxs (sum, 2) int32, cluster_offsets (clusters + 1) int32) of the directed search: seeds in ascending
    index; a seed's component is everything reachable through same-label list entries that no earlier component took;
    members in discovery order (first in, first out); components with fewer than `threshold` members are dropped."""
    n = start_len.shape[0]
    taken = np.zeros(n, dtype=bool)
    rows, offsets = [], [0]
    for seed in range(n):
        if taken[seed]:
            continue
        taken[seed] = True
        comp, head = [seed], 0
        while head < len(comp):
            cur = comp[head]
            head += 1
            s, c = int(start_len[cur, 0]), int(start_len[cur, 1])
            for j in idx[s:s + c]:
                j = int(j)
                if not taken[j] and label[j] == label[cur]:
                    taken[j] = True
                    comp.append(j)
        if len(comp) >= threshold:
            cid = len(offsets) - 1
            rows.extend((cid, m) for m in comp)
            offsets.append(offsets[-1] + len(comp))
    return (np.array(rows, dtype=np.int32).reshape(-1, 2), np.array(offsets, dtype=np.int32))


def sort_members(cluster_idxs, cluster_offsets):
    """every cluster's members in ascending index (the order the device clustering writes)"""
    out = cluster_idxs.copy()
    for c in range(cluster_offsets.shape[0] - 1):
        b, e = int(cluster_offsets[c]), int(cluster_offsets[c + 1])
        out[b:e, 1] = np.sort(cluster_idxs[b:e, 1])
    return out


def cluster(xyz, label, batch_offsets, radius, min_points):
    batch = np.repeat(np.arange(len(batch_offsets) - 1), np.diff(batch_offsets)).astype(np.int32)
    idx, start_len = ball_query(xyz, batch, batch_offsets, radius)
    return bfs_cluster(label, idx, start_len, min_points)


def proposals(cluster_idxs, cluster_offsets, prob, segment_pred, propose_points, row_map=None):
    """(pred_classes (P) int64, pred_scores (P) float64, members: list of P sorted row arrays): the clusters with MORE than
    propose_points members; class = segment_pred of the first listed member; score = the float64 mean over the members
    of prob[row, class]."""
    classes, scores, members = [], [], []
    for c in range(cluster_offsets.shape[0] - 1):
        b, e = int(cluster_offsets[c]), int(cluster_offsets[c + 1])
        if e - b <= propose_points:
            continue
        rows = cluster_idxs[b:e, 1].astype(np.int64)
        if row_map is not None:
            rows = np.asarray(row_map)[rows]
        cls = int(segment_pred[rows[0]])
        classes.append(cls)
        scores.append(np.asarray(prob, dtype=np.float64)[rows, cls].mean())
        members.append(np.sort(rows))
    return np.array(classes, dtype=np.int64), np.array(scores, dtype=np.float64), members
