"""Numpy restatements, written from the algorithm, of what the evaluator kernels and InsSegEvaluator count.

  confusion(pred, target, k, ignore)         the three histograms of a semantic evaluation, by bincount
  argmax_first(logits)                       the lowest index among a row's maxima
  codes(segment, instance, ...)              ground-truth instances of a scene and the per-point code
  associate(masks, code, g, idx)             inter (P, G + 1), vert_count (P), void_intersection (P), one proposal at a time
  scene_tables(masks, classes, segment, ...) the same, straight from labels: one pass per (proposal, instance)
  pairs(...)                                 (kept proposal, ground-truth id, intersection) rows, as the fixture stores them
"""
import numpy as np

VOID = -2 ** 31


def argmax_first(logits):
    logits = np.asarray(logits, dtype=np.float64)
    best = logits.max(axis=1, keepdims=True)
    k = logits.shape[1]
    return np.where(logits == best, np.arange(k)[None], k).min(axis=1)


def confusion(pred, target, k, ignore_index):
    """(3, k) int64: intersection, predicted area, target area; a value outside [0, k) is counted nowhere."""
    pred = np.asarray(pred, dtype=np.int64).copy()
    target = np.asarray(target, dtype=np.int64)
    pred[target == ignore_index] = ignore_index

    def hist(x):
        return np.bincount(x[(x >= 0) & (x < k)], minlength=k)[:k]

    return np.stack([hist(pred[pred == target]), hist(pred), hist(target)]).astype(np.int64)


def codes(segment, instance, segment_ignore_index, instance_ignore_index):
    """(code (N) int32, gt_id (G), gt_class (G), gt_count (G)): the instances in ascending id, without the ignored id
    and without those whose first point lies on an ignored segment; code = the compact index of the point's instance, or
    G, plus VOID where the point's own segment is ignored."""
    segment, instance = np.asarray(segment), np.asarray(instance)
    ids = sorted(set(instance.tolist()))
    gt_id, gt_class, gt_count = [], [], []
    code = np.full(instance.shape[0], -1, dtype=np.int64)
    for i in ids:
        where = np.flatnonzero(instance == i)
        cls = int(segment[where[0]])
        if i == instance_ignore_index or cls in segment_ignore_index:
            continue
        code[where] = len(gt_id)
        gt_id.append(i)
        gt_class.append(cls)
        gt_count.append(len(where))
    code[code < 0] = len(gt_id)
    code[np.isin(segment, list(segment_ignore_index))] += VOID
    return code.astype(np.int32), np.array(gt_id, dtype=np.int64), np.array(gt_class, dtype=np.int64), \
        np.array(gt_count, dtype=np.int64)


def associate(masks, code, g, idx=None):
    masks = np.asarray(masks)
    code = np.asarray(code).astype(np.int64)
    p = masks.shape[0]
    inter = np.zeros((p, g + 1), dtype=np.int64)
    vert = np.zeros(p, dtype=np.int64)
    void = np.zeros(p, dtype=np.int64)
    col = code & 0x7FFFFFFF
    is_void = code < 0
    for i in range(p):
        row = masks[i] != 0
        if idx is not None:
            row = row[np.asarray(idx)]
        inter[i] = np.bincount(col[row], minlength=g + 1)[: g + 1]
        vert[i] = row.sum()
        void[i] = (row & is_void).sum()
    return inter, vert, void


def scene_tables(masks, segment, instance, segment_ignore_index, instance_ignore_index, idx=None):
    """inter (P, G), vert_count, void_intersection, gt_id, gt_class, gt_count from the labels, one pass per pair."""
    masks = np.asarray(masks) != 0
    if idx is not None:
        masks = masks[:, np.asarray(idx)]
    segment, instance = np.asarray(segment), np.asarray(instance)
    _, gt_id, gt_class, gt_count = codes(segment, instance, segment_ignore_index, instance_ignore_index)
    void_mask = np.isin(segment, list(segment_ignore_index))
    inter = np.array([[np.count_nonzero(m & (instance == i)) for i in gt_id] for m in masks], dtype=np.int64)
    inter = inter.reshape(masks.shape[0], len(gt_id))
    vert = np.array([np.count_nonzero(m) for m in masks], dtype=np.int64)
    void = np.array([np.count_nonzero(m & void_mask) for m in masks], dtype=np.int64)
    return dict(inter=inter, vert_count=vert, void_intersection=void, gt_id=gt_id, gt_class=gt_class, gt_count=gt_count)


def kept(vert_count, pred_classes, segment_ignore_index, min_region=100):
    ok = (np.asarray(vert_count) >= min_region) & ~np.isin(np.asarray(pred_classes), list(segment_ignore_index))
    return np.flatnonzero(ok)


def pairs(scene, pred_classes, segment_ignore_index, min_region=100):
    """Rows (position among the kept proposals, ground-truth instance id, intersection) for every kept proposal and every
    instance of its class it touches, in instance-id order."""
    rows = []
    for k, p in enumerate(kept(scene["vert_count"], pred_classes, segment_ignore_index, min_region)):
        for g in np.flatnonzero(scene["gt_class"] == pred_classes[p]):
            if scene["inter"][p, g] > 0:
                rows.append((k, int(scene["gt_id"][g]), int(scene["inter"][p, g])))
    return np.array(rows, dtype=np.int64).reshape(-1, 3)
