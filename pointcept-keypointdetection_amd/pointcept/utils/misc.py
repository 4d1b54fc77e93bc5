"""Segmentation counts of the evaluators (reference: pointcept/utils/misc.py:38-65), names and signatures kept."""
import numpy as np
import torch

from ptv3_hip import ops

# Shapes at which ptv3_seg_confusion measured ahead of the torch composition by more than the run-to-run spread
# (tools/bench_evaluator.py): every shape timed, from 10 000 elements up; below that nothing was
# timed and the composition stays.
SEG_CONFUSION_MIN_ELEMENTS = 10_000


def seg_confusion_wired(n_elements, k):
    return n_elements >= SEG_CONFUSION_MIN_ELEMENTS and k <= ops.SEG_CONFUSION_MAX_K


def intersection_and_union(output, target, K, ignore_index=-1):
    """(intersection, union, target) areas of K classes from numpy label arrays of 1 to 3 dimensions (:38-50)."""
    assert output.ndim in [1, 2, 3]
    assert output.shape == target.shape
    output = output.reshape(output.size).copy()
    target = target.reshape(target.size)
    output[target == ignore_index] = ignore_index
    bins = np.arange(K + 1)
    area_intersection = np.histogram(output[output == target], bins=bins)[0]
    area_output = np.histogram(output, bins=bins)[0]
    area_target = np.histogram(target, bins=bins)[0]
    return area_intersection, area_output + area_target - area_intersection, area_target


def confusion_counts(src, target, k, ignore_index=-1, inverse=None, counts=None):
    """(3, K) int64 = intersection, predicted area, target area on the inputs' device, added to `counts` when given:
    the kernel at the shapes where it is wired, the torch composition elsewhere and for CPU tensors."""
    if src.is_cuda and seg_confusion_wired(target.numel(), k):
        return ops.seg_confusion(src.contiguous(), target.contiguous(), k, ignore_index,
                                 None if inverse is None else inverse.contiguous(), counts)
    return ops.seg_confusion_torch(src, target, k, ignore_index, inverse, counts)


def intersection_and_union_gpu(output, target, k, ignore_index=-1):
    """(intersection, union, target) areas, each (k) on the inputs' device (:53-65).  As in the reference `output` takes
    ignore_index where `target` has it, in place.  The areas are int64 (the reference's histc keeps the label dtype)."""
    assert output.dim() in [1, 2, 3]
    assert output.shape == target.shape
    output = output.view(-1)
    target = target.view(-1)
    output[target == ignore_index] = ignore_index
    area_intersection, area_output, area_target = confusion_counts(output, target, k, ignore_index)
    return area_intersection, area_output + area_target - area_intersection, area_target
