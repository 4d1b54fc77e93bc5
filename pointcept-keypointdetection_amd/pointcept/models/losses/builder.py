"""Loss registry + the `Criteria` aggregate the segmentor wrappers call (interface of the reference's
pointcept/models/losses/builder.py).  CrossEntropyLoss is plain torch (one fused launch there already); LovaszLoss and
FocalLoss run HIP kernels on a GPU prediction (csrc/seg_loss.hip), because the reference's
Lovasz composition is hundreds of small launches and one host read per class.  The registry exists so
DefaultSegmentor / DefaultSegmentorV2 configs build unchanged."""
from functools import reduce

from pointcept.utils.registry import Registry

LOSSES = Registry("losses")


class Criteria:
    """Sum of the configured losses; with no loss configured the prediction passes through (the model computes
    its own loss, as OffsetKeypointPTv3 does)."""

    def __init__(self, cfg=None):
        self.cfg = list(cfg) if cfg else []
        self.criteria = [LOSSES.build(cfg=c) for c in self.cfg]

    def __call__(self, pred, target):
        if not self.criteria:
            return pred
        return reduce(lambda acc, fn: acc + fn(pred, target), self.criteria, 0)


def build_criteria(cfg):
    return Criteria(cfg)
