"""Prompt-driven normalisation (reference: pointcept/models/point_prompt_training/prompt_driven_normalization.py).

One plain norm per dataset condition (`norm.{i}.*`), chosen by `point.condition` (a string, or a list whose first entry
counts); with adaptive=True the result is modulated by `feat * (1 + scale) + shift`, (shift, scale) =
modulation(point.context) (`modulation.1.*`).  The norms are the library's BatchNorm1d / LayerNorm, so a non-adaptive
PDNorm is, per forward, exactly one of them: `resolve_norm` hands that one to the places of PT-v3m1 that fuse a norm into
a neighbouring kernel.  A norm built without affine parameters (pdnorm_affine=False) has no
kernel form here and is composed in torch.
"""
import torch.nn as nn
import torch.nn.functional as F

from pointcept.models.modules import PointModule
from pointcept.models.builder import MODULES


@MODULES.register_module()
class PDNorm(PointModule):
    def __init__(self, num_features, norm_layer, context_channels=256,
                 conditions=("ScanNet", "S3DIS", "Structured3D"), decouple=True, adaptive=False):
        super().__init__()
        if not decouple:
            # the reference stores the un-called `norm_layer` partial as self.norm (:25) and then calls it on the
            # features (:42): that forward cannot run there either
            raise ValueError("PDNorm(decouple=False) cannot run in the reference (it keeps the norm's constructor, not a "
                             "norm, and calls it on the features); use decouple=True")
        self.conditions = conditions
        self.decouple = decouple
        self.adaptive = adaptive
        self.norm = nn.ModuleList([norm_layer(num_features) for _ in conditions])
        if self.adaptive:
            self.modulation = nn.Sequential(nn.SiLU(), nn.Linear(context_channels, 2 * num_features, bias=True))

    def active(self, point):
        """the plain norm of the point's condition"""
        assert "condition" in point.keys()
        condition = point.condition if isinstance(point.condition, str) else point.condition[0]
        if condition not in self.conditions:
            raise KeyError(f"PDNorm: condition {condition!r} is not one of {tuple(self.conditions)}")
        return self.norm[list(self.conditions).index(condition)]

    @staticmethod
    def _run_norm(norm, x):
        if getattr(norm, "weight", None) is not None:
            return norm(x)
        # no affine parameters: torch's own arithmetic
        if isinstance(norm, nn.LayerNorm):
            return F.layer_norm(x.float(), norm.normalized_shape, None, None, norm.eps).to(x.dtype)
        return nn.BatchNorm1d.forward(norm, x.float()).to(x.dtype)

    def forward(self, point):
        assert {"feat", "condition"}.issubset(point.keys())
        point.feat = self._run_norm(self.active(point), point.feat)
        if self.adaptive:
            assert "context" in point.keys()
            shift, scale = self.modulation(point.context.float()).chunk(2, dim=1)
            point.feat = (point.feat * (1.0 + scale) + shift).to(point.feat.dtype)
        return point


def resolve_norm(module, point):
    """A non-adaptive PDNorm whose active norm has affine parameters -> that plain norm; anything else unchanged.  The
    fused paths of PT-v3m1 test, fold and read `norm[0]`, `cpe[2]` and `proj[1]` through this."""
    if isinstance(module, PDNorm) and not module.adaptive and point is not None:
        norm = module.active(point)
        if getattr(norm, "weight", None) is not None:
            return norm
    return module
