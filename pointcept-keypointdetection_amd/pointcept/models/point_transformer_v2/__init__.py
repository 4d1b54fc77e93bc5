"""Point Transformer V2 (the reference's pointcept/models/point_transformer_v2 package; mode 2 only)."""
from .point_transformer_v2m2_base import PointTransformerV2  # noqa: F401
