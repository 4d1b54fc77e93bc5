"""Point Transformer V1 pieces on MI355X (the encoder side that KeypointPTv1 uses)."""
from .point_transformer_seg import PointTransformerLayer, TransitionDown, Bottleneck  # noqa: F401
