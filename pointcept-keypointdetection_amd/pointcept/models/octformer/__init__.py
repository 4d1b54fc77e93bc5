from .octformer_v1m1_base import OctFormer  # noqa: F401
