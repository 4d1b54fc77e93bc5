from .point_group_v1m1_base import PointGroup  # noqa: F401
from .point_group_v1m2_custom_criteria import PointGroupV1m2  # noqa: F401
