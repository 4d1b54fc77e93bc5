from .concerto_v1m1_base import Concerto  # noqa: F401
