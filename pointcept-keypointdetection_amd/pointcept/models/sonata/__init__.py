from .sonata_v1m1_base import OnlineCluster, Sonata  # noqa: F401
