from .oacnns_v1m1_base import OACNNs, BasicBlock, DonwBlock, UpBlock  # noqa: F401
