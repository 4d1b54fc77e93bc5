"""`pointops2` (the reference's libs/pointops2) over libptv3_hip.so: see pointops2.pointops."""
from . import pointops  # noqa: F401
