from .builder import LOSSES, Criteria, build_criteria  # noqa: F401
from .misc import CrossEntropyLoss, FocalLoss  # noqa: F401
from .lovasz import LovaszLoss  # noqa: F401
from .weight_regression_loss import RegressionL1Loss  # noqa: F401
