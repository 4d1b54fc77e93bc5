"""Only what pointcept/models/modules.py needs from the hook package (reference: engines/hooks/default.py)."""


class HookBase:
    """Base class for hooks; PointModel subclasses it (models/modules.py:114-120 in the reference)."""

    trainer = None

    def before_train(self):
        pass

    def before_epoch(self):
        pass

    def before_step(self):
        pass

    def after_step(self):
        pass

    def after_epoch(self):
        pass

    def after_train(self):
        pass


# the evaluator hooks register themselves with HOOKS on import, as in the reference (engines/hooks/__init__.py:7-8)
from .keypoint_evaluator import KeypointEvaluator  # noqa: E402,F401
from .offset_keypoint_evaluator import OffsetKeypointEvaluator  # noqa: E402,F401
from .default import ModelHook  # noqa: E402,F401
from .evaluator import ClsEvaluator, SemSegEvaluator, InsSegEvaluator  # noqa: E402,F401
