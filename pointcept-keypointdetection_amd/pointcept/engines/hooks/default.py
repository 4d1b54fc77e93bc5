"""HookBase and ModelHook (reference: pointcept/engines/hooks/default.py:13-66)."""
import weakref

from pointcept.utils import comm
from . import HookBase  # noqa: F401
from .builder import HOOKS


@HOOKS.register_module()
class ModelHook(HookBase):
    """Forwards the trainer's six callbacks to a model that is itself a HookBase (a PointModel such as "Sonata-v1m1",
    which steps its schedules and its teacher there); any other model gets an inert HookBase.  Under DistributedDataParallel
    the model is the wrapper's `.module`."""

    def before_train(self):
        model = self.trainer.model
        if comm.get_world_size() > 1 and isinstance(getattr(model, "module", None), HookBase):
            model = model.module
        self.model = weakref.proxy(model) if isinstance(model, HookBase) else HookBase()
        self.model.trainer = self.trainer
        self.model.before_train()

    def before_epoch(self):
        self.model.before_epoch()

    def before_step(self):
        self.model.before_step()

    def after_step(self):
        self.model.after_step()

    def after_epoch(self):
        self.model.after_epoch()

    def after_train(self):
        self.model.after_train()
