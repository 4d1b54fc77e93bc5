"""CosineScheduler (reference: pointcept/utils/scheduler.py:156-199): the value schedules that "Sonata-v1m1" steps once
per iteration - a linear warm-up from start_value to base_value, half a cosine from base_value to final_value, an
optional frozen tail - tabulated once."""
import numpy as np


class CosineScheduler:
    def __init__(self, base_value, final_value, total_iters, start_value=0, warmup_iters=0, freeze_value=None,
                 freeze_iters=0):
        self.base_value = base_value
        self.final_value = final_value
        self.total_iters = total_iters
        self.iter = 0
        decay_iters = total_iters - warmup_iters - freeze_iters
        phase = np.pi * np.arange(decay_iters) / decay_iters if decay_iters > 0 else np.zeros(0)
        self.schedule = np.concatenate((
            np.linspace(start_value, base_value, warmup_iters),                      # ends ON base_value
            final_value + 0.5 * (base_value - final_value) * (1 + np.cos(phase)),     # starts on it again
            np.full(freeze_iters, final_value if freeze_value is None else freeze_value),
        ))

    def get(self, it):
        return self.final_value if it >= self.total_iters else self.schedule[it]

    def step(self):
        value = self.get(self.iter)
        self.iter += 1
        return value

    def reset(self):
        self.iter = 0

    def __getitem__(self, it):
        return self.get(it)
