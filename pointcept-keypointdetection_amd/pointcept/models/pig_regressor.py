"""PigBodyRegressor: the fork's body-size-and-weight regression (pointcept/models/pig_regressor.py:15-57, built by
configs/my_dataset/ptv3_weight.py:40-77).  A DefaultClassifier with seven outputs whose result dict also carries, whenever
the batch has "category", the mean absolute error of each column in physical units (prediction and target times 100):
e_Len, e_Wid, e_Hei, e_Che, e_Wai, e_Hip, e_Wei - detached 0-d device tensors, nothing is read back.

The reference taps the logits with a forward hook on `cls_head`; here they are at hand, and with RegressionL1Loss as the
only criterion the head kernel has already reduced the seven columns (csrc/cls_head.hip), so no hook is registered - a
user's own hooks on the head still fire, because a hooked head takes the composed path (DefaultClassifier._head_plain).
"""
import torch

from .builder import MODELS
from .default import DefaultClassifier

ERROR_KEYS = ("e_Len", "e_Wid", "e_Hei", "e_Che", "e_Wai", "e_Hip", "e_Wei")


@MODELS.register_module()
class PigBodyRegressor(DefaultClassifier):
    metric_scale = 100.0

    def forward(self, input_dict):
        result, logits, stats = self._forward(input_dict)
        if "category" in input_dict:
            if stats is not None and self.num_classes == 7:
                errors = stats.detach()[1:]
            else:
                with torch.no_grad():
                    pred_real = logits.detach().view(-1, 7) * 100.0
                    target_real = input_dict["category"].view(-1, 7) * 100.0
                    errors = torch.abs(pred_real - target_real).mean(dim=0)
            for i, key in enumerate(ERROR_KEYS):
                result[key] = errors[i]
        return result
