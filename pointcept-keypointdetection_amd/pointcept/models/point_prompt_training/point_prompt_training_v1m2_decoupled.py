"""Point Prompt Training with a decoupled segmentation head per condition ("PPT-v1m2", reference
pointcept/models/point_prompt_training/point_prompt_training_v1m2_decoupled.py): constructor keywords, defaults,
backbone_mode, state_dict (`seg_heads.{i}.*`, `embedding_table.weight`, `backbone.*`) and result dicts are the
reference's; the heads are the library's Linear.  Under autocast the head runs in fp32 with autocast off."""
import torch
import torch.nn as nn

from pointcept.models.utils.hip_layers import Linear
from pointcept.models.builder import MODELS
from .point_prompt_training_v1m1_language_guided import _PromptBase


@MODELS.register_module("PPT-v1m2")
class PointPromptTrainingDecoupled(_PromptBase):
    def __init__(self, backbone=None, criteria=None, backbone_out_channels=96, context_channels=256,
                 conditions=("Structured3D", "ScanNet", "S3DIS"), num_classes=(25, 20, 13), backbone_mode=False):
        super().__init__()
        assert len(conditions) == len(num_classes)
        self._init_base(backbone, criteria, context_channels, conditions, backbone_mode)
        self.seg_heads = nn.ModuleList([Linear(backbone_out_channels, num_cls) for num_cls in num_classes])

    def forward(self, data_dict):
        index, feat = self._features(data_dict)
        if self.backbone_mode:
            return feat
        with torch.autocast(device_type=feat.device.type, enabled=False):
            seg_logits = self.seg_heads[index](feat.float().contiguous())
        return self._result(seg_logits, data_dict)
