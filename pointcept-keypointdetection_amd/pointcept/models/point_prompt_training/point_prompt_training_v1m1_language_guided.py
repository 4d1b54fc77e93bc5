"""Point Prompt Training with language-guided categorical alignment ("PPT-v1m1", reference
pointcept/models/point_prompt_training/point_prompt_training_v1m1_language_guided.py).

Constructor keywords, defaults, backbone_mode, state_dict (`class_embedding`, `logit_scale`, `proj_head.*`,
`embedding_table.weight`, `backbone.*`) and the three result dicts are the reference's.  Of its backbones only "PT-v3m1"
exists here (with PDNorm, prompt_driven_normalization.py).

CLIP: the class embeddings are CLIP's text encoding of the class names.  Where `clip` is importable they are computed as
in the reference (:61-77).  Where it is not, `class_embedding` is registered as zeros of (len(class_name), D) with D
from CLIP_TEXT_WIDTH and `logit_scale` as a frozen parameter at ln(100), and the model expects them from a reference
checkpoint (load_state_dict) or from set_class_embedding(); a forward before either raises.

Head (:98-107): seg_logits = exp(logit_scale) * normalize(proj_head(feat)) @ class_embedding[valid_index[cond]].T.  In
eval nothing nonlinear separates the two matrices, so the D-wide intermediate is collapsed away once per weights
(ops.ppt_head_collapse) and the head is one (N, C) x (C, C + K) product with a row-norm epilogue:
csrc/ppt_head.hip where `wired` says it measured ahead, else the better torch composition.  Training composes proj_head
(the library's Linear), the norm and the product in torch: a fused training head would need the factorisation and its
derivative every step.  set_fused(False), a hook on proj_head, a CPU tensor or features that require a gradient compose
the reference's statement order.
"""
import importlib.util
import math

import torch
import torch.nn as nn

from pointcept.models.utils.structure import Point
from pointcept.models.utils.hip_layers import Linear
from pointcept.models.utils.sparse import _ParamCache
from pointcept.models.builder import MODELS
from pointcept.models.losses import build_criteria
from ptv3_hip import ops

# width of the text space per CLIP model name, used only where `clip` is not importable; a caller with a checkpoint of
# another CLIP model adds its entry
CLIP_TEXT_WIDTH = {"ViT-B/16": 512, "ViT-B/32": 512, "ViT-L/14": 768}


def wired(k, c, n):
    """Which form the eval head takes at K valid classes, C channels, n rows: "kernel" (ptv3_ppt_head_fwd),
    "collapsed" (the collapsed operands composed in torch) or "reference" (the reference's statement order).  By the
    wiring rule the kernel is called only where it measured ahead of the better composition on an MI355X
    (tools/bench_ppt.py, profiles/ppt/): at every measured shape - K in {13, 20, 25, 36, 200},
    C in {64, 96}, D = 512, at 10 000, 100 000 and 1 000 000 rows.  Between the measured shapes the rule extrapolates
    downwards in K and C only (a (K, C) is wired when a measured shape with at least its K and its C is ahead) and not
    below the fewest measured rows.  Elsewhere the collapsed composition runs: it measured ahead of the reference order
    at every shape, and past the measured shapes it is the same arithmetic with fewer products."""
    if n >= 10000 and k <= 200 and c <= 96:
        return "kernel"
    return "collapsed"


def head_reference(feat, weight, bias, e_v, logit_scale):
    """:98-107 in the reference's statement order, in torch"""
    h = torch.nn.functional.linear(feat, weight, bias)
    h = h / h.norm(dim=-1, keepdim=True)
    return logit_scale.exp() * (h @ e_v.t())


def head_collapsed(x, B, bias, beta, s):
    """the collapsed operands composed in torch: one product, the row norm of its first C columns, one division"""
    c = x.shape[1]
    y = torch.addmm(bias, x, B)
    z = y[:, :c]
    return y[:, c:] * (s / torch.sqrt((z * z).sum(1, keepdim=True) + beta))


def _backbone_type(backbone):
    return backbone["type"] if isinstance(backbone, dict) else backbone.type


def _condition(data_dict):
    condition = data_dict["condition"]
    return condition if isinstance(condition, str) else condition[0]


class _PromptBase(nn.Module):
    """what PPT-v1m1 and PPT-v1m2 share (:52-59, :80-97): the backbone, the criteria, the context embedding"""

    def _init_base(self, backbone, criteria, context_channels, conditions, backbone_mode):
        assert _backbone_type(backbone) in ["SpUNet-v1m3", "PT-v2m3", "PT-v3m1"]
        self.backbone = MODELS.build(backbone)
        self.criteria = build_criteria(criteria)
        self.conditions = conditions
        self.embedding_table = nn.Embedding(len(conditions), context_channels)
        self.backbone_mode = backbone_mode
        self._fused = True
        self._index = {}

    def set_fused(self, on=True):
        """False: the head in the reference's statement order."""
        self._fused = bool(on)
        return self

    def _features(self, data_dict):
        """(index of the condition, backbone features) - :80-94"""
        condition = _condition(data_dict)
        if condition not in self.conditions:
            raise KeyError(f"{type(self).__name__}: condition {condition!r} is not one of {tuple(self.conditions)}")
        index = list(self.conditions).index(condition)
        device = data_dict["coord"].device
        key = (index, device)
        if key not in self._index:
            self._index[key] = torch.tensor([index], device=device)
        data_dict["context"] = self.embedding_table(self._index[key])
        data_dict["context_source"] = self.embedding_table.weight     # what SpUNet-v1m3 keys its cached folds on
        point = self.backbone(data_dict)
        return index, (point.feat if isinstance(point, Point) else point)

    def _result(self, seg_logits, data_dict):
        if self.training:
            return dict(loss=self.criteria(seg_logits, data_dict["segment"]))
        if "segment" in data_dict.keys():
            return dict(loss=self.criteria(seg_logits, data_dict["segment"]), seg_logits=seg_logits)
        return dict(seg_logits=seg_logits)


@MODELS.register_module("PPT-v1m1")
class PointPromptTraining(_PromptBase):
    def __init__(
        self,
        backbone=None,
        criteria=None,
        backbone_out_channels=96,
        context_channels=256,
        conditions=("Structured3D", "ScanNet", "S3DIS"),
        template="[x]",
        clip_model="ViT-B/16",
        # fmt: off
        class_name=(
            "wall", "floor", "cabinet", "bed", "chair", "sofa", "table", "door",
            "window", "bookshelf", "bookcase", "picture", "counter", "desk", "shelves", "curtain",
            "dresser", "pillow", "mirror", "ceiling", "refrigerator", "television", "shower curtain", "nightstand",
            "toilet", "sink", "lamp", "bathtub", "garbagebin", "board", "beam", "column",
            "clutter", "otherstructure", "otherfurniture", "otherprop",
        ),
        valid_index=(
            (0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 23, 25, 26, 33, 34, 35),
            (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 15, 20, 22, 24, 25, 27, 34),
            (0, 1, 4, 5, 6, 7, 8, 10, 19, 29, 30, 31, 32),
        ),
        # fmt: on
        backbone_mode=False,
    ):
        super().__init__()
        assert len(conditions) == len(valid_index)
        self._init_base(backbone, criteria, context_channels, conditions, backbone_mode)
        self.valid_index = valid_index
        self._filled = False
        if not self.backbone_mode:
            if importlib.util.find_spec("clip") is not None:
                import clip
                model, _ = clip.load(clip_model, device="cpu", download_root="./.cache/clip")
                model.requires_grad_(False)
                class_token = clip.tokenize([template.replace("[x]", name) for name in class_name])
                class_embedding = model.encode_text(class_token)
                class_embedding = class_embedding / class_embedding.norm(dim=-1, keepdim=True)
                width, logit_scale = model.text_projection.shape[1], model.logit_scale
                self._filled = True
            else:
                if clip_model not in CLIP_TEXT_WIDTH:
                    raise KeyError(f"PPT-v1m1: clip is not importable and the text width of {clip_model!r} is not in "
                                   f"CLIP_TEXT_WIDTH {sorted(CLIP_TEXT_WIDTH)}")
                width = CLIP_TEXT_WIDTH[clip_model]
                class_embedding = torch.zeros(len(class_name), width)
                logit_scale = nn.Parameter(torch.tensor(math.log(100.0)), requires_grad=False)
            self.register_buffer("class_embedding", class_embedding)
            self.proj_head = Linear(backbone_out_channels, width)
            self.logit_scale = logit_scale
            self._collapse_cache = _ParamCache()

    def set_class_embedding(self, class_embedding, logit_scale=None):
        """Fills `class_embedding` (len(class_name), D; rows as CLIP's encode_text gives them, normalised here as :70-72)
        and optionally `logit_scale` (CLIP's: the logarithm of the scale) by hand."""
        class_embedding = torch.as_tensor(class_embedding, dtype=torch.float32)
        if tuple(class_embedding.shape) != tuple(self.class_embedding.shape):
            raise ValueError(f"set_class_embedding: got {tuple(class_embedding.shape)}, expected "
                             f"{tuple(self.class_embedding.shape)}")
        with torch.no_grad():
            class_embedding = class_embedding / class_embedding.norm(dim=-1, keepdim=True)
            self.class_embedding.copy_(class_embedding.to(self.class_embedding.device))
            if logit_scale is not None:
                self.logit_scale.copy_(torch.as_tensor(float(logit_scale)))
        self._filled = True
        return self

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        if prefix + "class_embedding" in state_dict:
            self._filled = True
        return super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _valid(self, index):
        key = (index, self.class_embedding.device)
        if ("v",) + key not in self._index:
            self._index[("v",) + key] = torch.tensor(list(self.valid_index[index]), device=self.class_embedding.device)
        return self._index[("v",) + key]

    def collapsed(self, index):
        """(B, bias, beta, s) of condition `index`, cached on the versions and storages of proj_head.weight, proj_head.bias,
        class_embedding and logit_scale: an optimizer step or a load_state_dict rebuilds them (one host round trip), a
        forward on unchanged weights reads nothing back.  (R, q, beta) is kept per weights, (M, c) per condition."""
        head = self.proj_head
        qr = self._collapse_cache.get("qr", [head.weight, head.bias], lambda: ops.ppt_head_qr(head.weight, head.bias))
        return self._collapse_cache.get(
            ("cond", index, head.weight.device), [head.weight, head.bias, self.class_embedding, self.logit_scale],
            lambda: ops.ppt_head_collapse(head.weight, head.bias, self.class_embedding[self._valid(index)],
                                          self.logit_scale, qr=qr))

    def _hooked(self):
        m = self.proj_head
        return bool(m._forward_hooks or m._forward_pre_hooks or m._backward_hooks)

    def head(self, feat, index):
        """feat (N, C) -> seg_logits (N, K) in fp32; under autocast the features are upcast and autocast is off"""
        if not self._filled:
            raise RuntimeError("PPT-v1m1: class_embedding was never filled (CLIP is not importable here): load a "
                               "reference checkpoint with load_state_dict (keys class_embedding, logit_scale), or call "
                               "set_class_embedding(tensor, logit_scale=None)")
        with torch.autocast(device_type=feat.device.type, enabled=False):
            feat = feat.float().contiguous()
            head = self.proj_head
            k, c = len(self.valid_index[index]), feat.shape[1]
            collapse = (self._fused and not self.training and feat.is_cuda and not self._hooked()
                        and not (torch.is_grad_enabled() and feat.requires_grad))
            form = wired(k, c, feat.shape[0]) if collapse else "reference"
            if form == "kernel" and not ops.ppt_head_capable(c, k):
                form = "collapsed"
            if form == "reference":
                h = head(feat)
                h = h / h.norm(dim=-1, keepdim=True)
                return self.logit_scale.exp() * (h @ self.class_embedding[self._valid(index)].t())
            B, bias, beta, s = self.collapsed(index)
            if form == "kernel":
                return ops.ppt_head(feat, B, bias, beta, s)
            return head_collapsed(feat, B, bias, beta, s)

    def forward(self, data_dict):
        index, feat = self._features(data_dict)
        if self.backbone_mode:
            # PPT serve as a multi-dataset backbone when enable backbone mode
            return feat
        return self._result(self.head(feat, index), data_dict)
