"""Concerto 2D-3D joint pretraining ("Concerto-v1m1", reference pointcept/models/concerto/concerto_v1m1_base.py) on "PT-v3m2".

Sonata's three self-distillation losses (models/sonata/sonata_v1m1_base.py: distill_loss, the masks, matches, roll and
up-cast are inherited) plus an image branch: the per-point pixel correspondences are pooled down the backbone's pooling
hierarchy, the student's up-cast features are averaged per image patch, projected, and pulled towards the features of a
frozen 2D encoder with a mean-shifted cosine loss.  Constructor keywords, defaults, module tree, state_dict keys, the
result dict and the hooks are the reference's.  What differs is how the image branch is evaluated:

  reference                                                      here
  pool_corr: per level and image a torch.sort and a dozen ops    the pooling's own (order, seg_start), one launch a level
  feature3d[valid rows] -> (pairs, C), scatter_mean into a       a patch plan (sort of the pairs by patch), then a
    dense (images * patches, C) matrix                             gather-mean into the U occupied patches only
  patch_proj over all images * patches rows, then the select     patch_proj (a plain nn.Linear) over the U rows
  shift, cosine and mean in about eight passes                   one pass per row each way, in float64

  - fused (csrc/concerto.hip): ptv3_concerto_pool_corr; ops.concerto_plan (ptv3_concerto_pair_keys, ptv3_argsort_i64,
    ptv3_pool_segments, ptv3_concerto_plan_finish); ptv3_concerto_patch_mean_fwd / _bwd; ptv3_concerto_cos_fwd / _bwd.
  - composed - set_fused(False), CPU tensors, features that are neither fp32 nor bf16, D outside
    ops.concerto_cos_capable, or a shape `wired` does not list: the same arithmetic in torch, occupied patches only.

The student's second forward: with exactly one of mask_loss_weight and roll_mask_loss_weight zero the reference runs the
student on the masked view again (:746-748), which repeats the computation with new random draws; the first result is
reused here.  Without an image in the batch (img_num sums to 0) enc2d_loss is the weighted average of the other losses
(:854-866).  With images but no valid correspondence the composed path runs over zero rows without a launch and
returns what the reference returns, the mean over nothing (NaN).

Host reads of a step beyond Sonata's: the image count (as the reference), and the number of occupied patches U (the run
count of the plan's sort; the reference reads the valid-pair selection and the unique patch list instead, as the
composed path here does).  The rows of the principal views come from the offsets the backbone already holds on the host.
"""
import os
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.distributed as dist

from pointcept.models.utils.structure import Point
from pointcept.models.builder import MODELS, build_model
from pointcept.models.modules import PointModel
from pointcept.models.utils import batch2offset
from pointcept.models.sonata.sonata_v1m1_base import Sonata, OnlineCluster as SonataCluster
from pointcept.utils.comm import get_world_size
from ptv3_hip import ops
from ptv3_hip import autograd as A


def wired(kernel, width, rows):
    """Which kernels the model calls: by the wiring rule only what measured ahead of the composed path on an MI355X by
    more than the run-to-run spread (profiles/concerto/; two runs within 4.8 %).  Measured at one
    rank's batch of the two pretraining configs - 480 000 level-0 points with V = 4 images a scene, 120 000 level-1 rows,
    C = 1184 and 1664, D = 1536, 21 074 occupied patches - in fp32 and bf16, forward and forward + backward:
      pool_corr   (width V, rows n_in)  one level: 15 times ahead of the composed path, 72 of the literal one;
      patch_mean  (width C, rows n)     plan + patch mean + projection: 1.28 - 1.30 (fp32) and 1.7 - 1.9 (bf16) ahead
                                        forward + backward, 1.5 - 2.6 forward;
      cos         (width D, rows U)     3.1 - 3.9 ahead forward, 2.6 - 4.5 forward + backward.
    Nothing smaller was measured, so nothing smaller is listed: the rule extrapolates only towards more rows, where the
    composed path's full-size passes and copies grow with the kernel's one pass, and between the two measured widths C;
    V = 4 and D = 1536 are the only values of theirs that were measured and the only ones listed."""
    if kernel == "pool_corr":
        return width == 4 and rows >= 480000
    if kernel == "patch_mean":
        return 1184 <= width <= 1664 and rows >= 120000
    if kernel == "cos":
        return width == 1536 and rows >= 21000
    raise KeyError(kernel)


# -- the composed path: the same arithmetic in torch, occupied patches only ------------------------------------------
def pool_corr_torch(corr, inverse, n_out):
    """one pooling level (:545-570): (n_in, V, 2) -> (n_out, V, 2) fp32; count over the children with both entries set,
    sums over all children with -1 read as 0, in float64"""
    corr = corr.float()
    both = (corr != -1).all(-1)
    count = torch.zeros((n_out,) + both.shape[1:], dtype=torch.float64, device=corr.device).index_add_(0, inverse, both.double())
    total = torch.zeros((n_out,) + corr.shape[1:], dtype=torch.float64, device=corr.device).index_add_(
        0, inverse, torch.where(corr == -1, torch.zeros_like(corr), corr).double())
    mean = total / count.clamp(min=1).unsqueeze(-1)
    return torch.where((count > 0).unsqueeze(-1), mean, -torch.ones_like(mean)).float()


def patch_plan_torch(corr, rows, scene, img_base, patch_h, patch_w):
    """(patch_ids (U), slot (pairs), count (U), pair_row (pairs)) of the valid pairs in (row, view) order (:786-830)"""
    sub = corr[rows]
    r, v = torch.where((sub != -1).any(-1))
    c = sub[r, v].long()
    patch = (img_base[scene[r]] + v) * (patch_h * patch_w) + c[:, 0] * patch_w + c[:, 1]
    patch_ids, slot, count = torch.unique(patch, return_inverse=True, return_counts=True)
    return patch_ids, slot, count, rows[r]


def patch_mean_torch(feat, pair_row, slot, count):
    """(U, C) fp32 mean of feat[pair_row] over every patch"""
    gathered = feat[pair_row].float() if feat.dtype != torch.float64 else feat[pair_row]
    total = gathered.new_zeros((count.shape[0], feat.shape[1])).index_add_(0, slot, gathered)
    return total / count.to(total.dtype).unsqueeze(1)


def cos_loss_torch(a, b, patch_ids, shift=True):
    """10 mean_j (1 - cos(b[patch_ids[j]], a[j])), both rows less their mean over D with `shift` (:834-842)"""
    a = a if a.dtype == torch.float64 else a.float()
    b = b[patch_ids].to(a.dtype)
    if shift:
        a, b = a - a.mean(dim=-1, keepdim=True), b - b.mean(dim=-1, keepdim=True)
    return (1 - F.cosine_similarity(b, a, dim=1, eps=1e-6)).mean() * 10


class OnlineCluster(SonataCluster):
    """Sonata's projection head with `enable_mlp` (:34-78): without the MLP only the weight-normed prototypes remain."""

    def __init__(self, in_channels, hidden_channels=4096, embed_channels=512, num_prototypes=4096, enable_mlp=True):
        if enable_mlp:
            super().__init__(in_channels, hidden_channels, embed_channels, num_prototypes)
            return
        nn.Module.__init__(self)
        self.prototype = nn.utils.parametrizations.weight_norm(nn.Linear(embed_channels, num_prototypes, bias=False))
        norm = self.prototype.parametrizations.weight.original0
        norm.data.fill_(1)
        norm.requires_grad = False

    def forward(self, feat):
        if hasattr(self, "mlp"):
            return super().forward(feat)
        eps = 1e-6 if feat.dtype == torch.float16 else 1e-12
        return self.prototype(F.normalize(feat, dim=-1, p=2, eps=eps))


@MODELS.register_module("Concerto-v1m1")
class Concerto(Sonata):
    def __init__(self, image_weight_name, image_weight_path, backbone, head_in_channels, backbone_out_channels,
                 embedding_channels, patch_w, patch_h, student_pretrained_path=None, teacher_pretrained_path=None,
                 student_pretrained=False, head_hidden_channels=4096, head_embed_channels=512, head_num_prototypes=4096,
                 enc2d_head_in_channels=384, enc2d_head_hidden_channels=4096, enc2d_head_embed_channels=256,
                 enc2d_head_num_prototypes=384, teacher_custom=None, num_global_view=2, num_local_view=4,
                 mask_size_start=0.1, mask_size_base=0.4, mask_size_warmup_ratio=0.05, mask_ratio_start=0.3,
                 mask_ratio_base=0.7, mask_ratio_warmup_ratio=0.05, mask_jitter=None, teacher_temp_start=0.04,
                 teacher_temp_base=0.07, teacher_temp_warmup_ratio=0.05, student_temp=0.1, mask_loss_weight=2 / 10,
                 roll_mask_loss_weight=2 / 10, unmask_loss_weight=4 / 10, enc2d_loss_weight=2 / 10, momentum_base=0.996,
                 momentum_final=1, match_max_k=8, match_max_r=0.08, up_cast_level=2, enc2d_upcast_level=4,
                 enc2d_cos_shift=True, sonata_model_type="offline"):
        PointModel.__init__(self)
        assert sonata_model_type in ["online", "offline"]
        self.mask_loss_weight = mask_loss_weight
        self.roll_mask_loss_weight = roll_mask_loss_weight
        self.unmask_loss_weight = unmask_loss_weight
        self.enc2d_loss_weight = enc2d_loss_weight
        self.num_global_view = num_global_view
        self.num_local_view = num_local_view

        self.mask_size = self.mask_size_start = mask_size_start
        self.mask_size_base = mask_size_base
        self.mask_size_warmup_ratio = mask_size_warmup_ratio
        self.mask_size_scheduler = None
        self.mask_ratio = self.mask_ratio_start = mask_ratio_start
        self.mask_ratio_base = mask_ratio_base
        self.mask_ratio_warmup_ratio = mask_ratio_warmup_ratio
        self.mask_ratio_scheduler = None
        self.mask_jitter = mask_jitter
        self.teacher_temp = self.teacher_temp_start = teacher_temp_start
        self.teacher_temp_base = teacher_temp_base
        self.teacher_temp_warmup_ratio = teacher_temp_warmup_ratio
        self.teacher_temp_scheduler = None
        self.student_temp = student_temp
        self.momentum = self.momentum_base = momentum_base
        self.momentum_final = momentum_final
        self.momentum_scheduler = None
        self.match_max_k = match_max_k
        self.match_max_r = match_max_r
        self.up_cast_level = up_cast_level
        self.enc2d_upcast_level = enc2d_upcast_level

        distill = unmask_loss_weight + mask_loss_weight + roll_mask_loss_weight
        assert distill + enc2d_loss_weight > 0                                        # one of the losses is on
        assert num_global_view > 1 or roll_mask_loss_weight == 0                      # a roll needs two global views
        assert num_global_view == 1 or num_global_view == 2                           # and knows no more than two

        student_backbone = build_model(backbone)
        if student_pretrained_path is not None:
            student_backbone = self.load_sonata(student_backbone, path=student_pretrained_path)
        # the teacher's backbone without the student's regularisation (drop path ...); the caller's dict stays as it is
        teacher_backbone = build_model({**backbone, **(teacher_custom or {})})
        if sonata_model_type == "offline":
            teacher_backbone = self.load_sonata(teacher_backbone, path=teacher_pretrained_path)
        student, teacher = dict(backbone=student_backbone), dict(backbone=teacher_backbone)

        if enc2d_loss_weight > 0:
            self.patch_h = patch_h
            self.patch_w = patch_w
            self.image_weight_name = image_weight_name
            self.enc2d_model = self.load_enc2d(image_weight_name, image_weight_path)
            self.enc2d_model.requires_grad_(False)
            self._num_channels = enc2d_head_in_channels
            self.patch_proj = nn.Linear(backbone_out_channels, enc2d_head_in_channels)
            # the 2D heads exist for state_dict parity: forward uses neither (as the reference)
            enc2d_head = partial(OnlineCluster, in_channels=enc2d_head_in_channels,
                                 hidden_channels=enc2d_head_hidden_channels, embed_channels=enc2d_head_in_channels,
                                 num_prototypes=enc2d_head_num_prototypes)
            self.enc2d_head_student = enc2d_head()
            self.enc2d_head_teacher = enc2d_head(enable_mlp=False)
            self.enc2d_head_student.prototype.load_state_dict(self.enc2d_head_teacher.prototype.state_dict())
            for p in self.enc2d_head_teacher.parameters():
                p.requires_grad = False

        head = partial(OnlineCluster, in_channels=head_in_channels, hidden_channels=head_hidden_channels,
                       embed_channels=head_embed_channels, num_prototypes=head_num_prototypes)
        if mask_loss_weight > 0 or roll_mask_loss_weight > 0:
            student["mask_head"], teacher["mask_head"] = head(), head()
        if unmask_loss_weight > 0 or (enc2d_loss_weight > 0 and distill == 0):
            student["unmask_head"], teacher["unmask_head"] = head(), head()
        self.student = nn.ModuleDict(student)
        self.teacher = nn.ModuleDict(teacher)
        for name, module in self.student.items():
            if "head" in name:
                self.teacher[name].load_state_dict(module.state_dict())
        if sonata_model_type == "online":
            self.teacher.backbone.load_state_dict(self.student.backbone.state_dict())
        for p in self.teacher.parameters():
            p.requires_grad = False
        self.enc2d_cos_shift = enc2d_cos_shift
        self.sonata_model_type = sonata_model_type
        self._fused = True

    def set_fused(self, on=True):
        """False: every loss and the image branch as torch compositions."""
        return super().set_fused(on)

    # -- loading ----------------------------------------------------------------------------------------------------
    def load_enc2d(self, model_name, model_weight):
        """The frozen image encoder: transformers.AutoModel from a LOCAL directory (nothing is fetched).  The override
        point for another encoder; ENC2D_forward decides how its output is read."""
        try:
            from transformers import AutoModel
        except ImportError as e:
            raise ImportError(f"Concerto-v1m1: the image encoder '{model_name}' needs the `transformers` package") from e
        if not os.path.isdir(str(model_weight)):
            raise FileNotFoundError(f"Concerto-v1m1: image_weight_path '{model_weight}' is not a local directory with the "
                                    f"weights of '{model_name}'; they are not fetched, download them beforehand or "
                                    "override load_enc2d")
        try:
            model = AutoModel.from_pretrained(model_weight, trust_remote_code=True, local_files_only=True)
        except Exception as e:
            raise RuntimeError(f"Concerto-v1m1: could not load the image encoder '{model_name}' from '{model_weight}': "
                               f"{e}") from e
        return model.eval()

    def load_sonata(self, model, path):
        """A Sonata checkpoint into a backbone (:288-306): if keys under `state_dict` contain module.student.backbone.
        those, stripped to backbone keys, are loaded; otherwise the checkpoint as it is."""
        where = (lambda storage, loc: storage.cuda()) if torch.cuda.is_available() else "cpu"
        checkpoint = torch.load(path, map_location=where)
        weight = {}
        if "state_dict" in checkpoint.keys():
            checkpoint = checkpoint["state_dict"]
            mark = "module.student.backbone."
            weight = {key.replace(mark, "module.")[7:]: value for key, value in checkpoint.items() if mark in key}
        info = model.load_state_dict(weight if weight else checkpoint)
        print(f"Missing keys: {info[0]}")
        print(f"Unexpected keys: {info[1]}")
        return model

    @torch.no_grad()
    def ENC2D_forward(self, x):
        """(images, patch_h * patch_w, D) patch tokens by the reference's three conventions (:309-325)"""
        tokens = self.patch_h * self.patch_w
        if "radio" in self.image_weight_name:
            _, features = self.enc2d_model(x)
            return features.reshape(-1, tokens, self._num_channels)
        if hasattr(self.enc2d_model, "vision_model"):
            return self.enc2d_model.vision_model(x).last_hidden_state
        return self.enc2d_model(x).last_hidden_state[:, -tokens:, :]

    # -- hooks ------------------------------------------------------------------------------------------------------
    def after_step(self):
        with torch.no_grad():
            m = float(self.momentum)
            pairs = []
            if self.sonata_model_type == "online":
                pairs.append((list(self.teacher.backbone.parameters()), list(self.student.backbone.parameters())))
            pairs.append(([p for n, p in self.teacher.named_parameters() if "head" in n],
                          [p for n, p in self.student.named_parameters() if "head" in n]))
            for teacher, student in pairs:
                torch._foreach_mul_(teacher, m)
                torch._foreach_add_(teacher, student, alpha=1 - m)
            if self.enc2d_loss_weight > 0:
                torch._foreach_copy_([p for n, p in self.enc2d_head_teacher.named_parameters() if "prototype" in n],
                                     [p for n, p in self.enc2d_head_student.named_parameters() if "prototype" in n])

    # -- the image branch -------------------------------------------------------------------------------------------
    def up_cast(self, point, upcast_level=None):
        """features of the last `upcast_level` (default up_cast_level) pooling stages carried back to their points"""
        return super().up_cast(point, levels=upcast_level)

    def _kernels(self, kernel, tensor, width, rows):
        return (self._fused and tensor.is_cuda and tensor.dtype in (torch.float32, torch.bfloat16)
                and wired(kernel, width, rows))

    def pool_corr(self, point, correspondence):
        """The level-0 correspondences (N0, V, 2) pooled down to the level of `point` through the poolings between them
        (their stored order and segment starts; nothing is sorted again): Point(offset, feat, correspondence)."""
        levels = []
        at = point
        while "pooling_parent" in at.keys():
            assert "pooling_inverse" in at.keys()
            levels.append((at.pooling_inverse, at.get("_pool_segments"), at.feat.shape[0]))
            at = at.pooling_parent
        corr = correspondence
        for inverse, segments, n_out in reversed(levels):
            if corr.shape[1] == 0:
                corr = -torch.ones((n_out, 0, 2), device=corr.device)
            elif (segments is not None and self._fused and corr.is_cuda
                  and wired("pool_corr", corr.shape[1], corr.shape[0])):
                corr = ops.concerto_pool_corr(corr.contiguous(), segments[0], segments[1])
            else:
                corr = pool_corr_torch(corr, inverse, n_out)
        return Point(offset=point.offset, feat=point.feat, correspondence=corr)

    def principal_rows(self, offset, offset_host=None):
        """(rows, scene, offsets) of the first global view of every scene: its feature rows ascending, the scene of each,
        and the views' cumulative ends; from the host copy of the offsets when the backbone left one"""
        host = [int(v) for v in (offset_host if offset_host is not None else offset.tolist())]
        starts = [0] + host
        n, dev = self.num_global_view, offset.device
        views = range(0, len(host), n)
        rows = torch.cat([torch.arange(starts[i], starts[i + 1], device=dev) for i in views])
        scene = torch.cat([torch.full((starts[i + 1] - starts[i],), b, dtype=torch.long, device=dev)
                           for b, i in enumerate(views)])
        return rows, scene

    def enc2d_loss(self, feat, corr, rows, scene, feature2d, img_num, check=False):
        """The image loss (:786-842) from the student's up-cast features feat (n, C), the pooled correspondences corr
        (n, V, 2), the principal views' rows / scenes, the encoder's rows feature2d (images * patch_h * patch_w, D) and
        the images per scene.  -> (loss, dict of intermediates: patch_ids, patch_mean, projected)"""
        img_num = img_num.to(feat.device).long()
        img_base = torch.cumsum(img_num, 0) - img_num
        n_patches = feature2d.shape[0]
        corr = corr.float().contiguous()
        c, d = feat.shape[1], feature2d.shape[1]
        plan = None
        if self._kernels("patch_mean", feat, c, feat.shape[0]) and corr.is_cuda:
            plan = ops.concerto_plan(corr, rows, scene, img_base, self.patch_h, self.patch_w, n_patches, check=check)
        if plan is not None and plan.u > 0:
            patch_ids = plan.patch_ids
            mean = A.concerto_patch_mean(feat, plan)
        else:
            patch_ids, slot, count, pair_row = patch_plan_torch(corr, rows, scene, img_base, self.patch_h, self.patch_w)
            if check and patch_ids.numel() and not (0 <= int(patch_ids[0]) and int(patch_ids[-1]) < n_patches):
                raise RuntimeError(f"Concerto-v1m1: a correspondence points outside the {n_patches} patches")
            mean = patch_mean_torch(feat, pair_row, slot, count)
        projected = self.patch_proj(mean.to(self.patch_proj.weight.dtype))
        u = patch_ids.shape[0]
        if (u > 0 and feature2d.is_cuda and feature2d.dtype in (torch.float32, torch.bfloat16)
                and ops.concerto_cos_capable(d) and self._kernels("cos", projected, d, u)):
            loss = A.concerto_cos_loss(projected, feature2d, patch_ids, self.enc2d_cos_shift)
        else:
            loss = cos_loss_torch(projected, feature2d, patch_ids, self.enc2d_cos_shift)
        return loss, dict(patch_ids=patch_ids, patch_mean=mean, projected=projected)

    def forward(self, data_dict, return_point=False):
        if return_point:
            return dict(point=self.up_cast(self.teacher.backbone(data_dict)))

        def view(prefix, **extra):
            return Point(feat=data_dict[prefix + "_feat"], coord=data_dict[prefix + "_coord"],
                         origin_coord=data_dict[prefix + "_origin_coord"], offset=data_dict[prefix + "_offset"],
                         grid_size=data_dict["grid_size"][0], **extra)

        distill = self.mask_loss_weight + self.roll_mask_loss_weight + self.unmask_loss_weight
        masked = self.mask_loss_weight > 0 or self.roll_mask_loss_weight > 0
        with torch.no_grad():
            global_point = view("global")
            global_mask, _ = self.generate_mask(global_point.coord, global_point.offset)
            mask_global_coord = global_point.coord.clone().detach()
            if self.mask_jitter is not None:
                noise = torch.randn_like(mask_global_coord[global_mask]).mul(self.mask_jitter)
                mask_global_coord[global_mask] += torch.clip(noise, max=self.mask_jitter * 2)
            mask_global_point = view("global", mask=global_mask)
            mask_global_point["coord"] = mask_global_coord
            local_point = view("local")
            teacher_point = self.up_cast(self.teacher.backbone(global_point))
            # one shared teacher head for all three losses, mask before unmask (:634-640)
            teacher_sim = self.teacher["mask_head" if masked else "unmask_head"](teacher_point.feat)

        result, terms = dict(), []
        mask_point = None
        if masked or self.enc2d_loss_weight > 0:
            mask_point = self.up_cast(self.student.backbone(mask_global_point))
        if masked:
            student_sim = self.student.mask_head(mask_point.feat)
            if self.mask_loss_weight > 0:
                match = self.match_neighbour(mask_point.origin_coord, mask_point.offset,
                                             teacher_point.origin_coord, teacher_point.offset)
                result["mask_loss"] = self.distill_loss(student_sim, teacher_sim, match[:, 1], match[:, 0],
                                                        mask_point.offset)
                terms.append(result["mask_loss"] * self.mask_loss_weight)
            if self.roll_mask_loss_weight > 0:
                with torch.no_grad():
                    perm, rolled_offset = self._roll_index(teacher_point)
                match = self.match_neighbour(mask_point.origin_coord, mask_point.offset,
                                             teacher_point.origin_coord[perm].contiguous(), rolled_offset)
                result["roll_mask_loss"] = self.distill_loss(student_sim, teacher_sim, perm[match[:, 1]], match[:, 0],
                                                             mask_point.offset)
                terms.append(result["roll_mask_loss"] * self.roll_mask_loss_weight)
        if self.unmask_loss_weight > 0:
            local = self.up_cast(self.student.backbone(local_point))
            student_sim = self.student.unmask_head(local.feat)
            with torch.no_grad():
                # the first global view of every scene against all of its local views
                principal = teacher_point.batch % self.num_global_view == 0
                rows = principal.nonzero().squeeze(1)
                scene = teacher_point.batch[rows] // self.num_global_view
                match = self.match_neighbour(
                    local.origin_coord, local.offset[self.num_local_view - 1::self.num_local_view],
                    teacher_point.origin_coord[rows].contiguous(), batch2offset(scene))
            result["unmask_loss"] = self.distill_loss(student_sim, teacher_sim, rows[match[:, 1]], match[:, 0],
                                                      local.offset)
            terms.append(result["unmask_loss"] * self.unmask_loss_weight)
        if self.enc2d_loss_weight > 0:
            img_num = data_dict["img_num"]
            if int(img_num.sum()) > 0:
                enc2d_point = self.up_cast(mask_point, upcast_level=self.enc2d_upcast_level - self.up_cast_level)
                with torch.no_grad():
                    pooled = self.pool_corr(enc2d_point, data_dict["global_correspondence"])
                    rows, scene = self.principal_rows(enc2d_point.offset, enc2d_point.get("_offset_host"))
                    feature2d = self.ENC2D_forward(data_dict["images"])
                    feature2d = feature2d.contiguous().view(-1, feature2d.shape[-1])
                result["enc2d_loss"], _ = self.enc2d_loss(enc2d_point.feat, pooled.correspondence, rows, scene,
                                                          feature2d, img_num)
                terms.append(result["enc2d_loss"] * self.enc2d_loss_weight)
            elif distill > 0:
                result["enc2d_loss"] = sum(terms) / distill
                terms.append(result["enc2d_loss"] * self.enc2d_loss_weight)
        result["loss"] = sum(terms)
        if get_world_size() > 1:
            for loss in result.values():
                dist.all_reduce(loss, op=dist.ReduceOp.AVG)
        return result
