"""Sonata self-distillation pretraining ("Sonata-v1m1", reference pointcept/models/sonata/sonata_v1m1_base.py) on "PT-v3m2".

Constructor keywords, defaults, module tree, state_dict keys, the result dict and the hooks are the reference's.  What
differs is how a loss is evaluated.  The reference gathers the matched teacher rows into an (M, K) matrix, runs
sinkhorn_knopp over it (:267-291: exp, the total, three rounds of row sum / divide / column sum / divide - about twenty
sweeps), and then materialises log_softmax of the gathered student rows and the product (:443-449).  With E = exp(x / T)
that assignment is a column scaling and a row normalisation:

    u_1 = 1 / (K sum_m E[m, k]),   u_{i+1} = 1 / (K sum_m E[m, k] / (n d_i[m])),   d_i[m] = sum_k E[m, k] u_i[k]
    target[m, k] = E[m, k] u_3[k] / d_3[m]

so the only thing that has to cross ranks is n and a K-vector per sweep, and no (M, K) matrix has to exist:
  - fused (csrc/sonata_loss.hip): ptv3_sonata_sk_pass three times, ptv3_sonata_ce_fwd, and ptv3_sonata_ce_bwd in the
    backward; the gather by the match index is part of the kernels, the target and the log-softmax are formed on the fly;
  - composed - set_fused(False), CPU tensors, logits that are neither fp32 nor bf16, K outside ops.sonata_capable, or a
    shape `wired` does not list: the same scaling-form arithmetic in torch (it does write E and the target).
exp is taken without a shift as the reference does: the logits are cosines (unit feature, weight-norm with g = 1) and
T >= 0.04, so |x / T| <= 25.

The per-scene mean follows torch_scatter.segment_coo(reduce="mean") with dim_size = index.max() + 1 as documented: a scene
without a pair in the middle of the batch has mean 0 and counts, trailing scenes without a pair do not.  Neither path
reads anything back for it (the scene of the last pair stays on the device).

roll_point: the rolled view is an index into the teacher's rows, so the (N, K) teacher logits are not copied for the
roll-mask loss; roll_point itself still returns the reference's Point.
generate_mask keeps torch.unique and its host read (the number of patches); `patch_index` can be given.  The other host
reads of a step: the sizes of the global views for the roll permutation (as the reference's roll_point), the boolean cut
of every kNN match and the nonzero() of the principal views (as the reference), the backbone's pooling counts, and with
more than one rank the all-reduced pair count once per loss.
"""
from functools import partial
from itertools import chain

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.distributed as dist

import pointops
from pointcept.models.utils.structure import Point
from pointcept.models.builder import MODELS, build_model
from pointcept.models.modules import PointModel
from pointcept.models.utils import offset2batch, offset2bincount, batch2offset
from pointcept.utils.comm import get_world_size
from pointcept.utils.scheduler import CosineScheduler
from ptv3_hip import ops
from ptv3_hip import autograd as A


def wired(kernel, k, m):
    """Which kernels the model calls: by the wiring rule only what measured ahead of the composed path on an MI355X by
    more than the run-to-run spread (profiles/sonata/).  `loss` is the whole fused loss of one
    pairing - three sweeps, the cross entropy and its backward - at K prototypes and M pairs.  Measured at K = 1088, 2048,
    3072 and 4096 (all on the 64-entries-per-lane variant, whose time barely depends on K while the composed path's does)
    and M = 20 000 / 100 000, fp32 and bf16, forward and forward + backward: ahead 1.8 - 2.7 times at 4096, 1.5 - 2.2 at
    3072, 1.25 - 1.47 at (2048, 100 000), a tie at (2048, 20 000), behind at 1088.  The rule extrapolates only towards
    shapes where the kernel gets relatively cheaper: a larger K up to the variant's 4096, and more pairs."""
    if kernel == "loss":
        return (3072 <= k <= 4096 and m >= 20000) or (2048 <= k < 3072 and m >= 100000)
    raise KeyError(kernel)


# -- the composed path: the scaling form in torch -------------------------------------------------------------------
def _f32(t):
    return t if t.dtype in (torch.float32, torch.float64) else t.float()


def sk_sweep_torch(e, u=None, n_total=None):
    """A (K) of one sweep over E (M, K), this rank's rows: sum_m E (u None) or sum_m E / (n_total d), d = E u"""
    if u is None:
        return e.sum(0)
    d = (e * u).sum(1, keepdim=True)
    return (e / (n_total * d)).sum(0)


def sinkhorn_scaling_torch(e, n_total=None, all_reduce=None):
    """u_3 (K) for E (M, K); all_reduce(A) sums the partial sums of all ranks in place, n_total counts their rows"""
    k = e.shape[1]
    n = e.shape[0] if n_total is None else n_total
    u = None
    for _ in range(3):
        a = sk_sweep_torch(e, u, n)
        if all_reduce is not None:
            all_reduce(a)
        u = 1.0 / (k * a)
    return u


def pair_losses_torch(s, x, idx_t, idx_s, temp, student_temp, n_total=None, all_reduce=None):
    """(loss per pair (M), target (M, K)) of one pairing by the scaling form"""
    e = torch.exp(_f32(x.detach())[idx_t] / temp)
    u = sinkhorn_scaling_torch(e, n_total, all_reduce)
    target = e * u
    target = target / target.sum(1, keepdim=True)
    return -torch.sum(target * F.log_softmax(_f32(s)[idx_s] / student_temp, dim=-1), dim=-1), target


def scene_mean_torch(values, scene, num_scenes):
    """mean over the scenes 0 .. scene[-1] of the per-scene means of `values` (scene ids ascending, at least one):
    segment_coo(reduce="mean") with dim_size = index.max() + 1 followed by .mean(), nothing read back"""
    total = values.new_zeros(num_scenes).index_add_(0, scene, values)
    count = values.new_zeros(num_scenes).index_add_(0, scene, torch.ones_like(values))
    return (total / count.clamp(min=1)).sum() / (scene[-1] + 1).to(values.dtype)


def sonata_loss_torch(s, x, idx_t, idx_s, offset_s, temp, student_temp, n_total=None, all_reduce=None):
    """the composed loss of one pairing; 0 (with a zero gradient) without a pair"""
    if idx_t.shape[0] == 0:
        if all_reduce is not None:      # the other ranks wait in their three reductions
            sinkhorn_scaling_torch(_f32(x.detach())[:0], n_total, all_reduce)
        return s.sum() * 0.0
    per_pair, _ = pair_losses_torch(s, x, idx_t, idx_s, temp, student_temp, n_total, all_reduce)
    scene = torch.bucketize(idx_s, offset_s.to(idx_s.device), right=True)
    return scene_mean_torch(per_pair, scene, offset_s.shape[0])


class OnlineCluster(nn.Module):
    """The projection head (:27-68): Linear - GELU - Linear, L2 normalisation, cosine logits against weight-normed
    prototypes whose norms are frozen at 1.  Three matrix products of M rows: plain torch."""

    def __init__(self, in_channels, hidden_channels=4096, embed_channels=512, num_prototypes=4096):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(in_channels, hidden_channels), nn.GELU(),
                                 nn.Linear(hidden_channels, embed_channels))
        self.apply(self._init_weights)
        self.prototype = nn.utils.parametrizations.weight_norm(nn.Linear(embed_channels, num_prototypes, bias=False))
        norm = self.prototype.parametrizations.weight.original0
        norm.data.fill_(1)
        norm.requires_grad = False

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)

    def forward(self, feat):
        feat = self.mlp(feat)
        eps = 1e-6 if feat.dtype == torch.float16 else 1e-12
        return self.prototype(F.normalize(feat, dim=-1, p=2, eps=eps))


@MODELS.register_module("Sonata-v1m1")
class Sonata(PointModel):
    def __init__(self, backbone, head_in_channels, head_hidden_channels=4096, head_embed_channels=512,
                 head_num_prototypes=4096, teacher_custom=None, num_global_view=2, num_local_view=4,
                 mask_size_start=0.1, mask_size_base=0.4, mask_size_warmup_ratio=0.05, mask_ratio_start=0.3,
                 mask_ratio_base=0.7, mask_ratio_warmup_ratio=0.05, mask_jitter=None, teacher_temp_start=0.04,
                 teacher_temp_base=0.07, teacher_temp_warmup_ratio=0.05, student_temp=0.1, mask_loss_weight=2 / 8,
                 roll_mask_loss_weight=2 / 8, unmask_loss_weight=4 / 8, momentum_base=0.996, momentum_final=1,
                 match_max_k=8, match_max_r=0.08, up_cast_level=2):
        super().__init__()
        self.mask_loss_weight = mask_loss_weight
        self.roll_mask_loss_weight = roll_mask_loss_weight
        self.unmask_loss_weight = unmask_loss_weight
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

        assert unmask_loss_weight + mask_loss_weight + roll_mask_loss_weight > 0     # one of the losses is on
        assert num_global_view > 1 or roll_mask_loss_weight == 0                      # a roll needs two global views
        assert num_global_view == 1 or num_global_view == 2                           # and knows no more than two

        # the teacher's backbone without the student's regularisation (drop path ...); the caller's dict stays as it is
        student = dict(backbone=build_model(backbone))
        teacher = dict(backbone=build_model({**backbone, **(teacher_custom or {})}))
        head = partial(OnlineCluster, in_channels=head_in_channels, hidden_channels=head_hidden_channels,
                       embed_channels=head_embed_channels, num_prototypes=head_num_prototypes)
        if mask_loss_weight > 0 or roll_mask_loss_weight > 0:
            student["mask_head"], teacher["mask_head"] = head(), head()
        if unmask_loss_weight > 0:
            student["unmask_head"], teacher["unmask_head"] = head(), head()
        self.student = nn.ModuleDict(student)
        self.teacher = nn.ModuleDict(teacher)
        for name, module in self.student.items():
            self.teacher[name].load_state_dict(module.state_dict())
        for p in self.teacher.parameters():
            p.requires_grad = False
        self._fused = True

    def set_fused(self, on=True):
        """False: every loss as a torch composition (the scaling form, with E and the target written out)."""
        self._fused = bool(on)
        return self

    # -- hooks: the four schedules and the teacher's moving average ----------------------------------------------------
    def before_train(self):
        total = self.trainer.cfg.scheduler.total_steps
        done = self.trainer.start_epoch * len(self.trainer.train_loader)

        def warmed(start, base, ratio):
            sched = CosineScheduler(start_value=start, base_value=base, final_value=base,
                                    warmup_iters=int(total * ratio), total_iters=total)
            sched.iter = done
            return sched

        self.mask_size_scheduler = warmed(self.mask_size_start, self.mask_size_base, self.mask_size_warmup_ratio)
        self.mask_ratio_scheduler = warmed(self.mask_ratio_start, self.mask_ratio_base, self.mask_ratio_warmup_ratio)
        self.teacher_temp_scheduler = warmed(self.teacher_temp_start, self.teacher_temp_base,
                                             self.teacher_temp_warmup_ratio)
        self.momentum_scheduler = CosineScheduler(base_value=self.momentum_base, final_value=self.momentum_final,
                                                  total_iters=total)
        self.momentum_scheduler.iter = done

    def before_step(self):
        self.mask_size = self.mask_size_scheduler.step()
        self.mask_ratio = self.mask_ratio_scheduler.step()
        self.teacher_temp = self.teacher_temp_scheduler.step()
        self.momentum = self.momentum_scheduler.step()
        writer = getattr(self.trainer, "writer", None)
        if writer is not None:
            for name in ("mask_size", "mask_ratio", "teacher_temp", "momentum"):
                writer.add_scalar(f"params/{name}", getattr(self, name), getattr(self, name + "_scheduler").iter)

    def after_step(self):
        with torch.no_grad():
            m = float(self.momentum)
            teacher = list(self.teacher.parameters())
            torch._foreach_mul_(teacher, m)
            torch._foreach_add_(teacher, list(self.student.parameters()), alpha=1 - m)

    # -- views ------------------------------------------------------------------------------------------------------
    def generate_mask(self, coord, offset, patch_index=None):
        """(point_mask (N) bool, point_cluster (N)): points fall into cubes of mask_size per scene, the first
        int(patches * mask_ratio) cubes of a random order are masked.  Patch ids are the sorted unique (batch, cell) rows;
        patch_index (a permutation of them) defaults to torch.randperm on the device."""
        batch = offset2batch(offset, coord.shape[0])
        low = coord.new_zeros((offset.shape[0], coord.shape[1])).scatter_reduce_(
            0, batch.unsqueeze(-1).expand_as(coord), coord, "amin", include_self=False)
        cell = torch.div(coord - low[batch], self.mask_size, rounding_mode="floor").int()
        cell = torch.cat([batch.unsqueeze(-1).to(cell.dtype), cell], dim=-1)
        unique, point_cluster = torch.unique(cell, dim=0, sorted=True, return_inverse=True)
        patch_num = unique.shape[0]
        if patch_index is None:
            patch_index = torch.randperm(patch_num, device=coord.device)
        masked = patch_index.to(coord.device)[:int(patch_num * self.mask_ratio)]
        return torch.isin(point_cluster, masked), point_cluster

    @torch.no_grad()
    def match_neighbour(self, view1_coord, view1_offset, view2_coord, view2_offset):
        """(M, 2) rows (view1, nearest of view2 in the same scene) closer than match_max_r; view1 ascending"""
        index2, distance = pointops.knn_query(1, view2_coord.float().contiguous(), view2_offset.int(),
                                              view1_coord.float().contiguous(), view1_offset.int())
        index1 = torch.arange(index2.shape[0], device=index2.device, dtype=torch.long).unsqueeze(-1)
        return torch.cat([index1, index2.long()], dim=-1)[distance.squeeze(-1) < self.match_max_r]

    def _roll_index(self, point):
        """row permutation that swaps the two global views of every scene, [a, a', b, b'] -> [a', a, b', b], and the
        offsets of the result"""
        n = self.num_global_view
        sizes = offset2bincount(point.offset).tolist()
        starts = [0]
        for v in sizes:
            starts.append(starts[-1] + v)
        order = list(chain(*[range(n * b, n * (b + 1))[::-1] for b in range(len(sizes) // n)]))
        dev = point.offset.device
        perm = torch.cat([torch.arange(starts[i], starts[i + 1], device=dev) for i in order])
        offset = torch.tensor([sizes[i] for i in order], device=dev, dtype=point.offset.dtype).cumsum(0)
        return perm, offset

    @torch.no_grad()
    def roll_point(self, point):
        perm, offset = self._roll_index(point)
        rolled = {key: point[key][perm] for key in ("feat", "coord", "origin_coord") if key in point.keys()}
        rolled["batch"] = offset2batch(offset, perm.shape[0])
        return Point(rolled)

    def up_cast(self, point, levels=None):
        """features of the last `levels` (default `up_cast_level`) pooling stages carried back to the points they were
        pooled from"""
        for _ in range(self.up_cast_level if levels is None else levels):
            assert "pooling_parent" in point.keys()
            assert "pooling_inverse" in point.keys()
            parent = point.pop("pooling_parent")
            inverse = point.pop("pooling_inverse")
            segments = point.get("_pool_segments")
            if segments is not None and point.feat.requires_grad:
                carried = A.cluster_gather(point.feat, inverse, segments[0], segments[1])
            else:
                carried = point.feat[inverse]
            parent.feat = torch.cat([parent.feat, carried], dim=-1)
            point = parent
        return point

    # -- one loss ---------------------------------------------------------------------------------------------------
    def _use_kernels(self, student, teacher, pairs):
        k = student.shape[1]
        return (self._fused and student.is_cuda and teacher.is_cuda
                and student.dtype in (torch.float32, torch.bfloat16) and teacher.dtype in (torch.float32, torch.bfloat16)
                and ops.sonata_capable(k) and wired("loss", k, pairs))

    def _reduction(self, pairs, device):
        """(n_total, all_reduce) of the Sinkhorn sums: None, None on one rank"""
        if get_world_size() == 1:
            return None, None
        n = torch.tensor([pairs], dtype=torch.float64, device=device)
        dist.all_reduce(n)
        return float(n.item()), dist.all_reduce

    def distill_loss(self, student, teacher, idx_t, idx_s, offset_s):
        """mean over the student's scenes of the mean over their pairs of
        -sum_k sinkhorn_knopp(teacher[idx_t], teacher_temp)[m, k] log_softmax(student[idx_s[m]] / student_temp)[k]"""
        idx_t, idx_s = idx_t.contiguous(), idx_s.contiguous()
        pairs = idx_t.shape[0]
        n_total, all_reduce = self._reduction(pairs, student.device)
        fn = A.sonata_loss if self._use_kernels(student, teacher, pairs) else sonata_loss_torch
        return fn(student, teacher, idx_t, idx_s, offset_s, float(self.teacher_temp), float(self.student_temp), n_total,
                  all_reduce)

    def forward(self, data_dict, return_point=False):
        if return_point:
            return dict(point=self.up_cast(self.teacher.backbone(data_dict)))

        def view(prefix, **extra):
            return Point(feat=data_dict[prefix + "_feat"], coord=data_dict[prefix + "_coord"],
                         origin_coord=data_dict[prefix + "_origin_coord"], offset=data_dict[prefix + "_offset"],
                         grid_size=data_dict["grid_size"][0], **extra)

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
            global_feat = teacher_point.feat

        result, terms = dict(), []
        if self.mask_loss_weight > 0 or self.roll_mask_loss_weight > 0:
            with torch.no_grad():
                teacher_sim = self.teacher.mask_head(global_feat)
            student_point = self.up_cast(self.student.backbone(mask_global_point))
            student_sim = self.student.mask_head(student_point.feat)
            if self.mask_loss_weight > 0:
                match = self.match_neighbour(student_point.origin_coord, student_point.offset,
                                             teacher_point.origin_coord, teacher_point.offset)
                result["mask_loss"] = self.distill_loss(student_sim, teacher_sim, match[:, 1], match[:, 0],
                                                        student_point.offset)
                terms.append(result["mask_loss"] * self.mask_loss_weight)
            if self.roll_mask_loss_weight > 0:
                with torch.no_grad():
                    perm, rolled_offset = self._roll_index(teacher_point)
                match = self.match_neighbour(student_point.origin_coord, student_point.offset,
                                             teacher_point.origin_coord[perm].contiguous(), rolled_offset)
                result["roll_mask_loss"] = self.distill_loss(student_sim, teacher_sim, perm[match[:, 1]], match[:, 0],
                                                             student_point.offset)
                terms.append(result["roll_mask_loss"] * self.roll_mask_loss_weight)
        if self.unmask_loss_weight > 0:
            with torch.no_grad():
                teacher_sim = self.teacher.unmask_head(global_feat)
            student_point = self.up_cast(self.student.backbone(local_point))
            student_sim = self.student.unmask_head(student_point.feat)
            with torch.no_grad():
                # the first global view of every scene against all of its local views
                principal = teacher_point.batch % self.num_global_view == 0
                rows = principal.nonzero().squeeze(1)
                scene = teacher_point.batch[rows] // self.num_global_view
                match = self.match_neighbour(
                    student_point.origin_coord, student_point.offset[self.num_local_view - 1::self.num_local_view],
                    teacher_point.origin_coord[rows].contiguous(), batch2offset(scene))
            result["unmask_loss"] = self.distill_loss(student_sim, teacher_sim, rows[match[:, 1]], match[:, 0],
                                                      student_point.offset)
            terms.append(result["unmask_loss"] * self.unmask_loss_weight)
        result["loss"] = sum(terms)
        if get_world_size() > 1:
            for loss in result.values():
                dist.all_reduce(loss, op=dist.ReduceOp.AVG)
        return result
