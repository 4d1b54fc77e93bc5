"""OA-CNNs (omni-adaptive sparse CNN) on MI355X.

Counterpart of the reference's pointcept/models/oacnns/oacnns_v1m1_base.py:12-344: the same classes (BasicBlock,
DonwBlock - the reference's spelling -, UpBlock, OACNNs), constructor arguments, attribute names and therefore
state_dict keys, shapes and order.  A stem of three submanifold convs, four stages that halve the grid with a kernel-2 /
stride-2 sparse conv and run `enc_depth[i]` BasicBlocks, four UpBlocks that invert the strided convs and fuse the skips.

BasicBlock is the model's own piece (:87-110): for each of L grid sizes the stage's sites are partitioned into cells,
a per-cell softmax over learned logits weights a per-cell sum of projected features, and a per-site softmax over the L
grids mixes the cell aggregates back onto the sites, in front of two submanifold convs.
Eval (fused = True): the 2L + 1 projections of the block input are ONE ptv3_gemm with stacked weights and stacked folded
BatchNorm; ptv3_cluster_center, ptv3_cluster_softmax_sum and ptv3_cluster_mix do the per-cell arithmetic (the global
maximum of the logits stays a device scalar); BatchNorm / ReLU ride in GEMM epilogues.  No host read after the plan.
Training, or set_fused(False): the torch composition of the same formulas over the taped HIP Functions, with cell sums
as sorted-order segment sums (deterministic).  fp32 throughout.

torch_geometric's voxel_grid is restated (parity unpinned, the package is not installed): the cell of a site is
(b, (x - min_x) // g, (y - min_y) // g, (z - min_z) // g) with the per-axis minimum over ALL sites of the batch at that
level; only the partition matters (the ids go through torch.unique in the reference).  voxel_grid divides in fp32 and
truncates, which equals integer division for coordinates below 65536 and g <= 128; a larger g is refused.
"""
from functools import partial

import torch
import torch.nn as nn

from ptv3_hip import ops
from ptv3_hip import autograd as A
from pointcept.models.builder import MODELS
from pointcept.models.utils.misc import offset2batch
from pointcept.models.utils.hip_layers import Linear, BatchNorm1d, ReLU
from pointcept.models.utils.sparse import (SparseConvTensor, SubMConv3d, SparseConv3d, SparseInverseConv3d,
                                           SparseSequential, _ParamCache)

MAX_GRID = 128
NUM_STAGES = 4


def _lbr(cin, cout, norm_fn, bias=False):
    return nn.Sequential(Linear(cin, cout, bias=bias), norm_fn(cout), ReLU())


class BasicBlock(nn.Module):
    def __init__(self, in_channels, embed_channels, norm_fn=None, indice_key=None, depth=4, groups=None, grid_size=None,
                 bias=False):
        super().__init__()
        assert embed_channels % groups == 0
        if depth - 1 > 4:
            raise NotImplementedError("BasicBlock: at most 4 grid sizes per stage (ptv3_cluster_mix)")
        self.groups = groups
        self.embed_channels = embed_channels
        self.proj = nn.ModuleList()
        self.grid_size = grid_size
        self.weight = nn.ModuleList()
        self.l_w = nn.ModuleList()
        self.proj.append(_lbr(embed_channels, embed_channels, norm_fn))
        for _ in range(depth - 1):
            self.proj.append(_lbr(embed_channels, embed_channels, norm_fn))
            self.l_w.append(_lbr(embed_channels, embed_channels, norm_fn))
            self.weight.append(Linear(embed_channels, embed_channels, bias=False))
        self.adaptive = Linear(embed_channels, depth - 1, bias=False)
        self.fuse = _lbr(embed_channels * 2, embed_channels, norm_fn)
        self.voxel_block = SparseSequential(
            SubMConv3d(embed_channels, embed_channels, kernel_size=3, stride=1, padding=1, indice_key=indice_key, bias=bias),
            norm_fn(embed_channels),
            ReLU(),
            SubMConv3d(embed_channels, embed_channels, kernel_size=3, stride=1, padding=1, indice_key=indice_key, bias=bias),
            norm_fn(embed_channels),
        )
        self.act = ReLU()
        self.fused = True
        self._cache = _ParamCache()
        self.tap = None     # tests: set to a dict to receive `mixed`

    def _stacked(self):
        """weights (2L + 1)C x C and folded BatchNorm of l_w[0..L), proj[0..L), proj[L], in that order"""
        seqs = list(self.l_w) + list(self.proj)
        params = [p for s in seqs for p in (s[0].weight, s[1].weight, s[1].bias, s[1].running_mean, s[1].running_var)]

        def make():
            w = torch.cat([s[0].weight.detach().float() for s in seqs]).contiguous()
            folded = [s[1].folded() for s in seqs]
            return w, torch.cat([f[0] for f in folded]).contiguous(), torch.cat([f[1] for f in folded]).contiguous()
        return self._cache.get("stack", params, make)

    def _aggregate_fused(self, feat, clusters):
        c, nl = self.embed_channels, len(clusters)
        w, scale, shift = self._stacked()
        st = ops.gemm(feat, w, bn_scale=scale, bn_shift=shift, act=ops.ACT_RELU)         # (m, (2L + 1) C)
        logits = ops.gemm(feat, self.adaptive.weight_for(torch.float32))                 # (m, L)
        aggs = []
        for l, plan in enumerate(clusters):
            centred = ops.cluster_center(st[:, l * c:(l + 1) * c], plan)
            p = ops.gemm(centred, self.weight[l].weight_for(torch.float32))
            aggs.append(ops.cluster_softmax_sum(p, st[:, (nl + l) * c:(nl + l + 1) * c], torch.amax(p), plan))
        both = ops.cluster_mix(logits, aggs, clusters, head=st[:, 2 * nl * c:])          # cat([proj[L](f), mixed])
        if self.tap is not None:
            self.tap["mixed"] = both[:, c:]
        s, t = self.fuse[1].folded()
        return self.fuse[0](both, bn_scale=s, bn_shift=t, act=ops.ACT_RELU, res=feat)

    def _aggregate_composed(self, feat, clusters):
        feats = []
        for i, plan in enumerate(clusters):
            k = plan.count()
            seg = plan.seg_start[:k + 1]
            size = (seg[1:] - seg[:-1]).to(feat.dtype).unsqueeze(1)

            def total(v):
                return A.segment_sum(v, plan.cluster, plan.order, seg, k)

            def spread(v):
                return A.cluster_gather(v, plan.cluster, plan.order, seg)
            pw = self.l_w[i](feat)
            pw = pw - spread(total(pw) / size)
            pw = self.weight[i](pw)
            pw = torch.exp(pw - pw.max())
            pw = pw / (spread(total(pw)) + 1e-6)
            feats.append(spread(total(self.proj[i](feat) * pw)))
        adp = torch.softmax(self.adaptive(feat), dim=1)
        mixed = sum(adp[:, l:l + 1] * f for l, f in enumerate(feats))
        if self.tap is not None:
            self.tap["mixed"] = mixed
        return self.fuse(torch.cat([self.proj[-1](feat), mixed], dim=1)) + feat

    def forward(self, x, clusters):
        feat = x.features
        if self.fused and not self.training:
            res = self._aggregate_fused(feat, clusters)
            y = self.voxel_block(x.replace_feature(res))
            return y.replace_feature(ops.add_act(y.features, res, ops.ACT_RELU))
        res = self._aggregate_composed(feat, clusters)
        y = self.voxel_block(x.replace_feature(res))
        return y.replace_feature(self.act(y.features + res))


class DonwBlock(nn.Module):
    def __init__(self, in_channels, embed_channels, depth, sp_indice_key, point_grid_size, num_ref=16, groups=None,
                 norm_fn=None, sub_indice_key=None):
        super().__init__()
        for g in point_grid_size:
            if int(g) != g or not 1 <= g <= MAX_GRID:
                raise ValueError(f"point_grid_size {g}: an integer from 1 to {MAX_GRID} (voxel_grid's fp32 division is "
                                 "restated as integer division, exact only in that range)")
        self.num_ref = num_ref
        self.depth = depth
        self.point_grid_size = point_grid_size
        self.down = SparseSequential(
            SparseConv3d(in_channels, embed_channels, kernel_size=2, stride=2, indice_key=sp_indice_key, bias=False),
            norm_fn(embed_channels),
            ReLU(),
        )
        self.blocks = nn.ModuleList()
        for _ in range(depth):
            self.blocks.append(BasicBlock(in_channels=embed_channels, embed_channels=embed_channels,
                                          depth=len(point_grid_size) + 1, groups=groups, grid_size=point_grid_size,
                                          norm_fn=norm_fn, indice_key=sub_indice_key))

    def forward(self, x):
        x = self.down(x)
        low = x.indices[:, 1:].amin(dim=0).contiguous()     # (3) int32, stays on the device
        plans = {}
        for g in self.point_grid_size:                        # equal grid sizes share one partition
            if int(g) not in plans:
                plans[int(g)] = ops.cluster_plan(x.indices, low, int(g))
        clusters = [plans[int(g)] for g in self.point_grid_size]
        for block in self.blocks:
            x = block(x, clusters)
        return x


class UpBlock(nn.Module):
    def __init__(self, in_channels, skip_channels, embed_channels, depth, sp_indice_key, norm_fn=None, down_ratio=2,
                 sub_indice_key=None):
        super().__init__()
        assert depth > 0
        self.up = SparseSequential(
            SparseInverseConv3d(in_channels, embed_channels, kernel_size=down_ratio, indice_key=sp_indice_key, bias=False),
            norm_fn(embed_channels),
            ReLU(),
        )
        self.blocks = nn.ModuleList()    # empty in the reference too
        self.fuse = nn.Sequential(
            Linear(skip_channels + embed_channels, embed_channels),
            norm_fn(embed_channels),
            ReLU(),
            Linear(embed_channels, embed_channels),
            norm_fn(embed_channels),
            ReLU(),
        )
        self.fused = True

    def forward(self, x, skip_x):
        x = self.up(x)
        both = torch.cat([x.features, skip_x.features], dim=1)
        if self.fused and not self.training:
            s0, t0 = self.fuse[1].folded()
            s1, t1 = self.fuse[4].folded()
            h = self.fuse[0](both, bn_scale=s0, bn_shift=t0, act=ops.ACT_RELU)
            return x.replace_feature(self.fuse[3](h, bn_scale=s1, bn_shift=t1, act=ops.ACT_RELU, res=x.features))
        return x.replace_feature(self.fuse(both) + x.features)


def check_extent(name, shape, stages=NUM_STAGES):
    """Every strided conv needs 2 cells per axis: raise before any device work, naming the axis and the level."""
    shape = [int(s) for s in shape]
    for level in range(stages):
        for axis, s in enumerate(shape):
            if s < 2:
                raise ValueError(f"{name}: spatial shape {s} on axis {'xyz'[axis]} at level {level} is under the 2 "
                                 f"cells a stride-2 conv needs ({stages} down convs: at least {2 ** stages} cells at "
                                 "the input)")
        shape = [(s - 2) // 2 + 1 for s in shape]


@MODELS.register_module()
class OACNNs(nn.Module):
    def __init__(self, in_channels, num_classes, embed_channels=64, enc_num_ref=[16, 16, 16, 16],
                 enc_channels=[64, 64, 128, 256], groups=[2, 4, 8, 16], enc_depth=[2, 3, 6, 4], down_ratio=[2, 2, 2, 2],
                 dec_channels=[96, 96, 128, 256], point_grid_size=[[16, 32, 64], [8, 16, 24], [4, 8, 12], [2, 4, 6]],
                 dec_depth=[2, 2, 2, 2]):
        super().__init__()
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.num_stages = len(enc_channels)
        self.embed_channels = embed_channels
        norm_fn = partial(BatchNorm1d, eps=1e-3, momentum=0.01)

        def stem_conv(cin):
            return SubMConv3d(cin, embed_channels, kernel_size=3, padding=1, indice_key="stem", bias=False)
        self.stem = SparseSequential(
            stem_conv(in_channels), norm_fn(embed_channels), ReLU(),
            stem_conv(embed_channels), norm_fn(embed_channels), ReLU(),
            stem_conv(embed_channels), norm_fn(embed_channels), ReLU(),
        )
        self.enc = nn.ModuleList()
        self.dec = nn.ModuleList()
        for i in range(self.num_stages):
            self.enc.append(DonwBlock(in_channels=embed_channels if i == 0 else enc_channels[i - 1],
                                      embed_channels=enc_channels[i], depth=enc_depth[i], norm_fn=norm_fn,
                                      groups=groups[i], point_grid_size=point_grid_size[i], num_ref=enc_num_ref[i],
                                      sp_indice_key=f"spconv{i}", sub_indice_key=f"subm{i + 1}"))
            self.dec.append(UpBlock(in_channels=enc_channels[-1] if i == self.num_stages - 1 else dec_channels[i + 1],
                                    skip_channels=embed_channels if i == 0 else enc_channels[i - 1],
                                    embed_channels=dec_channels[i], depth=dec_depth[i], norm_fn=norm_fn,
                                    sp_indice_key=f"spconv{i}", sub_indice_key=f"subm{i}"))
        self.final = SubMConv3d(dec_channels[0], num_classes, kernel_size=1)
        self.apply(self._init_weights)

    def set_fused(self, fused):
        """fused = False: eval runs the training path's torch composition (running-statistic BatchNorm) instead of the
        fused kernels - what the fused path is tested against."""
        for m in self.modules():
            if hasattr(m, "fused"):
                m.fused = bool(fused)
        return self

    def backbone(self, input_dict, taps=None):
        """-> (decoder output SparseConvTensor on the input sites, scene ends as a host list).  One host read here
        (spatial shape and offsets) and one per stage (the coarse row count)."""
        grid = input_dict["grid_coord"]
        offset = input_dict["offset"]
        head = torch.cat([grid.max(dim=0).values.long(), offset.long()]).tolist()     # the forward's entry read
        shape, ends = [v + 1 for v in head[:3]], head[3:]
        check_extent(type(self).__name__, shape, self.num_stages)
        batch = offset2batch(offset.long(), ends[-1])
        x = SparseConvTensor(features=input_dict["feat"].float().contiguous(),
                             indices=torch.cat([batch.unsqueeze(-1), grid], dim=1).int().contiguous(),
                             spatial_shape=shape, batch_size=len(ends))
        x = self.stem(x)
        skips = [x]
        if taps is not None:
            taps.append(x)
        for i in range(self.num_stages):
            x = self.enc[i](x)
            skips.append(x)
            if taps is not None:
                taps.append(x)
        x = skips.pop(-1)
        for i in reversed(range(self.num_stages)):
            x = self.dec[i](x, skips.pop(-1))
            if taps is not None:
                taps.append(x)
        return x, ends

    def forward(self, input_dict):
        x, _ = self.backbone(input_dict)
        return self.final(x).features

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, SubMConv3d):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.BatchNorm1d):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)
