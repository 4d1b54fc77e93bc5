"""Point Transformer V2 (mode 2: plain Linear weight encoding) on MI355X.

Counterpart of the reference's pointcept/models/point_transformer_v2/point_transformer_v2m2_base.py:26-583: same
constructors, attribute names and state_dict keys, the same `[coord, feat, offset]` list passed from module to module,
and the registry name "PT-v2m2".

`.eval()` (with `fused = True`, the default): every Linear with its folded PointBatchNorm / ReLU is one ptv3_gemm, the
whole GroupedVectorAttention after its three projections is ptv3_gva_fwd, GridPool is ptv3_grid_keys + argsort +
segments + the max / mean reduces, and the map unpooling rides in a GEMM epilogue.  The list may carry a fourth entry, a
SceneOffsets with the scene ends as host integers; with it a level reads nothing back except each GridPool's row count.
`.train()` (or `fused = False`): the torch composition of the reference's formulas (batch-statistic BatchNorm in
training) over the HIP kNN, the taped HIP grouping, the HIP partition and a segment-sum backward of the unpooling
gather.  fp32 throughout, as the reference runs this config.
"""
import torch
import torch.nn as nn

import pointops
from ptv3_hip import ops
from ptv3_hip import autograd as A
from pointcept.models.builder import MODELS
from pointcept.models.utils.hip_layers import DropPath
from pointcept.models.utils.sparse import _ParamCache
from pointcept.models.point_transformer.point_transformer_seg import SceneOffsets, _linear, _folded, _scene_state


class PointBatchNorm(nn.Module):
    """BatchNorm1d over the channels of (n, c) or (n, l, c) point features."""

    def __init__(self, embed_channels):
        super().__init__()
        self.norm = nn.BatchNorm1d(embed_channels)

    def forward(self, input):
        if input.dim() == 3:     # (n, l, c): the statistics run over every (point, slot) row
            n, l, c = input.shape
            return self.norm(input.reshape(n * l, c)).view(n, l, c)
        if input.dim() == 2:
            return self.norm(input)
        raise NotImplementedError


def _norm_act_linear(width_in, hidden, width_out):
    return nn.Sequential(nn.Linear(width_in, hidden), PointBatchNorm(hidden), nn.ReLU(inplace=True),
                         nn.Linear(hidden, width_out))


def _proj(width_in, width_out, bias):
    return nn.Sequential(nn.Linear(width_in, width_out, bias=bias), PointBatchNorm(width_out), nn.ReLU(inplace=True))


def _proj_fused(x, seq, cache, **extra):
    """Linear + PointBatchNorm + ReLU as one GEMM (the Linear's bias is added in front of the folded norm)."""
    scale, shift = _folded(seq[1].norm, cache)
    return _linear(x, seq[0], cache, bn_scale=scale, bn_shift=shift, act=ops.ACT_RELU, **extra)


def _f32(cache, t):
    return cache.get(("f", id(t)), [t], lambda: t.detach().float().contiguous())


class GroupedVectorAttention(nn.Module):
    def __init__(self, embed_channels, groups, attn_drop_rate=0.0, qkv_bias=True, pe_multiplier=False, pe_bias=True):
        super().__init__()
        if embed_channels % groups != 0:
            raise ValueError(f"GroupedVectorAttention: groups={groups} does not divide embed_channels={embed_channels}")
        self.embed_channels, self.groups = embed_channels, groups
        self.attn_drop_rate, self.qkv_bias = attn_drop_rate, qkv_bias
        self.pe_multiplier, self.pe_bias = pe_multiplier, pe_bias
        self.linear_q = _proj(embed_channels, embed_channels, qkv_bias)
        self.linear_k = _proj(embed_channels, embed_channels, qkv_bias)
        self.linear_v = nn.Linear(embed_channels, embed_channels, bias=qkv_bias)
        if pe_multiplier:
            self.linear_p_multiplier = _norm_act_linear(3, embed_channels, embed_channels)
        if pe_bias:
            self.linear_p_bias = _norm_act_linear(3, embed_channels, embed_channels)
        self.weight_encoding = _norm_act_linear(embed_channels, groups, groups)
        self.softmax = nn.Softmax(dim=1)     # over the neighbour slots
        self.attn_drop = nn.Dropout(attn_drop_rate)
        self.fused = True
        self._cache = _ParamCache()

    def fusable(self, neighbours=16):
        """What ptv3_gva_fwd computes: the positional bias only, widths and neighbour count within its limits."""
        c, g = self.embed_channels, self.groups
        return (self.pe_bias and not self.pe_multiplier and c % 8 == 0 and c <= 512 and g <= 64
                and 1 <= neighbours <= 32)

    def forward(self, feat, coord, reference_index):
        if self.training or not self.fused or not self.fusable(reference_index.shape[1]):
            return self.compose(feat, coord, reference_index)
        cache = self._cache
        q = _proj_fused(feat, self.linear_q, cache)
        k = _proj_fused(feat, self.linear_k, cache)
        v = _linear(feat, self.linear_v, cache)
        lp, lw = self.linear_p_bias, self.weight_encoding
        s_p, t_p = _folded(lp[1].norm, cache, lp[0])
        s_w, t_w = _folded(lw[1].norm, cache, lw[0])
        return ops.grouped_vector_attention(q, k, v, coord.contiguous(), reference_index.contiguous(), self.groups,
                                            _f32(cache, lp[0].weight), s_p, t_p, _f32(cache, lp[3].weight),
                                            _f32(cache, lp[3].bias), _f32(cache, lw[0].weight), s_w, t_w,
                                            _f32(cache, lw[3].weight), _f32(cache, lw[3].bias))

    def compose(self, feat, coord, reference_index):
        """point_transformer_v2m2_base.py:110-136 as torch ops over the taped HIP row gather."""
        coord = coord.contiguous()
        idx = reference_index.contiguous()
        query, key, value = self.linear_q(feat), self.linear_k(feat), self.linear_v(feat)
        key = pointops.grouping(idx, key.contiguous(), coord, with_xyz=True)      # (n, ns, 3 + c), zeros where missing
        value = pointops.grouping(idx, value.contiguous(), coord, with_xyz=False)
        pos, key = key[:, :, 0:3], key[:, :, 3:]
        relation = key - query.unsqueeze(1)
        if self.pe_multiplier:
            relation = relation * self.linear_p_multiplier(pos)
        if self.pe_bias:
            peb = self.linear_p_bias(pos)
            relation = relation + peb
            value = value + peb
        weight = self.attn_drop(self.softmax(self.weight_encoding(relation)))     # (n, ns, g)
        weight = weight * torch.sign(idx + 1).to(weight.dtype).unsqueeze(-1)      # after the softmax, not renormalised
        n, ns, c = value.shape
        g = self.groups
        return (value.view(n, ns, g, c // g) * weight.unsqueeze(-1)).sum(1).reshape(n, c)


class Block(nn.Module):
    def __init__(self, embed_channels, groups, qkv_bias=True, pe_multiplier=False, pe_bias=True, attn_drop_rate=0.0,
                 drop_path_rate=0.0, enable_checkpoint=False):
        super().__init__()
        self.attn = GroupedVectorAttention(embed_channels=embed_channels, groups=groups, qkv_bias=qkv_bias,
                                           attn_drop_rate=attn_drop_rate, pe_multiplier=pe_multiplier, pe_bias=pe_bias)
        self.fc1 = nn.Linear(embed_channels, embed_channels, bias=False)
        self.fc3 = nn.Linear(embed_channels, embed_channels, bias=False)
        self.norm1 = PointBatchNorm(embed_channels)
        self.norm2 = PointBatchNorm(embed_channels)
        self.norm3 = PointBatchNorm(embed_channels)
        self.act = nn.ReLU(inplace=True)
        self.enable_checkpoint = enable_checkpoint
        self.drop_path = DropPath(drop_path_rate) if drop_path_rate > 0.0 else nn.Identity()
        self.fused = True
        self._cache = _ParamCache()

    def forward(self, points, reference_index):
        coord, feat, offset = points[:3]
        identity = feat
        if self.fused and not self.training and feat.shape[1] % 4 == 0:
            cache = self._cache
            s1, t1 = _folded(self.norm1.norm, cache)
            s2, t2 = _folded(self.norm2.norm, cache)
            s3, t3 = _folded(self.norm3.norm, cache)
            feat = _linear(feat, self.fc1, cache, bn_scale=s1, bn_shift=t1, act=ops.ACT_RELU)
            feat = ops.affine_act(self.attn(feat, coord, reference_index), s2, t2, ops.ACT_RELU)
            feat = _linear(feat, self.fc3, cache, bn_scale=s3, bn_shift=t3)
            feat = ops.add_act(identity.contiguous(), feat, ops.ACT_RELU)
        else:
            feat = torch.relu(self.norm1(self.fc1(feat)))
            if self.enable_checkpoint and self.training:
                from torch.utils.checkpoint import checkpoint
                feat = checkpoint(self.attn, feat, coord, reference_index, use_reentrant=False)
            else:
                feat = self.attn(feat, coord, reference_index)
            feat = torch.relu(self.norm2(feat))
            feat = self.norm3(self.fc3(feat))
            feat = torch.relu(identity + self.drop_path(feat))
        return [coord, feat, offset] + list(points[3:])


class BlockSequence(nn.Module):
    def __init__(self, depth, embed_channels, groups, neighbours=16, qkv_bias=True, pe_multiplier=False, pe_bias=True,
                 attn_drop_rate=0.0, drop_path_rate=0.0, enable_checkpoint=False):
        super().__init__()
        # one rate per block: a list as given, a single number for all of them, nothing = no DropPath
        rates = list(drop_path_rate) if isinstance(drop_path_rate, list) else [float(drop_path_rate or 0.0)] * depth
        if len(rates) != depth:
            raise ValueError(f"BlockSequence: {len(rates)} drop path rates for {depth} blocks")
        self.neighbours = neighbours
        self.blocks = nn.ModuleList(
            Block(embed_channels=embed_channels, groups=groups, qkv_bias=qkv_bias, pe_multiplier=pe_multiplier,
                  pe_bias=pe_bias, attn_drop_rate=attn_drop_rate, drop_path_rate=rates[i],
                  enable_checkpoint=enable_checkpoint) for i in range(depth))

    def forward(self, points):
        coord, feat, offset = points[:3]
        so = points[3] if len(points) > 3 else None
        # one neighbour search per sequence, shared by its blocks
        if so is not None:
            reference_index = so.knn_rows(self.neighbours, coord.contiguous())
        else:
            reference_index, _ = pointops.knn_query(self.neighbours, coord.contiguous(), offset)
        for block in self.blocks:
            points = block(points, reference_index)
        return points


class GridPool(nn.Module):
    """Partition-based pooling: the points of one grid cell become one point (feature max, coordinate mean)."""

    def __init__(self, in_channels, out_channels, grid_size, bias=False):
        super().__init__()
        self.in_channels, self.out_channels, self.grid_size = in_channels, out_channels, grid_size
        self.fc = nn.Linear(in_channels, out_channels, bias=bias)
        self.norm = PointBatchNorm(out_channels)
        self.act = nn.ReLU(inplace=True)
        self.fused = True
        self._cache = _ParamCache()

    def forward(self, points, start=None):
        coord, feat, offset = points[:3]
        if start is not None:
            raise NotImplementedError("GridPool: a caller-supplied `start` is not used by PT-v2m2 and is not built")
        coord = coord.float().contiguous()
        fused = self.fused and not self.training and feat.shape[1] % 4 == 0 and self.out_channels % 4 == 0
        if fused:
            scale, shift = _folded(self.norm.norm, self._cache)
            feat = _linear(feat, self.fc, self._cache, bn_scale=scale, bn_shift=shift, act=ops.ACT_RELU)
        else:
            feat = torch.relu(self.norm(self.fc(feat)))
        plan = ops.grid_pool_plan(coord, offset, self.grid_size)      # reads the pooled row count
        new_coord = ops.segment_mean3(coord, plan.order, plan.seg_start, plan.n_out)
        if fused:
            feat = ops.pool_max(feat.contiguous(), plan.order, plan.seg_start, plan.n_out)
        else:
            rows = plan.cluster.unsqueeze(1).expand(-1, feat.shape[1])
            feat = feat.new_zeros((plan.n_out, feat.shape[1])).scatter_reduce(0, rows, feat, "amax", include_self=False)
        new_offset = plan.offset.int()
        so = SceneOffsets(plan.offset_host, new_offset)
        so.plan = plan
        return [new_coord, feat, new_offset, so], plan.cluster


class UnpoolWithSkip(nn.Module):
    """Map unpooling with a skip connection: every fine point takes its cluster's projected feature."""

    def __init__(self, in_channels, skip_channels, out_channels, bias=True, skip=True, backend="map"):
        super().__init__()
        self.in_channels, self.skip_channels, self.out_channels = in_channels, skip_channels, out_channels
        self.skip, self.backend = skip, backend
        assert self.backend in ["map", "interp"]
        self.proj = _proj(in_channels, out_channels, bias)
        self.proj_skip = _proj(skip_channels, out_channels, bias)
        self.fused = True
        self._cache = _ParamCache()

    def forward(self, points, skip_points, cluster=None):
        coord, feat, offset = points[:3]
        skip_coord, skip_feat, skip_offset = skip_points[:3]
        mapped = self.backend == "map" and cluster is not None
        widths_ok = feat.shape[1] % 4 == 0 and skip_feat.shape[1] % 4 == 0
        if self.fused and not self.training and mapped and self.skip and widths_ok:
            coarse = _proj_fused(feat, self.proj, self._cache)
            feat = _proj_fused(skip_feat, self.proj_skip, self._cache, res=coarse, res_index=cluster.int())
        else:
            feat = self.proj(feat)
            if mapped:
                plan = getattr(points[3], "plan", None) if len(points) > 3 else None
                if plan is not None and plan.cluster is cluster:
                    feat = A.cluster_gather(feat, cluster, plan.order, plan.seg_start)   # segment-sum backward
                else:
                    feat = feat[cluster]
            else:
                feat = pointops.interpolation(coord.contiguous(), skip_coord.contiguous(), feat.contiguous(), offset,
                                              skip_offset)
            if self.skip:
                feat = feat + self.proj_skip(skip_feat)
        return [skip_coord, feat, skip_offset] + list(skip_points[3:])


class Encoder(nn.Module):
    def __init__(self, depth, in_channels, embed_channels, groups, grid_size=None, neighbours=16, qkv_bias=True,
                 pe_multiplier=False, pe_bias=True, attn_drop_rate=None, drop_path_rate=None, enable_checkpoint=False):
        super().__init__()
        self.down = GridPool(in_channels=in_channels, out_channels=embed_channels, grid_size=grid_size)
        self.blocks = BlockSequence(
            depth=depth, embed_channels=embed_channels, groups=groups, neighbours=neighbours, qkv_bias=qkv_bias,
            pe_multiplier=pe_multiplier, pe_bias=pe_bias,
            attn_drop_rate=attn_drop_rate if attn_drop_rate is not None else 0.0,
            drop_path_rate=drop_path_rate if drop_path_rate is not None else 0.0, enable_checkpoint=enable_checkpoint)

    def forward(self, points):
        points, cluster = self.down(points)
        return self.blocks(points), cluster


class Decoder(nn.Module):
    def __init__(self, in_channels, skip_channels, embed_channels, groups, depth, neighbours=16, qkv_bias=True,
                 pe_multiplier=False, pe_bias=True, attn_drop_rate=None, drop_path_rate=None, enable_checkpoint=False,
                 unpool_backend="map"):
        super().__init__()
        self.up = UnpoolWithSkip(in_channels=in_channels, out_channels=embed_channels, skip_channels=skip_channels,
                                 backend=unpool_backend)
        self.blocks = BlockSequence(
            depth=depth, embed_channels=embed_channels, groups=groups, neighbours=neighbours, qkv_bias=qkv_bias,
            pe_multiplier=pe_multiplier, pe_bias=pe_bias,
            attn_drop_rate=attn_drop_rate if attn_drop_rate is not None else 0.0,
            drop_path_rate=drop_path_rate if drop_path_rate is not None else 0.0, enable_checkpoint=enable_checkpoint)

    def forward(self, points, skip_points, cluster):
        return self.blocks(self.up(points, skip_points, cluster))


class GVAPatchEmbed(nn.Module):
    def __init__(self, depth, in_channels, embed_channels, groups, neighbours=16, qkv_bias=True, pe_multiplier=False,
                 pe_bias=True, attn_drop_rate=0.0, drop_path_rate=0.0, enable_checkpoint=False):
        super().__init__()
        self.in_channels, self.embed_channels = in_channels, embed_channels
        self.proj = _proj(in_channels, embed_channels, False)
        self.blocks = BlockSequence(
            depth=depth, embed_channels=embed_channels, groups=groups, neighbours=neighbours, qkv_bias=qkv_bias,
            pe_multiplier=pe_multiplier, pe_bias=pe_bias, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate,
            enable_checkpoint=enable_checkpoint)
        self.fused = True
        self._cache = _ParamCache()

    def forward(self, points):
        coord, feat, offset = points[:3]
        if self.fused and not self.training:
            feat = _proj_fused(feat.float(), self.proj, self._cache)     # _linear pads the input width to the K granule
        else:
            feat = self.proj(feat)
        return self.blocks([coord, feat, offset] + list(points[3:]))


@MODELS.register_module("PT-v2m2")
class PointTransformerV2(nn.Module):
    def __init__(self, in_channels, num_classes, patch_embed_depth=1, patch_embed_channels=48, patch_embed_groups=6,
                 patch_embed_neighbours=8, enc_depths=(2, 2, 6, 2), enc_channels=(96, 192, 384, 512),
                 enc_groups=(12, 24, 48, 64), enc_neighbours=(16, 16, 16, 16), dec_depths=(1, 1, 1, 1),
                 dec_channels=(48, 96, 192, 384), dec_groups=(6, 12, 24, 48), dec_neighbours=(16, 16, 16, 16),
                 grid_sizes=(0.06, 0.12, 0.24, 0.48), attn_qkv_bias=True, pe_multiplier=False, pe_bias=True,
                 attn_drop_rate=0.0, drop_path_rate=0, enable_checkpoint=False, unpool_backend="map"):
        super().__init__()
        self.in_channels, self.num_classes = in_channels, num_classes
        self.num_stages = len(enc_depths)
        for seq in (dec_depths, enc_channels, dec_channels, enc_groups, dec_groups, enc_neighbours, dec_neighbours,
                    grid_sizes):
            assert self.num_stages == len(seq)
        shared = dict(qkv_bias=attn_qkv_bias, pe_multiplier=pe_multiplier, pe_bias=pe_bias,
                      attn_drop_rate=attn_drop_rate, enable_checkpoint=enable_checkpoint)
        self.patch_embed = GVAPatchEmbed(in_channels=in_channels, embed_channels=patch_embed_channels,
                                         groups=patch_embed_groups, depth=patch_embed_depth,
                                         neighbours=patch_embed_neighbours, **shared)
        enc_dp = [x.item() for x in torch.linspace(0, drop_path_rate, sum(enc_depths))]
        dec_dp = [x.item() for x in torch.linspace(0, drop_path_rate, sum(dec_depths))]
        enc_channels = [patch_embed_channels] + list(enc_channels)
        dec_channels = list(dec_channels) + [enc_channels[-1]]
        self.enc_stages = nn.ModuleList()
        self.dec_stages = nn.ModuleList()
        for i in range(self.num_stages):
            self.enc_stages.append(Encoder(
                depth=enc_depths[i], in_channels=enc_channels[i], embed_channels=enc_channels[i + 1],
                groups=enc_groups[i], grid_size=grid_sizes[i], neighbours=enc_neighbours[i],
                drop_path_rate=enc_dp[sum(enc_depths[:i]):sum(enc_depths[:i + 1])], **shared))
            self.dec_stages.append(Decoder(
                depth=dec_depths[i], in_channels=dec_channels[i + 1], skip_channels=enc_channels[i],
                embed_channels=dec_channels[i], groups=dec_groups[i], neighbours=dec_neighbours[i],
                drop_path_rate=dec_dp[sum(dec_depths[:i]):sum(dec_depths[:i + 1])], unpool_backend=unpool_backend,
                **shared))
        self.seg_head = nn.Sequential(
            nn.Linear(dec_channels[0], dec_channels[0]), PointBatchNorm(dec_channels[0]), nn.ReLU(inplace=True),
            nn.Linear(dec_channels[0], num_classes)) if num_classes > 0 else nn.Identity()

    def set_fused(self, fused):
        """fused = False: eval runs the training path's torch composition (running-statistic BatchNorm) instead of the
        fused kernels - what the fused path is tested against."""
        for m in self.modules():
            if hasattr(m, "fused"):
                m.fused = bool(fused)
        return self

    def forward(self, data_dict):
        coord = data_dict["coord"].float().contiguous()
        feat = data_dict["feat"]
        so = data_dict.get("scene_offsets")
        if so is None:
            so = SceneOffsets.read(data_dict["offset"])       # the forward's one read of `offset`
        sizes = [b - a for a, b in zip([0] + so.host[:-1], so.host)]
        if not sizes or min(sizes) < 1:
            raise ValueError(f"PT-v2m2: a scene without points (scene sizes {sizes})")
        if so.host[-1] != coord.shape[0]:
            raise ValueError(f"PT-v2m2: offset ends at {so.host[-1]} for {coord.shape[0]} points")
        points = self.patch_embed([coord, feat, so.dev, so])
        skips = [[points]]
        for i in range(self.num_stages):
            points, cluster = self.enc_stages[i](points)
            skips[-1].append(cluster)
            skips.append([points])
        points = skips.pop(-1)[0]
        for i in reversed(range(self.num_stages)):
            skip_points, cluster = skips.pop(-1)
            points = self.dec_stages[i](points, skip_points, cluster)
        feat = points[1]
        if self.num_classes > 0:
            feat = self.seg_head(feat)
        return feat
