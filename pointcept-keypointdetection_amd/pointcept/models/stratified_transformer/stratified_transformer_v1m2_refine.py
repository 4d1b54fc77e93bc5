"""Stratified Transformer (ST-v1m2) on MI355X.

Counterpart of the reference's pointcept/models/stratified_transformer/stratified_transformer_v1m2_refine.py: the same
constructor arguments, attribute names and state_dict keys (a reference checkpoint loads with strict=True), registry
name "ST-v1m2".

`.eval()` with `fused = True` (the default): `offset` is read from the device once and every level's sample counts
follow on the host; each BasicLayer builds one attention plan per parity (ops.stratified_plan: the groups of queries
that share a small and a large window, and each group's keys; one host read per plan) and every block attends with one
launch of ptv3_strat_attn_fwd.  LayerNorm, the linear layers, GELU and the residuals around it run in ptv3_layernorm /
ptv3_gemm; farthest point sampling, kNN, grouping, interpolation and the ball query are HIP kernels as well.
`.train()`, or `set_fused(False)`: the reference's formulas over the `pointops2` compositions on the edge list, which
is expanded from the same plan on the device; autograd carries the backward (a HIP backward of the attention is the
follow-up).

Deliberate differences from the reference, all documented in DESIGN.md section 18:
  * shifted blocks decide "same small window" with the voxel_grid expression ((x + w/2) - min) / w that also forms the
    windows, not with (x - min + w/2) / w (:423), which can differ by rounding at a cell face;
  * KPConvLayer / FastBatchNorm1d (torch_points3d) and the partial_dense ball query (torch_points_kernels) are not in
    the reference tree and are restated from their published semantics; a fresh KPConvLayer gets a deterministic
    kernel-point disposition that is NOT torch_points3d's optimised one (a checkpoint brings its own K_points).
Two quirks are reproduced: BasicLayer samples int(n_b * ratio) + 1 rows per scene (:361-367) while TransitionDown
accumulates n_b * ratio + 1 without int() and lets IntTensor truncate the running sum (:470-476).
"""
import math

import torch
import torch.nn as nn

import pointops2.pointops as pointops
from pointops import _C, functions as _po
from ptv3_hip import ops
from pointcept.models.builder import MODELS
from pointcept.models.point_transformer.point_transformer_seg import SceneOffsets
from pointcept.models.utils.hip_layers import Linear, LayerNorm, BatchNorm1d, DropPath, check_sync_batchnorm
from pointcept.models.utils.sparse import _ParamCache


def _scatter_softmax(src, index_0, n):
    """torch_scatter.scatter_softmax(src, index_0, dim=0) for (M, h) logits (the maximum is a constant of the softmax)."""
    idx = index_0.view(-1, 1).expand_as(src)
    mx = torch.full((n, src.shape[1]), -float("inf"), dtype=src.dtype, device=src.device)
    mx = mx.scatter_reduce(0, idx, src.detach(), "amax", include_self=True)
    e = torch.exp(src - mx.gather(0, idx))
    return e / torch.zeros_like(mx).scatter_add(0, idx, e).gather(0, idx)


def basic_layer_counts(sizes, ratio):
    """BasicLayer.forward :361-367: int(n_b * ratio) + 1 samples of every scene -> cumulative ends."""
    out, total = [], 0
    for n in sizes:
        total += int(n * ratio) + 1
        out.append(total)
    return out


def transition_down_counts(sizes, ratio):
    """TransitionDown.forward :470-476: the first scene as above, the others add n_b * ratio + 1 WITHOUT int(), and
    torch.cuda.IntTensor truncates the running (float) sum."""
    total = int(sizes[0] * ratio) + 1
    out = [total]
    for n in sizes[1:]:
        total += (n * ratio) + 1
        out.append(total)
    return [int(v) for v in out]


def _sizes(ends):
    return [e - s for s, e in zip([0] + list(ends[:-1]), ends)]


def _level(host, device):
    return SceneOffsets(host, torch.tensor(host, dtype=torch.int32, device=device))


@torch.no_grad()
def _knn2(nsample, xyz, so, new_xyz, new_so):
    """pointops2.knnquery without its read-back of the offsets (the host copies were checked already): idx with a short
    scene padded by its first row, and the distances (sqrt(1e10) in a padded slot)."""
    if so.host[-1] != xyz.shape[0] or new_so.host[-1] != new_xyz.shape[0]:
        raise ValueError(f"offsets end at {so.host[-1]} / {new_so.host[-1]} for {xyz.shape[0]} / {new_xyz.shape[0]} rows")
    m = new_xyz.shape[0]
    idx = torch.zeros((m, nsample), dtype=torch.int32, device=xyz.device)
    dist2 = torch.zeros((m, nsample), dtype=torch.float32, device=xyz.device)
    _C.knn_query_cuda(m, nsample, xyz, new_xyz, so.dev, new_so.dev, idx, dist2)
    return pointops._pad_first_row(idx, new_so.dev, so.dev).contiguous(), dist2.sqrt_()


class WindowAttention(nn.Module):
    def __init__(self, embed_channels, num_heads, window_size, quant_size, attn_drop=0.0, proj_drop=0.0, scale=None,
                 rel_query=True, rel_key=True, rel_value=True, qkv_bias=True):
        super().__init__()
        self.embed_channels, self.num_heads = embed_channels, num_heads
        self.head_channels = embed_channels // num_heads
        self.scale = scale or self.head_channels ** -0.5
        self.window_size, self.quant_size = window_size, quant_size
        self.rel_query, self.rel_key, self.rel_value = rel_query, rel_key, rel_value
        self.quant_grid_length = int((2 * window_size + 1e-4) // quant_size)
        if not (rel_query and rel_key and rel_value):
            raise NotImplementedError("WindowAttention: only rel_query = rel_key = rel_value = True (the fork config) is "
                                      "built on the HIP path")
        shape = (2 * self.quant_grid_length, num_heads, self.head_channels, 3)
        self.relative_pos_query_table = nn.Parameter(torch.zeros(shape))
        self.relative_pos_key_table = nn.Parameter(torch.zeros(shape))
        self.relative_pos_value_table = nn.Parameter(torch.zeros(shape))
        # the reference draws the QUERY table three times (:119, :127, :135) and leaves the other two at zero
        nn.init.trunc_normal_(self.relative_pos_query_table, std=0.02)
        self.qkv = Linear(embed_channels, embed_channels * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop, inplace=True)
        self.proj = Linear(embed_channels, embed_channels)
        self.proj_drop = nn.Dropout(proj_drop, inplace=True)
        self.softmax = nn.Softmax(dim=-1)
        self._cache = _ParamCache()

    @property
    def table_rows(self):
        return 2 * self.quant_grid_length

    def packed_tables(self):
        params = [self.relative_pos_query_table, self.relative_pos_key_table, self.relative_pos_value_table]
        return self._cache.get("tables", params, lambda: tuple(ops.strat_pack_tables(t) for t in params))

    def forward_fused(self, feats, coords, plan):
        """One launch of ptv3_strat_attn_fwd between qkv and proj."""
        n, c = feats.shape
        if not ops.strat_attn_capable(self.num_heads, self.head_channels, self.table_rows):
            raise NotImplementedError(
                f"WindowAttention: heads={self.num_heads}, head_dim={self.head_channels}, table_rows={self.table_rows} "
                "is not served by ptv3_strat_attn_fwd (head_dim 16, at most 80 table rows); set_fused(False) runs the "
                "edge composition")
        qkv = self.qkv(feats).view(n, 3, self.num_heads, self.head_channels)
        tq, tk, tv = self.packed_tables()
        x = ops.stratified_attention(qkv, coords, plan, tq, tk, tv, self.scale, self.window_size, self.quant_size)
        return self.proj(x.view(n, c))

    def forward(self, feats, coords, index_0, index_1, index_0_offsets, n_max):
        """The reference's WindowAttention.forward (:144-225) over the edge list."""
        n, c = feats.shape
        qkv = self.qkv(feats).reshape(n, 3, self.num_heads, c // self.num_heads).permute(1, 0, 2, 3).contiguous()
        query, key, value = qkv[0], qkv[1], qkv[2]
        query = query * self.scale
        attn_flat = pointops.attention_step1_v2(query.float(), key.float(), index_1, index_0_offsets, n_max)
        rel = pointops.relative_position_index(coords, index_0, index_1, self.window_size, self.quant_size,
                                               self.table_rows)
        bias = pointops.dot_prod_with_idx_v3(query.float(), index_0_offsets, n_max, key.float(), index_1,
                                             self.relative_pos_query_table.float(),
                                             self.relative_pos_key_table.float(), rel)
        attn_flat = _scatter_softmax(attn_flat + bias, index_0, n)
        x = pointops.attention_step2_with_rel_pos_value_v2(attn_flat, value.float(), index_0_offsets, n_max, index_1,
                                                           self.relative_pos_value_table.float(), rel)
        x = self.proj(x.view(n, c))
        return self.proj_drop(x)


class MLP(nn.Module):
    def __init__(self, in_channels, hidden_channels=None, out_channels=None, drop=0.0):
        super().__init__()
        out_channels = out_channels or in_channels
        hidden_channels = hidden_channels or in_channels
        self.fc1 = Linear(in_channels, hidden_channels)
        self.act = nn.GELU()
        self.fc2 = Linear(hidden_channels, out_channels)
        self.drop = nn.Dropout(drop, inplace=True)

    def forward(self, x, res=None):
        x = self.drop(self.fc1(x, act=ops.ACT_GELU))
        if res is not None and not self.training:
            return self.fc2(x, res=res)
        x = self.drop(self.fc2(x))
        return x if res is None else res + x


class Block(nn.Module):
    def __init__(self, embed_channels, num_heads, window_size, quant_size, mlp_expend_ratio=4.0, drop_path=0.0,
                 qk_scale=None, rel_query=True, rel_key=True, rel_value=True, qkv_bias=True):
        super().__init__()
        self.norm1 = LayerNorm(embed_channels)
        self.attn = WindowAttention(embed_channels, num_heads, window_size, quant_size, scale=qk_scale,
                                    rel_query=rel_query, rel_key=rel_key, rel_value=rel_value, qkv_bias=qkv_bias)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = LayerNorm(embed_channels)
        self.mlp = MLP(in_channels=embed_channels, hidden_channels=int(embed_channels * mlp_expend_ratio))

    def forward(self, feats, coords, plan, edges=None):
        short_cut = feats
        feats = self.norm1(feats)
        if edges is None:
            feats = self.attn.forward_fused(feats, coords, plan)
        else:
            feats = self.attn(feats, coords, *edges)
        feats = short_cut + self.drop_path(feats)
        if self.training:
            return feats + self.drop_path(self.mlp(self.norm2(feats)))
        return self.mlp(self.norm2(feats), res=feats)


class BasicLayer(nn.Module):
    def __init__(self, embed_channels, out_channels, depth, num_heads, window_size, quant_size, mlp_expend_ratio=4.0,
                 down_ratio=0.25, down_num_sample=16, drop_path=None, qk_scale=None, down=True, rel_query=True,
                 rel_key=True, rel_value=True, qkv_bias=True):
        super().__init__()
        self.depth, self.window_size, self.quant_size, self.down_ratio = depth, window_size, quant_size, down_ratio
        if isinstance(drop_path, list):
            assert len(drop_path) == depth
        elif isinstance(drop_path, float):
            drop_path = [drop_path] * depth
        else:
            drop_path = [0.0] * depth
        self.blocks = nn.ModuleList(
            Block(embed_channels, num_heads, window_size, quant_size, mlp_expend_ratio=mlp_expend_ratio,
                  drop_path=drop_path[i], qk_scale=qk_scale, rel_query=rel_query, rel_key=rel_key, rel_value=rel_value,
                  qkv_bias=qkv_bias) for i in range(depth))
        self.down = TransitionDown(embed_channels, out_channels, down_ratio, down_num_sample) if down else None
        self.fused = True
        self.record = None     # a dict, when a test asks for the sampled rows and the plans

    def forward(self, feats, coords, so):
        coords = coords.contiguous()
        nso = _level(basic_layer_counts(_sizes(so.host), self.down_ratio), coords.device)
        down_idx = ops.farthest_point_sampling(coords, so.dev, nso.dev, so.host, nso.host)
        cmin = coords.min(0).values
        plans = [ops.stratified_plan(coords, so.dev, down_idx, self.window_size, bool(parity), cmin)
                 for parity in range(min(self.depth, 2))]
        if self.record is not None:
            self.record.update(down_idx=down_idx, plans=plans)
        fused = self.fused and not self.training
        edges = [None, None]
        n = coords.shape[0]
        for i, blk in enumerate(self.blocks):
            plan = plans[i % 2]
            if not fused and edges[i % 2] is None:
                index_0, index_1 = plan.edges()
                counts = torch.bincount(index_0, minlength=n)
                offsets = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
                edges[i % 2] = (index_0, index_1, offsets, None)
            feats = blk(feats, coords, plan, None if fused else edges[i % 2])
        if self.down is not None:
            feats_down, coords_down, so_down = self.down(feats, coords, so)
        else:
            feats_down, coords_down, so_down = None, None, None
        return feats, coords, so, feats_down, coords_down, so_down


class TransitionDown(nn.Module):
    def __init__(self, in_channels, out_channels, ratio, k, norm_layer=nn.LayerNorm):
        super().__init__()
        self.ratio, self.k = ratio, k
        self.norm = LayerNorm(in_channels) if norm_layer else None
        self.linear = Linear(in_channels, out_channels, bias=False)
        self.pool = nn.MaxPool1d(k)

    def forward(self, feats, coords, so):
        coords = coords.contiguous()
        nso = _level(transition_down_counts(_sizes(so.host), self.ratio), coords.device)
        idx = ops.farthest_point_sampling(coords, so.dev, nso.dev, so.host, nso.host)
        new_coords = coords[idx.long(), :].contiguous()
        knn, _ = _knn2(self.k, coords, so, new_coords, nso)
        feats = pointops.queryandgroup(self.k, coords, new_coords, feats.contiguous(), knn, so.dev, nso.dev,
                                       use_xyz=False)                                   # (m, k, c)
        m, k, c = feats.shape
        feats = feats.view(m * k, c)
        if self.norm is not None:
            feats = self.norm(feats)
        feats = self.linear(feats).view(m, k, -1).max(dim=1).values                     # MaxPool1d(k) over the neighbours
        return feats, new_coords, nso


class TransitionUp(nn.Module):
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.linear1 = nn.Sequential(LayerNorm(out_channels), Linear(out_channels, out_channels))
        self.linear2 = nn.Sequential(LayerNorm(in_channels), Linear(in_channels, out_channels))

    def forward(self, feats, coords, so, skip_feats, skip_coords, skip_so):
        up = self.linear2(feats).contiguous()
        knn, dist = _knn2(3, coords.contiguous(), so, skip_coords.contiguous(), skip_so)
        w = torch.reciprocal(dist + 1e-8)
        w = (w / w.sum(dim=1, keepdim=True)).contiguous()
        feats = self.linear1(skip_feats) + _po._KnnBlend.apply(up, knn.contiguous(), w)
        return feats, skip_coords, skip_so


def kernel_point_disposition(radius, n=15):
    """A deterministic disposition of n kernel points in the ball of `radius`: the centre, then a Fibonacci spiral on the
    sphere of 0.66 radius.  NOT torch_points3d's optimised disposition (its load_kernels reads or optimises a file that is
    not in the reference tree); a checkpoint overwrites it with its own K_points."""
    pts = [[0.0, 0.0, 0.0]]
    golden = math.pi * (3.0 - math.sqrt(5.0))
    for i in range(n - 1):
        z = 1.0 - 2.0 * (i + 0.5) / (n - 1)
        r = math.sqrt(max(0.0, 1.0 - z * z))
        pts.append([0.66 * radius * r * math.cos(golden * i), 0.66 * radius * r * math.sin(golden * i),
                    0.66 * radius * z])
    return torch.tensor(pts, dtype=torch.float32)


class KPConvLayer(nn.Module):
    """torch_points3d.modules.KPConv.kernels.KPConvLayer restated from its published source (parity unpinned): rigid
    kernel points, linear influence max(0, 1 - |y - K_k| / point_influence), sum aggregation; neighbour index -1 reads a
    shadow point at 1e6 with zero features."""
    _INFLUENCE_TO_RADIUS = 1.5

    def __init__(self, num_inputs, num_outputs, point_influence, n_kernel_points=15, add_one=False, **kwargs):
        super().__init__()
        if add_one:
            raise NotImplementedError("KPConvLayer: add_one is not used by ST-v1m2")
        self.kernel_radius = self._INFLUENCE_TO_RADIUS * point_influence
        self.point_influence, self.n_kernel_points = point_influence, n_kernel_points
        self.num_inputs, self.num_outputs = num_inputs, num_outputs
        self.K_points = nn.Parameter(kernel_point_disposition(self.kernel_radius, n_kernel_points), requires_grad=False)
        self.weight = nn.Parameter(torch.empty(n_kernel_points, num_inputs, num_outputs))
        nn.init.xavier_normal_(self.weight)

    def forward(self, query_points, support_points, neighbors, x):
        support = torch.cat([support_points, torch.full_like(support_points[:1], 1e6)], 0)
        rel = support[neighbors] - query_points.unsqueeze(1)                      # (n, m, 3); -1 reads the shadow row
        sq = (rel.unsqueeze(2) - self.K_points).square().sum(3)                   # (n, m, K)
        w = torch.clamp(1 - torch.sqrt(sq) / self.point_influence, min=0.0).transpose(2, 1)   # (n, K, m)
        feats = torch.cat([x, torch.zeros_like(x[:1])], 0)[neighbors]             # (n, m, in)
        weighted = torch.matmul(w, feats).permute(1, 0, 2)                        # (K, n, in)
        return torch.matmul(weighted, self.weight).sum(0)


class FastBatchNorm1d(nn.Module):
    """torch_points3d.core.common_modules.FastBatchNorm1d on (n, c) rows: a BatchNorm1d under `batch_norm`."""

    def __init__(self, num_features, momentum=0.1, **kwargs):
        super().__init__()
        self.batch_norm = BatchNorm1d(num_features, momentum=momentum, **kwargs)

    def forward(self, x, act=ops.ACT_NONE):
        return self.batch_norm(x.contiguous(), act=act)


class KPConvSimpleBlock(nn.Module):
    def __init__(self, in_channels, out_channels, prev_grid_size, sigma=1.0, negative_slope=0.2, bn_momentum=0.02):
        super().__init__()
        self.kpconv = KPConvLayer(in_channels, out_channels, point_influence=prev_grid_size * sigma, add_one=False)
        self.bn = FastBatchNorm1d(out_channels, momentum=bn_momentum)
        self.activation = nn.LeakyReLU(negative_slope=negative_slope)

    def forward(self, feats, xyz, batch, neighbor_idx):
        return self.activation(self.bn(self.kpconv(xyz, xyz, neighbor_idx, feats)))


class KPConvResBlock(nn.Module):
    def __init__(self, in_channels, out_channels, prev_grid_size, sigma=1.0, negative_slope=0.2, bn_momentum=0.02):
        super().__init__()
        d_2 = out_channels // 4
        activation = nn.LeakyReLU(negative_slope=negative_slope)
        self.unary_1 = nn.Sequential(Linear(in_channels, d_2, bias=False), FastBatchNorm1d(d_2, momentum=bn_momentum),
                                     activation)
        self.unary_2 = nn.Sequential(Linear(d_2, out_channels, bias=False),
                                     FastBatchNorm1d(out_channels, momentum=bn_momentum), activation)
        self.kpconv = KPConvLayer(d_2, d_2, point_influence=prev_grid_size * sigma, add_one=False)
        self.bn = FastBatchNorm1d(out_channels, momentum=bn_momentum)   # a parameter holder, as in the reference: unused
        self.activation = activation
        if in_channels != out_channels:
            self.shortcut_op = nn.Sequential(Linear(in_channels, out_channels, bias=False),
                                             FastBatchNorm1d(out_channels, momentum=bn_momentum))
        else:
            self.shortcut_op = nn.Identity()

    def forward(self, feats, xyz, batch, neighbor_idx):
        shortcut = feats
        feats = self.unary_1(feats)
        feats = self.kpconv(xyz, xyz, neighbor_idx, feats)
        feats = self.unary_2(feats)
        return feats + self.shortcut_op(shortcut)


@MODELS.register_module("ST-v1m2")
class StratifiedTransformer(nn.Module):
    def __init__(self, in_channels, num_classes, channels=(48, 96, 192, 384, 384), num_heads=(6, 12, 24, 24),
                 depths=(3, 9, 3, 3), window_size=(0.2, 0.4, 0.8, 1.6), quant_size=(0.01, 0.02, 0.04, 0.08),
                 mlp_expend_ratio=4.0, down_ratio=0.25, down_num_sample=16, kp_ball_radius=2.5 * 0.02,
                 kp_max_neighbor=34, kp_grid_size=0.02, kp_sigma=1.0, drop_path_rate=0.2, rel_query=True, rel_key=True,
                 rel_value=True, qkv_bias=True, stem=True):
        super().__init__()
        dpr = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        self.kp_ball_radius, self.kp_max_neighbor, self.stem = kp_ball_radius, kp_max_neighbor, stem
        if stem:
            self.point_embed = nn.ModuleList([
                KPConvSimpleBlock(in_channels, channels[0], kp_grid_size, sigma=kp_sigma),
                KPConvResBlock(channels[0], channels[0], kp_grid_size, sigma=kp_sigma)])
            self.down = TransitionDown(channels[0], channels[1], down_ratio, down_num_sample)
        else:
            assert channels[0] == channels[1]
            self.point_embed = nn.ModuleList([KPConvSimpleBlock(in_channels, channels[1], kp_grid_size, sigma=kp_sigma)])
        num_layers = len(depths)
        self.layers = nn.ModuleList(
            BasicLayer(embed_channels=channels[i + 1],
                       out_channels=channels[i + 2] if i < num_layers - 1 else channels[i + 1], depth=depths[i],
                       num_heads=num_heads[i], window_size=window_size[i], quant_size=quant_size[i],
                       mlp_expend_ratio=mlp_expend_ratio, down_ratio=down_ratio, down_num_sample=down_num_sample,
                       drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], rel_query=rel_query, rel_key=rel_key,
                       rel_value=rel_value, qkv_bias=qkv_bias, down=i < num_layers - 1) for i in range(num_layers))
        self.up = nn.ModuleList([TransitionUp(channels[i + 1], channels[i]) for i in reversed(range(1, num_layers))])
        if self.stem:
            self.up.append(TransitionUp(channels[1], channels[0]))
        self.classifier = nn.Sequential(Linear(channels[0], channels[0]), BatchNorm1d(channels[0]),
                                        nn.ReLU(inplace=True), Linear(channels[0], num_classes))
        self.init_weights()

    def set_fused(self, fused):
        """fused = False: eval attends through the pointops2 edge composition instead of ptv3_strat_attn_fwd - what the
        fused path is tested and measured against."""
        for m in self.modules():
            if isinstance(m, BasicLayer):
                m.fused = bool(fused)
        return self

    def backbone(self, data_dict):
        """(n, channels[0]) point features and the level-0 SceneOffsets."""
        check_sync_batchnorm(self)
        feats = data_dict["feat"].float().contiguous()
        coords = data_dict["coord"].float().contiguous()
        offset = data_dict["offset"]
        so = SceneOffsets.read(offset)                  # the forward's one read of the offsets
        if so.host[-1] != coords.shape[0] or min(_sizes(so.host)) < 1:
            raise ValueError(f"StratifiedTransformer: offsets {so.host} do not describe {coords.shape[0]} points in "
                             "non-empty scenes")
        neighbor_idx = ops.ball_query(self.kp_ball_radius, self.kp_max_neighbor, coords, so.dev, so.host)
        feats_stack, coords_stack, so_stack = [], [], []
        for layer in self.point_embed:
            feats = layer(feats, coords, None, neighbor_idx)
        feats = feats.contiguous()
        if self.stem:
            feats_stack.append(feats)
            coords_stack.append(coords)
            so_stack.append(so)
            feats, coords, so = self.down(feats, coords, so)
        for layer in self.layers:
            feats, coords, so, feats_down, coords_down, so_down = layer(feats, coords, so)
            feats_stack.append(feats)
            coords_stack.append(coords)
            so_stack.append(so)
            feats, coords, so = feats_down, coords_down, so_down
        feats, coords, so = feats_stack.pop(), coords_stack.pop(), so_stack.pop()
        for up in self.up:
            feats, coords, so = up(feats, coords, so, feats_stack.pop(), coords_stack.pop(), so_stack.pop())
        return feats, so

    def forward(self, data_dict):
        feats, _ = self.backbone(data_dict)
        lin0, bn, _, lin1 = self.classifier
        return lin1(bn(lin0(feats), act=ops.ACT_RELU))

    def init_weights(self):
        def _init_weights(m):
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, (nn.LayerNorm, nn.BatchNorm1d)):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)
        self.apply(_init_weights)
