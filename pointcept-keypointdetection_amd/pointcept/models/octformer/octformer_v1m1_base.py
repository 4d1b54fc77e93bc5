"""OctFormer-v1m1 on MI355X.

Counterpart of the reference's pointcept/models/octformer/octformer_v1m1_base.py: the same classes, constructor
arguments, parameter and buffer names and shapes, so a fork checkpoint loads with strict=True.  The reference leans on
three packages this tree does not carry (ocnn, dwconv, torch_scatter); their behaviour is restated here from the
published sources and their parity is UNPINNED (DESIGN.md section 19 lists every restated rule).

The octree comes from ops.octree_build (one key kernel, one sort, one segment pass per depth, one host read); with
nempty=True, the only mode the fork uses, every tensor of a depth has one row per non-empty node in key order.  In eval
an OctFormerBlock is ptv3_octree_dwconv, ptv3_layernorm, ptv3_gemm and ptv3_octree_attn_fwd: no padded copy, no mask,
no gathered RPE.  The 3^3 convolutions and the stride-2 deconvolution run through ptv3_gemm over a 27-tap table with the
BatchNorm and ReLU folded into its epilogue, the kernel-2 / stride-2 convolutions through ptv3_down2_conv.  Training, and
eval after set_fused(False), run the same plan composed in torch with autograd (ops.octree_attention_torch is the
reference's algorithm); a HIP backward is the follow-up.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils.checkpoint import checkpoint

from pointcept.models.builder import MODELS
from ptv3_hip import ops

BN_EPS, BN_MOMENTUM = 1e-3, 0.01   # ocnn.modules' BatchNorm1d settings


def octree_cells(coord, scale_factor, depth):
    """(n, 3) int64 leaf cells of ocnn's Points / Octree.build_octree in torch (what ptv3_octree_keys evaluates):
    p = coord / scale_factor, cell = floor((p + 1) * 2^(depth-1)) in fp32; a point outside -1 <= p < 1 raises."""
    p = coord.float() / scale_factor
    if not bool(((p >= -1) & (p < 1)).all()):
        raise ValueError(f"octree_cells: a point lies outside -1 <= coord / {scale_factor} < 1 (the octree's domain)")
    return torch.floor((p + 1.0) * float(2 ** (depth - 1))).long()


class _Fusable(nn.Module):
    fused = True

    def _hip(self, x):
        return self.fused and not self.training and x.is_cuda and x.dtype == torch.float32


def _gather_rows(x, idx):
    """x[idx] with a zero row for idx < 0"""
    xp = torch.cat([x, x.new_zeros((1, x.shape[1]))])
    return xp[torch.where(idx >= 0, idx, x.shape[0]).long()]


class OctreeT:
    """The reference's OctreeT(Octree): an ops.OctreeLevels plus the patch settings.  Its batch_idx / patch_mask /
    rel_pos tensors are not built: the attention reads the node coordinates and scene ids of the depth."""

    def __init__(self, octree, patch_size=24, dilation=4, nempty=True, max_depth=None, start_depth=None, **kwargs):
        if not nempty:
            raise NotImplementedError("OctreeT: only nempty=True (the fork's mode) is built")
        self.levels = octree
        self.patch_size, self.dilation, self.nempty = patch_size, dilation, nempty
        self.max_depth = max_depth or octree.depth
        self.start_depth = start_depth or octree.min_depth
        self.invalid_mask_value = -1e3
        assert self.start_depth > 1
        self.block_num = patch_size * dilation

    def __getattr__(self, name):
        return getattr(self.__dict__["levels"], name)


class MLP(_Fusable):
    def __init__(self, in_features, hidden_features=None, out_features=None, activation=nn.GELU, drop=0.0, **kwargs):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features or in_features
        self.hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(self.in_features, self.hidden_features)
        self.act = activation()
        self.fc2 = nn.Linear(self.hidden_features, self.out_features)
        self.drop = nn.Dropout(drop, inplace=True)

    def forward(self, data, res=None):
        if self._hip(data) and isinstance(self.act, nn.GELU):
            h = ops.gemm(data, self.fc1.weight, bias=self.fc1.bias, act=ops.ACT_GELU)
            return ops.gemm(h, self.fc2.weight, bias=self.fc2.bias, res=res)
        data = self.drop(self.fc2(self.drop(self.act(self.fc1(data)))))
        return data if res is None else res + data


class OctreeConv(_Fusable):
    """ocnn.nn.OctreeConv / OctreeDeconv restated for nempty=True: weights (kdim, cin, cout) ((kdim, cout, cin) for the
    deconvolution), taps x outermost.  kernel [3] stride 1: the 27 neighbours; kernel [2] stride 2: a parent sums its
    children, tap (x&1)*4 + (y&1)*2 + (z&1); deconvolution [3] stride 2: the transpose of the stride-2 3^3 convolution
    whose window of parent P covers the fine cells 2P + {-1, 0, 1}.  forward(data, octree, depth) takes the rows of
    `depth` and returns those of depth (stride 1), depth - 1 (stride 2) or depth + 1 (deconvolution)."""

    def __init__(self, in_channels, out_channels, kernel_size=(3,), stride=1, nempty=True, use_bias=False, deconv=False):
        super().__init__()
        if not nempty:
            raise NotImplementedError("OctreeConv: only nempty=True (the fork's mode) is built")
        k = list(kernel_size)
        self.mode = ("deconv" if deconv else "conv") + f"{k[0]}s{stride}"
        if len(set(k)) != 1 or self.mode not in ("conv3s1", "conv2s2", "deconv3s2"):
            raise NotImplementedError(f"OctreeConv: kernel {k} stride {stride} deconv={deconv} is not built")
        self.in_channels, self.out_channels = in_channels, out_channels
        cin, cout = (out_channels, in_channels) if deconv else (in_channels, out_channels)
        self.weights = nn.Parameter(torch.empty(k[0] ** 3, cin, cout))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if use_bias else None
        nn.init.xavier_uniform_(self.weights)

    def table(self, octree, depth):
        if self.mode == "conv3s1":
            return octree.neighbors(depth)
        return octree.children[depth - 1] if self.mode == "conv2s2" else octree.deconv_table(depth)

    def forward(self, data, octree, depth, bn_scale=None, bn_shift=None, act=ops.ACT_NONE):
        """bn_scale / bn_shift / act: the folded epilogue, for the fused eval path of the modules around this one"""
        tab = self.table(octree, depth)
        if bn_scale is not None and self.in_channels % 4 == 0:
            if self.mode == "conv2s2":
                w = self.weights.detach().permute(2, 0, 1).contiguous()
                return ops.down2_conv(data.contiguous(), w, octree.down_plan(depth), bn_scale, bn_shift, act)
            if self.mode == "deconv3s2":
                # ptv3_gemm addresses x as the feature matrix of the table's rows: give it that many rows
                x = data.new_zeros((tab.shape[0], data.shape[1]))
                x[:data.shape[0]] = data
                w = self.weights.detach().permute(1, 0, 2).contiguous()
            else:
                x, w = data.contiguous(), self.weights.detach().permute(2, 0, 1).contiguous()
            return ops.gemm(x, w, nbr=tab, kvol=27, bn_scale=bn_scale, bn_shift=bn_shift, act=act)
        out = data.new_zeros((tab.shape[0], self.out_channels))
        for t in range(tab.shape[1]):
            w = self.weights[t].t() if self.mode == "deconv3s2" else self.weights[t]
            out = out + _gather_rows(data, tab[:, t]) @ w
        if self.bias is not None:
            out = out + self.bias
        if bn_scale is not None:
            out = out * bn_scale + bn_shift
            out = F.relu(out) if act == ops.ACT_RELU else out
        return out


class OctreeConvBnRelu(_Fusable):
    """ocnn.modules.OctreeConvBnRelu / OctreeDeconvBnRelu (the convolution is `conv` or `deconv`, as there)"""

    def __init__(self, in_channels, out_channels, kernel_size=(3,), stride=1, nempty=True, deconv=False):
        super().__init__()
        conv = OctreeConv(in_channels, out_channels, kernel_size, stride, nempty, deconv=deconv)
        self._name = "deconv" if deconv else "conv"
        setattr(self, self._name, conv)
        self.bn = nn.BatchNorm1d(out_channels, BN_EPS, BN_MOMENTUM)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, data, octree, depth):
        conv = getattr(self, self._name)
        if self._hip(data):
            scale, shift = ops.fold_batchnorm(self.bn)
            return conv(data, octree, depth, scale, shift, ops.ACT_RELU)
        return self.relu(self.bn(conv(data, octree, depth)))


class OctreeDWConv(nn.Module):
    """dwconv.OctreeDWConv restated: weights (27, 1, C), out[i] = sum_t weights[t] * x[neighbour t of i]"""

    def __init__(self, in_channels, kernel_size=(3,), nempty=True, use_bias=False):
        super().__init__()
        if not nempty or list(kernel_size) != [3] or use_bias:
            raise NotImplementedError("OctreeDWConv: kernel [3], nempty=True, no bias (the fork's use) is built")
        self.weights = nn.Parameter(torch.empty(27, 1, in_channels))
        nn.init.xavier_uniform_(self.weights)

    def forward(self, data, octree, depth):
        nbr = octree.neighbors(depth)
        out = torch.zeros_like(data)
        for t in range(27):
            out = out + _gather_rows(data, nbr[:, t]) * self.weights[t]
        return out


class OctreeDWConvBn(_Fusable):
    def __init__(self, in_channels, kernel_size=(3,), stride=1, nempty=False):
        super().__init__()
        self.conv = OctreeDWConv(in_channels, kernel_size, nempty, use_bias=False)
        self.bn = nn.BatchNorm1d(in_channels)

    def forward(self, data, octree, depth):
        return self.bn(self.conv(data, octree, depth))

    def forward_residual(self, data, octree, depth):
        """cpe(data) + data"""
        if self._hip(data) and data.shape[1] % 4 == 0:
            scale, shift = ops.fold_batchnorm(self.bn)
            return ops.octree_dwconv(data.contiguous(), self.conv.weights.detach(), octree.neighbors(depth), scale, shift)
        return self.forward(data, octree, depth) + data


class RPE(nn.Module):
    def __init__(self, patch_size, num_heads, dilation=1):
        super().__init__()
        self.patch_size, self.num_heads, self.dilation = patch_size, num_heads, dilation
        self.pos_bnd = self.get_pos_bnd(patch_size)
        self.rpe_num = 2 * self.pos_bnd + 1
        self.rpe_table = nn.Parameter(torch.zeros(3 * self.rpe_num, num_heads))
        nn.init.trunc_normal_(self.rpe_table, std=0.02)

    def get_pos_bnd(self, patch_size):
        return int(0.8 * patch_size * self.dilation ** 0.5)

    def extra_repr(self):
        return f"num_heads={self.num_heads}, pos_bnd={self.pos_bnd}, dilation={self.dilation}"


class OctreeAttention(_Fusable):
    def __init__(self, dim, patch_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0,
                 dilation=1, use_rpe=True):
        super().__init__()
        if not use_rpe or attn_drop:
            raise NotImplementedError("OctreeAttention: use_rpe=True and attn_drop=0 (the fork's use) are built")
        self.dim, self.patch_size, self.num_heads, self.dilation, self.use_rpe = dim, patch_size, num_heads, dilation, True
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.softmax = nn.Softmax(dim=-1)
        self.rpe = RPE(patch_size, num_heads, dilation)

    def attend(self, qkv, octree, depth, fused):
        # the fused eval path takes no gradient: a table that asks for one would send ops to the composition
        table = self.rpe.rpe_table.detach() if fused else self.rpe.rpe_table
        return ops.octree_attention(qkv, octree.xyz[depth], octree.batch[depth], table, self.num_heads,
                                    self.patch_size, self.dilation, self.rpe.pos_bnd, self.scale, self.qkv.bias, fused)

    def forward(self, data, octree, depth, res=None):
        if self._hip(data):
            qkv = ops.gemm(data, self.qkv.weight, bias=self.qkv.bias)
            return ops.gemm(self.attend(qkv, octree, depth, True), self.proj.weight, bias=self.proj.bias, res=res)
        data = self.proj_drop(self.proj(self.attend(self.qkv(data), octree, depth, False)))
        return data if res is None else res + data

    def extra_repr(self):
        return f"dim={self.dim}, patch_size={self.patch_size}, num_heads={self.num_heads}, dilation={self.dilation}"


class OctreeDropPath(nn.Module):
    """ocnn.nn.OctreeDropPath restated: one keep decision per scene, scaled by 1 / keep; identity in eval and at rate 0"""

    def __init__(self, drop_prob=0.0, nempty=True, scale_by_keep=True):
        super().__init__()
        self.drop_prob, self.nempty, self.scale_by_keep = drop_prob, nempty, scale_by_keep

    def forward(self, data, octree, depth):
        if self.drop_prob <= 0.0 or not self.training:
            return data
        keep = 1.0 - self.drop_prob
        mask = torch.floor(keep + torch.rand(octree.batch_size, 1, dtype=data.dtype, device=data.device))
        if keep > 0.0 and self.scale_by_keep:
            mask = mask / keep
        return data * mask[octree.batch[depth].long()]


class OctFormerBlock(_Fusable):
    def __init__(self, dim, num_heads, patch_size=32, dilation=0, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 attn_drop=0.0, proj_drop=0.0, drop_path=0.0, nempty=True, activation=nn.GELU, **kwargs):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim)
        self.attention = OctreeAttention(dim, patch_size, num_heads, qkv_bias, qk_scale, attn_drop, proj_drop, dilation)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = MLP(dim, int(dim * mlp_ratio), dim, activation, proj_drop)
        self.drop_path = OctreeDropPath(drop_path, nempty)
        self.cpe = OctreeDWConvBn(dim, nempty=nempty)

    def forward(self, data, octree, depth):
        data = self.cpe.forward_residual(data, octree, depth)
        if self._hip(data) and data.shape[1] % 4 == 0:
            h = ops.layernorm(data, self.norm1.weight, self.norm1.bias, self.norm1.eps)
            data = self.attention(h, octree, depth, res=data)
            h = ops.layernorm(data, self.norm2.weight, self.norm2.bias, self.norm2.eps)
            return self.mlp(h, res=data)
        data = data + self.drop_path(self.attention(self.norm1(data), octree, depth), octree, depth)
        return data + self.drop_path(self.mlp(self.norm2(data)), octree, depth)


class OctFormerStage(nn.Module):
    def __init__(self, dim, num_heads, patch_size=32, dilation=0, mlp_ratio=4.0, qkv_bias=True, qk_scale=None,
                 attn_drop=0.0, proj_drop=0.0, drop_path=0.0, nempty=True, activation=nn.GELU, interval=6,
                 use_checkpoint=True, num_blocks=2, octformer_block=OctFormerBlock, **kwargs):
        super().__init__()
        self.num_blocks, self.use_checkpoint, self.interval = num_blocks, use_checkpoint, interval
        self.num_norms = (num_blocks - 1) // interval
        self.blocks = nn.ModuleList([
            octformer_block(dim=dim, num_heads=num_heads, patch_size=patch_size,
                            dilation=1 if i % 2 == 0 else dilation, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias,
                            qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=proj_drop,
                            drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path, nempty=nempty,
                            activation=activation) for i in range(num_blocks)])

    def forward(self, data, octree, depth):
        for block in self.blocks:
            if self.use_checkpoint and self.training:
                data = checkpoint(block, data, octree, depth, use_reentrant=False)
            else:
                data = block(data, octree, depth)
        return data


def _linear(lin, x, fused):
    return ops.gemm(x.contiguous(), lin.weight, bias=lin.bias) if fused else lin(x)


def octree_upsample(data, octree, depth, target_depth=None):
    """ocnn.nn.OctreeUpsample("nearest", nempty=True): a node's row goes to its non-empty children, up to target_depth"""
    target_depth = depth + 1 if target_depth is None else target_depth
    for d in range(depth, target_depth):
        data = data[octree.parent[d + 1]]
    return data


class OctFormerDecoder(_Fusable):
    def __init__(self, channels, fpn_channel, nempty, head_up=1):
        super().__init__()
        self.head_up, self.num_stages = head_up, len(channels)
        self.conv1x1 = nn.ModuleList([nn.Linear(channels[i], fpn_channel) for i in range(self.num_stages - 1, -1, -1)])
        self.conv3x3 = nn.ModuleList([OctreeConvBnRelu(fpn_channel, fpn_channel, [3], 1, nempty)
                                      for _ in range(self.num_stages)])
        self.up_conv = nn.ModuleList([OctreeConvBnRelu(fpn_channel, fpn_channel, [3], 2, nempty, deconv=True)
                                      for _ in range(self.head_up)])

    def forward(self, features, octree):
        depth, depth_max = min(features.keys()), max(features.keys())
        assert self.num_stages == len(features)
        fused = self._hip(features[depth]) and all(f.shape[1] % 4 == 0 for f in features.values())
        feature = _linear(self.conv1x1[0], features[depth], fused)
        out = octree_upsample(self.conv3x3[0](feature, octree, depth), octree, depth, depth_max)
        for i in range(1, self.num_stages):
            depth_i = depth + i
            feature = _linear(self.conv1x1[i], features[depth_i], fused) + octree_upsample(feature, octree, depth_i - 1)
            out = out + octree_upsample(self.conv3x3[i](feature, octree, depth_i), octree, depth_i, depth_max)
        for i in range(self.head_up):
            out = self.up_conv[i](out, octree, depth_max + i)
        return out


class PatchEmbed(nn.Module):
    def __init__(self, in_channels=3, dim=96, num_down=2, nempty=True, **kwargs):
        super().__init__()
        self.num_stages, self.delta_depth = num_down, -num_down
        channels = [int(dim * 2 ** i) for i in range(-self.num_stages, 1)]
        self.convs = nn.ModuleList([OctreeConvBnRelu(in_channels if i == 0 else channels[i], channels[i], [3], 1, nempty)
                                    for i in range(self.num_stages)])
        self.downsamples = nn.ModuleList([OctreeConvBnRelu(channels[i], channels[i + 1], [2], 2, nempty)
                                          for i in range(self.num_stages)])
        self.proj = OctreeConvBnRelu(channels[-1], dim, [3], 1, nempty)

    def forward(self, data, octree, depth):
        for i in range(self.num_stages):
            data = self.convs[i](data, octree, depth - i)
            data = self.downsamples[i](data, octree, depth - i)
        return self.proj(data, octree, depth - self.num_stages)


class Downsample(_Fusable):
    def __init__(self, in_channels, out_channels, kernel_size=(2,), nempty=True):
        super().__init__()
        self.norm = nn.BatchNorm1d(out_channels)
        self.conv = OctreeConv(in_channels, out_channels, kernel_size, stride=2, nempty=nempty, use_bias=True)

    def forward(self, data, octree, depth):
        if self._hip(data):
            scale, shift = ops.fold_batchnorm(self.norm, self.conv.bias)
            return self.conv(data, octree, depth, scale, shift, ops.ACT_NONE)
        return self.norm(self.conv(data, octree, depth))


class OctFormerBackbone(nn.Module):
    """What OctFormer, KeypointOctFormer and OffsetKeypointOctFormer share: patch_embed, layers, downsamples, decoder and
    the nearest interpolation back to the points (octformer_v1m1_base.py:584-627)."""

    def _build_backbone(self, in_channels, fpn_channels, channels, num_blocks, num_heads, patch_size, stem_down, head_up,
                        dilation, drop_path, nempty, octree_scale_factor, octree_depth, octree_full_depth):
        self.patch_size, self.dilation, self.nempty = patch_size, dilation, nempty
        self.num_stages, self.stem_down, self.head_up = len(num_blocks), stem_down, head_up
        self.octree_scale_factor, self.octree_depth = octree_scale_factor, octree_depth
        self.octree_full_depth = octree_full_depth
        if head_up != stem_down:
            raise ValueError("OctFormer: head_up must equal stem_down for the decoder to end at the leaves")
        drop_ratio = torch.linspace(0, drop_path, sum(num_blocks)).tolist()
        self.patch_embed = PatchEmbed(in_channels, channels[0], stem_down, nempty)
        self.layers = nn.ModuleList([
            OctFormerStage(dim=channels[i], num_heads=num_heads[i], patch_size=patch_size,
                           drop_path=drop_ratio[sum(num_blocks[:i]):sum(num_blocks[:i + 1])], dilation=dilation,
                           nempty=nempty, num_blocks=num_blocks[i]) for i in range(self.num_stages)])
        self.downsamples = nn.ModuleList([Downsample(channels[i], channels[i + 1], kernel_size=[2], nempty=nempty)
                                          for i in range(self.num_stages - 1)])
        self.decoder = OctFormerDecoder(channels=channels, fpn_channel=fpn_channels, nempty=nempty, head_up=head_up)

    def set_fused(self, fused):
        """fused = False: eval runs the torch composition of the same plan (the reference's algorithm) instead of the
        kernels - what the fused path is tested and measured against."""
        for m in self.modules():
            if isinstance(m, _Fusable):
                m.fused = bool(fused)
        return self

    def points2octree(self, coord, feat, offset):
        min_depth = self.octree_depth - self.stem_down - self.num_stages + 1
        if min_depth < 2:
            raise ValueError(f"OctFormer: octree_depth {self.octree_depth} leaves the deepest stage at depth {min_depth}")
        return ops.octree_build(coord.float().contiguous(), feat.float().contiguous(), offset, self.octree_scale_factor,
                                self.octree_depth, min_depth)

    def backbone(self, data_dict, taps=None):
        """(n, fpn_channels) features of the input points; taps (a dict) collects the stages' outputs for the tests"""
        levels = data_dict.get("octree")
        if levels is None:
            levels = self.points2octree(data_dict["coord"], data_dict["feat"], data_dict["offset"])
        feat = self.patch_embed(levels.features, levels, levels.depth)
        depth = levels.depth - self.stem_down
        octree = OctreeT(levels, self.patch_size, self.dilation, self.nempty, max_depth=depth,
                         start_depth=depth - self.num_stages + 1)
        if taps is not None:
            taps["patch_embed"] = feat
        features = {}
        for i in range(self.num_stages):
            feat = self.layers[i](feat, octree, depth - i)
            features[depth - i] = feat
            if taps is not None:
                taps[f"stage{i}"] = feat
            if i < self.num_stages - 1:
                feat = self.downsamples[i](feat, octree, depth - i)
        out = self.decoder(features, octree)
        if taps is not None:
            taps["decoder"] = out
        out = out[levels.leaf]   # OctreeInterp("nearest"): every point has its leaf
        if taps is not None:
            taps["interp"] = out
        return out


@MODELS.register_module("OctFormer-v1m1")
class OctFormer(OctFormerBackbone):
    def __init__(self, in_channels, num_classes, fpn_channels=168, channels=(96, 192, 384, 384),
                 num_blocks=(2, 2, 18, 2), num_heads=(6, 12, 24, 24), patch_size=26, stem_down=2, head_up=2, dilation=4,
                 drop_path=0.5, nempty=True, octree_scale_factor=10.24, octree_depth=11, octree_full_depth=2):
        super().__init__()
        self._build_backbone(in_channels, fpn_channels, channels, num_blocks, num_heads, patch_size, stem_down, head_up,
                             dilation, drop_path, nempty, octree_scale_factor, octree_depth, octree_full_depth)
        self.seg_head = (nn.Sequential(nn.Linear(fpn_channels, fpn_channels), nn.BatchNorm1d(fpn_channels),
                                       nn.ReLU(inplace=True), nn.Linear(fpn_channels, num_classes))
                         if num_classes > 0 else nn.Identity())

    def forward(self, data_dict):
        return self.seg_head(self.backbone(data_dict))
