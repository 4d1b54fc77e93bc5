"""PT-v3m1-Plus and KeypointPTv3Plus on MI355X.

Counterpart of the reference's pointcept/models/keypoint_ptv3_plus.py: same class names (BlockPlus :27,
PointTransformerV3Plus :156 under the registry name "PT-v3m1-Plus", KeypointPTv3Plus :473), same constructor keywords
and defaults, same module tree (`enc_stages.{s}.{down,block{i}}`, `dec.dec{s}.{up,block{i}}`, the nine `cpe` modules)
and so the same state_dict.  Against PT-v3m1 the backbone changes three things:

  * BlockPlus.cpe is a bottleneck (:68-94): 1x1 conv C -> mid, LayerNorm, ReLU, k^3 conv mid -> mid (k = 5 in the fork
    config), LayerNorm, ReLU, 1x1 conv mid -> C, Linear, LayerNorm; mid = C // 4, or C when that is below 16.
    Eval, fused: ptv3_rows_linear_ln, the k^3 conv (ptv3_subm_conv_ln where use_fused_cpe says it wins, else ptv3_gemm
    + ptv3_layernorm + ReLU), one GEMM with the folded expand matrix W_lin W_up, then Block's own dispatch from the
    CPE's last LayerNorm on (Block._eval_after_cpe; BlockPlus is a subclass of Block).  set_fused(False) and training
    run the reference's statement order on the unfused layer ops; a kernel size the fused conv kernel does not serve
    takes the composed conv.
  * every block attends along order 0 (:283, :334);
  * the encoder re-serializes after pooling at the stages with s % 3 != 0 (:389-454): the coordinate columns are
    permuted, one "z" order is computed, and the level is physically sorted by it.  All of it runs on the device.

Reproduced as the reference computes it, including what looks accidental: after a reorder a
level carries ONE order and later levels inherit it through pooling; the column permutations accumulate; the sparse
tensor's spatial_shape is not permuted (the site hash here never reads it); and `pooling_inverse` of a reordered level
is NOT re-indexed, so the decoder's `point.feat[inverse]` reads the reordered rows through the stale map.
"""
from functools import partial

import torch
import torch.nn as nn

from ptv3_hip import ops
from ptv3_hip import autograd as A
from pointcept.models.builder import MODELS
from pointcept.models.utils.structure import Point
from pointcept.models.utils.sparse import SubMConv3d, SparseConvTensor
from pointcept.models.utils.hip_layers import Linear, LayerNorm, BatchNorm1d, GELU, ReLU, check_sync_batchnorm
from pointcept.models.modules import PointModule, PointSequential
from pointcept.models.point_transformer_v3.point_transformer_v3m1_base import (
    Block, SerializedAttention, MLP, SerializedPooling, SerializedUnpooling, Embedding, PointTransformerV3, RPE, _add,
    _input_feat)  # noqa: F401
from pointcept.models.keypoint_ptv3 import KeypointPTv3


def cpe_mid_channels(channels):
    """bottleneck width of BlockPlus.cpe (:63-66)"""
    mid = channels // 4
    return channels if mid < 16 else mid


def fold_expand(w_up, w_lin):
    """cpe[6] (1x1 conv, no bias) followed by cpe[7] (Linear) is one linear map: W = W_lin @ W_up, (C, mid)."""
    return w_lin @ w_up.reshape(w_up.shape[0], w_up.shape[-1])


# The wiring rule of the fused CPE kernels (timings: profiles/ptv3_plus/bench_cpe_plus.jsonl, table in DESIGN.md
# section 16; every level of the fork config on 8 x 20 000 and 1 x 100 000 sites, both dtypes).
# ptv3_rows_linear_ln beat its composition at every measured shape but 512 -> 128 (0.5x in fp32, 0.9x in bf16).
FUSED_FRONT_OFF = frozenset({(512, 128)})                 # (c_in, mid), either dtype
# ptv3_subm_conv_ln lost to ptv3_gemm -> ptv3_layernorm -> ReLU at every width measured at 125 taps (0.03x to 0.9x; 1.03x
# to 1.06x at c = 16, fp32, 100 000 rows and more, which is inside the spread), and 27 taps were not timed: no shape
# takes it yet.  (mid, kvol, dtype) goes here once the kernel wins there.
FUSED_CONV_ON = frozenset()


def use_fused_cpe(c_in, mid, kvol, dtype):
    """(front, conv): whether cpe[0..2] / cpe[3..5] run as ptv3_rows_linear_ln / ptv3_subm_conv_ln.  A shape takes the
    fused kernel when the kernel serves it and the measurement above does not show it slower than its composition."""
    front = ops.rows_linear_ln_capable(c_in, mid, dtype) and (c_in, mid) not in FUSED_FRONT_OFF
    conv = ops.subm_conv_ln_capable(mid, kvol, dtype) and (mid, kvol, dtype) in FUSED_CONV_ON
    return front, conv


class PointwiseConv3d(SubMConv3d):
    """SubMConv3d(in, out, kernel_size=1): one tap, the site itself - a linear layer on the feature rows under the
    parameter layout (out, 1, 1, 1, in) of spconv; no neighbour table is built for it."""

    def forward(self, x, **epilogue):
        if self.training:
            if epilogue:
                raise NotImplementedError("training-mode PointwiseConv3d: epilogues are eval-only fusions")
            return x.replace_feature(A.linear(x.features, self.weight.view(self.out_channels, self.in_channels),
                                              self.bias))
        w = self._weight_for(x.features.dtype, self.in_channels)
        bias = None if self.bias is None else self.bias.detach().float()
        return x.replace_feature(ops.gemm(x.features, w, bias=bias, **epilogue))


class BlockPlus(Block):
    """Block with the bottleneck CPE (:27-153).  Training and set_fused(False) run Block's generic statement order (the
    reference's :125-153) through the nine CPE modules; the native executor does not know this class."""

    def __init__(self, *args, cpe_kernel_size=3, **kwargs):   # Block's signature, then cpe_kernel_size (:28-48)
        super().__init__(*args, cpe_kernel_size=cpe_kernel_size, **kwargs)
        self.cpe_kernel_size = cpe_kernel_size
        self.fused = True

    @staticmethod
    def _build_cpe(channels, norm_layer, indice_key, cpe_kernel_size):
        mid = cpe_mid_channels(channels)
        return PointSequential(
            PointwiseConv3d(channels, mid, kernel_size=1, bias=False),
            norm_layer(mid),
            ReLU(inplace=True),
            SubMConv3d(mid, mid, kernel_size=cpe_kernel_size, padding=cpe_kernel_size // 2, bias=True,
                       indice_key=indice_key),
            norm_layer(mid),
            ReLU(inplace=True),
            PointwiseConv3d(mid, channels, kernel_size=1, bias=False),
            Linear(channels, channels),
            norm_layer(channels),
        )

    def _fusable(self):
        c = self.cpe
        return (self.pre_norm and all(isinstance(c[i], LayerNorm) for i in (1, 4, 8))
                and isinstance(self.norm1[0], LayerNorm) and isinstance(self.norm2[0], LayerNorm)
                and c[0].bias is None and c[6].bias is None and c[7].bias is not None)

    def expand_weight(self, dtype):
        """folded cpe[6] + cpe[7] in `dtype` (product taken in fp32), once per parameter version"""
        up, lin = self.cpe[6], self.cpe[7]
        return self._param_cache().get(
            ("expand", dtype), [up.weight, lin.weight],
            lambda: fold_expand(up.weight.detach().float(), lin.weight.detach().float()).to(dtype).contiguous())

    def cpe_rows(self, spt):
        """cpe[0..7] in eval: the (N, C) rows in front of the last LayerNorm.  Reads the sparse tensor's features, as the
        reference's first conv does."""
        c = self.cpe
        x = spt.features
        dt = x.dtype
        conv = c[3]
        kvol = conv.kernel_size ** 3
        nbr = spt.neighbors(conv.kernel_size, conv.indice_key)
        front, fused_conv = use_fused_cpe(x.shape[1], conv.in_channels, kvol, dt)
        g1, b1 = c[1].affine_f32()
        w_down = c[0]._weight_for(dt, c[0].in_channels)
        if front:
            h = ops.rows_linear_ln(x, w_down, None, g1, b1, c[1].eps, ops.ACT_RELU)
        else:
            h = ops.affine_act(ops.layernorm(ops.gemm(x, w_down), g1, b1, c[1].eps), None, None, ops.ACT_RELU)
        g4, b4 = c[4].affine_f32()
        w_conv = conv._weight_for(dt, conv.in_channels)
        bias = conv.bias.detach().float()
        if fused_conv:
            h = ops.subm_conv_ln(h, w_conv, nbr, bias, g4, b4, c[4].eps, ops.ACT_RELU, row_order=spt.row_order)
        else:
            h = ops.gemm(h, w_conv, bias=bias, nbr=nbr, kvol=kvol, row_order=spt.row_order)
            h = ops.affine_act(ops.layernorm(h, g4, b4, c[4].eps), None, None, ops.ACT_RELU)
        return ops.gemm(h, self.expand_weight(dt), bias=c[7].bias_f32())

    def forward(self, point: Point):
        if self.training or not self.fused or not self._fusable():
            return self._forward_generic(point)
        return self._eval_after_cpe(point, x=self.cpe_rows(point.sparse_conv_feat))


AXIS_PERMUTATIONS = {1: [1, 2, 0], 2: [2, 0, 1]}   # s % 3 -> YZX, ZXY (:391-396); 0: no reorder


def reserialize(point: Point, permutation):
    """Multi-view re-serialization of one encoder level (:399-454), on the device: permute the coordinate columns,
    compute one "z" order, sort the level physically by it, rebuild the sparse tensor on the sorted sites and reset
    order / inverse to the identity.  Returns the order applied ((n) int64, the argsort's own tensor).

    Scenes stay contiguous and `offset` stays valid: the z code carries the batch index above the 3 * depth position
    bits (ptv3_sfc_encode, as the reference's encode()), so sorting by it never moves a row across a scene boundary and
    keeps the scenes in their order.  No host read: the depth comes from the per-axis maxima the Point already holds
    (their maximum does not change under a column permutation)."""
    idx = torch.tensor(permutation, device=point.grid_coord.device)
    if "coord" in point.keys():
        point.coord = point.coord.index_select(1, idx)
    point.grid_coord = point.grid_coord.index_select(1, idx)
    if "_grid_max_host" in point.keys():
        point["_grid_max_host"] = [point["_grid_max_host"][p] for p in permutation]
    point.serialization(order="z")
    order = point.serialized_order[0]
    point.feat = point.feat.index_select(0, order)
    for key in ("coord", "grid_coord", "batch", "condition", "context"):
        if key in point.keys() and torch.is_tensor(point[key]):
            point[key] = point[key].index_select(0, order)
    sp = point.sparse_conv_feat
    indices = torch.cat([point.batch.unsqueeze(-1).int(), point.grid_coord.int()], dim=1).contiguous()
    # a fresh tensor: its site hash and neighbour tables are built once on the sorted sites and shared by the encoder
    # and decoder blocks of this level; rows are already in z order, so no visiting order is attached
    point.sparse_conv_feat = SparseConvTensor(point.feat, indices, sp.spatial_shape, sp.batch_size)
    n = order.shape[0]
    ident = torch.arange(n, device=order.device, dtype=point.serialized_order.dtype).unsqueeze(0)
    point.serialized_code = point.serialized_code.index_select(1, order)
    point.serialized_order = ident
    point.serialized_inverse = ident.clone()
    return order


@MODELS.register_module("PT-v3m1-Plus")
class PointTransformerV3Plus(PointModule):
    def __init__(
        self,
        in_channels=6,
        order=("z", "z-trans"),
        stride=(2, 2, 2, 2),
        enc_depths=(2, 2, 2, 6, 2),
        enc_channels=(32, 64, 128, 256, 512),
        enc_num_head=(2, 4, 8, 16, 32),
        enc_patch_size=(48, 48, 48, 48, 48),
        dec_depths=(2, 2, 2, 2),
        dec_channels=(64, 64, 128, 256),
        dec_num_head=(4, 4, 8, 16),
        dec_patch_size=(48, 48, 48, 48),
        mlp_ratio=4,
        qkv_bias=True,
        qk_scale=None,
        attn_drop=0.0,
        proj_drop=0.0,
        drop_path=0.3,
        pre_norm=True,
        shuffle_orders=True,
        enable_rpe=False,
        enable_flash=True,
        upcast_attention=False,
        upcast_softmax=False,
        enc_mode=False,
        pdnorm_bn=False,
        pdnorm_ln=False,
        pdnorm_decouple=True,
        pdnorm_adaptive=False,
        pdnorm_affine=True,
        pdnorm_conditions=("ScanNet", "S3DIS", "Structured3D"),
        cpe_kernel_size=5,
    ):
        super().__init__()
        self.num_stages = len(enc_depths)
        self.order = [order] if isinstance(order, str) else order
        self.enc_mode = enc_mode
        self.shuffle_orders = shuffle_orders
        self.cpe_kernel_size = cpe_kernel_size
        # None: follow torch autocast (bf16) else fp32; or force torch.float32 / torch.bfloat16 (as PT-v3m1)
        self.compute_dtype = None

        assert self.num_stages == len(stride) + 1
        assert self.num_stages == len(enc_depths)
        assert self.num_stages == len(enc_channels)
        assert self.num_stages == len(enc_num_head)
        assert self.num_stages == len(enc_patch_size)

        if pdnorm_bn or pdnorm_ln:
            raise NotImplementedError("PDNorm (pdnorm_bn / pdnorm_ln) is off in every target config and is not "
                                      "part of the MI355X path (SURVEY.md section 2a row 10)")
        bn_layer = partial(BatchNorm1d, eps=1e-3, momentum=0.01)
        ln_layer = LayerNorm
        act_layer = GELU

        self.embedding = Embedding(in_channels=in_channels, embed_channels=enc_channels[0], norm_layer=bn_layer,
                                   act_layer=act_layer)

        block = partial(BlockPlus, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop,
                        proj_drop=proj_drop, norm_layer=ln_layer, act_layer=act_layer, pre_norm=pre_norm,
                        order_index=0, enable_rpe=enable_rpe, enable_flash=enable_flash,
                        upcast_attention=upcast_attention, upcast_softmax=upcast_softmax,
                        cpe_kernel_size=cpe_kernel_size)

        self.enc_stages = nn.ModuleList()
        enc_drop_path = [x.item() for x in torch.linspace(0, drop_path, sum(enc_depths))]
        for s in range(self.num_stages):
            stage = PointSequential()
            if s > 0:
                stage.add(SerializedPooling(in_channels=enc_channels[s - 1], out_channels=enc_channels[s],
                                            stride=stride[s - 1], norm_layer=bn_layer, act_layer=act_layer),
                          name="down")
            enc_drop_path_ = enc_drop_path[sum(enc_depths[:s]): sum(enc_depths[: s + 1])]
            for i in range(enc_depths[s]):
                stage.add(block(channels=enc_channels[s], num_heads=enc_num_head[s], patch_size=enc_patch_size[s],
                                drop_path=enc_drop_path_[i], cpe_indice_key=f"stage{s}"), name=f"block{i}")
            self.enc_stages.append(stage)

        if not self.enc_mode:
            dec_drop_path = [x.item() for x in torch.linspace(0, drop_path, sum(dec_depths))]
            self.dec = PointSequential()
            dec_channels = list(dec_channels) + [enc_channels[-1]]
            for s in reversed(range(self.num_stages - 1)):
                dec_drop_path_ = dec_drop_path[sum(dec_depths[:s]): sum(dec_depths[: s + 1])]
                dec_drop_path_.reverse()
                dec = PointSequential()
                dec.add(SerializedUnpooling(in_channels=dec_channels[s + 1], skip_channels=enc_channels[s],
                                            out_channels=dec_channels[s], norm_layer=bn_layer, act_layer=act_layer),
                        name="up")
                for i in range(dec_depths[s]):
                    dec.add(block(channels=dec_channels[s], num_heads=dec_num_head[s], patch_size=dec_patch_size[s],
                                  drop_path=dec_drop_path_[i], cpe_indice_key=f"stage{s}"), name=f"block{i}")
                self.dec.add(module=dec, name=f"dec{s}")

    resolve_dtype = PointTransformerV3.resolve_dtype

    def set_fused(self, fused):
        """True (default): the fused CPE kernels in eval.  False: the reference's statement order on the unfused ops."""
        for m in self.modules():
            if isinstance(m, BlockPlus):
                m.fused = bool(fused)
        return self

    def forward(self, data_dict):
        check_sync_batchnorm(self)
        with torch.set_grad_enabled(self.training and torch.is_grad_enabled()):
            point = Point(data_dict)
            point.feat = _input_feat(point.feat, self.resolve_dtype())
            point.serialization(order=self.order, shuffle_orders=self.shuffle_orders)
            point.sparsify()
            point = self.embedding(point)
            for s, stage in enumerate(self.enc_stages):
                if s == 0:      # stage 0 is never reordered: the output rows align with the input
                    point = stage(point)
                    continue
                blocks = []
                for name, module in stage.named_children():
                    if name == "down":
                        point = module(point)   # the unplanned path: a planned geometry cannot span a reorder
                    else:
                        blocks.append(module)
                permutation = AXIS_PERMUTATIONS.get(s % 3)
                if permutation is not None:
                    reserialize(point, permutation)
                for block in blocks:
                    point = block(point)
            if not self.enc_mode:
                point = self.dec(point)
        return point


@MODELS.register_module()
class KeypointPTv3Plus(KeypointPTv3):
    """keypoint_ptv3_plus.py:473-547: KeypointPTv3 on the "PT-v3m1-Plus" backbone (same head, same result dict)."""

    def __init__(self, backbone_conf, num_keypoints=6, hidden_dim=256):
        super().__init__(backbone_conf, num_keypoints, hidden_dim)

    def set_fused(self, fused):
        self.backbone.set_fused(fused)
        return self
