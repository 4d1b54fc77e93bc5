"""SpUNet-v1m1 (the plain sparse-CNN U-Net) on MI355X.

Counterpart of the reference's pointcept/models/sparse_unet/spconv_unet_v1m1_base.py:23-280: the same classes
(BasicBlock, SpUNetBase), constructor arguments, attribute names and therefore state_dict keys, shapes and order.  A 5^3
submanifold stem, `num_stages` encoder stages (a kernel-2 / stride-2 sparse conv, then `layers[s]` BasicBlocks) and as
many decoder stages (the inverse conv, the skip concatenation, `layers[-1 - s]` BasicBlocks of which the first narrows
cat(up, skip) through a 1x1 projection).  SpUNetNoSkipBase is not built.

Eval (fused = True): where `res_conv_wired` says so a BasicBlock is two launches - conv2 + bn2 + shortcut + ReLU is one
ptv3_res_conv, and the decoder front's conv1 + bn1 + ReLU and proj + bn is one ptv3_res_conv over (up, skip) that never
writes the concatenation (the 96-output shapes of the two finest levels); elsewhere ptv3_gemm with the folded
BatchNorm epilogue, torch.cat and ptv3_add_act.  The strided
convs run ptv3_down2_conv / ptv3_up2_conv with folded BatchNorm + ReLU.  One host read at entry (spatial shape and
offsets) and one per stage (the coarse row count).
Training, or set_fused(False): the torch composition over the taped HIP Functions (batch-statistic BatchNorm).  fp32.
"""
from collections import OrderedDict
from functools import partial

import torch
import torch.nn as nn

from ptv3_hip import ops
from ptv3_hip import autograd as A
from pointcept.models.builder import MODELS
from pointcept.models.utils.misc import offset2batch
from pointcept.models.utils.hip_layers import BatchNorm1d, ReLU
from pointcept.models.utils.sparse import (SparseConvTensor, SubMConv3d, SparseConv3d, SparseInverseConv3d,
                                           SparseSequential)
from pointcept.models.oacnns.oacnns_v1m1_base import check_extent
from pointcept.models.keypoint_ptv3_plus import PointwiseConv3d

MARGIN = 96      # sparse_shape = max(grid_coord) + 96 (:250)


def res_conv_wired(m, ca, cb, cout):
    """Whether a fused BasicBlock conv of this shape runs ptv3_res_conv (True) or ptv3_gemm + cat + add_act (False):
    the one place the decision is kept.  The rule is "only where the kernel measured faster".  tools/bench_spunet.py,
    MI355X, 8 x 20 000 sites, ms per call with the launches queued back to back, parent's ops / ptv3_res_conv
    (profiles/spunet/bench_spunet.jsonl):
        decoder front  96+32 -> 96    160 000 rows  1.445 / 1.103  (1.31x)    35 382 rows  0.386 / 0.342  (1.13x)
        block tail     96 -> 96       160 000 rows  1.089 / 0.731  (1.49x)    35 382 rows  0.293 / 0.248  (1.18x)
        block tail     32 -> 32        35 382 rows  0.0456 / 0.0418 (1.09x; 0.99x and 1.05x timed call by call: 4 us,
                                                                     not wired on that margin)
        128+64 -> 128, 256+128 -> 256, 64, 128, 256 plain (7 093 rows and fewer): 0.12x .. 0.59x, and ptv3_gemm
        splits K there (6 to 54 slabs), which this kernel does not do: stay.
    So the two 96-output shapes take the kernel, and never where ptv3_gemm would split K."""
    if (ca, cb, cout) not in WIRED or not ops.res_conv_capable(m, ca, cb, cout, 27):
        return False
    return ops.gemm_splits(m, ca + cb, cout, 27, torch.float32) <= 1


WIRED = frozenset({(96, 32, 96), (96, 0, 96)})      # (ca, cb, cout) that measured faster through ptv3_res_conv


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, in_channels, embed_channels, stride=1, norm_fn=None, indice_key=None, bias=False):
        super().__init__()
        assert norm_fn is not None
        if in_channels == embed_channels:
            self.proj = SparseSequential(nn.Identity())
        else:
            # the 1x1 conv as a linear layer on the rows (spconv's (out, 1, 1, 1, in) parameter, no neighbour table)
            self.proj = SparseSequential(PointwiseConv3d(in_channels, embed_channels, kernel_size=1, bias=False),
                                         norm_fn(embed_channels))
        self.conv1 = SubMConv3d(in_channels, embed_channels, kernel_size=3, stride=stride, padding=1, bias=bias,
                                indice_key=indice_key)
        self.bn1 = norm_fn(embed_channels)
        self.relu = ReLU()
        self.conv2 = SubMConv3d(embed_channels, embed_channels, kernel_size=3, stride=stride, padding=1, bias=bias,
                                indice_key=indice_key)
        self.bn2 = norm_fn(embed_channels)
        self.stride = stride
        self.fused = True
        self.res_conv = None     # None: res_conv_wired decides; True / False: the kernel wherever it is capable / nowhere

    def _wired(self, m, ca, cb, cout):
        if self.res_conv is None:
            return res_conv_wired(m, ca, cb, cout)
        return bool(self.res_conv) and ops.res_conv_capable(m, ca, cb, cout, 27)

    def _fusable(self):
        return (self.conv1.in_channels % 4 == 0 and self.conv1.out_channels % 4 == 0 and self.conv1.bias is None
                and self.conv2.bias is None)

    def _forward_fused(self, x, skip):
        """relu(bn2(conv2(relu(bn1(conv1(x))))) + proj(x)) with x = cat(x.features, skip), in two launches"""
        xa = x.features
        m, ca = xa.shape
        cb = 0 if skip is None else skip.shape[1]
        cout = self.conv1.out_channels
        nbr = x.neighbors(3, self.conv1.indice_key)
        order = x.row_order
        s1, t1 = self.bn1.folded()
        s2, t2 = self.bn2.folded()
        w1 = self.conv1._weight_for(torch.float32, ca + cb)
        w2 = self.conv2._weight_for(torch.float32, cout)
        projected = not isinstance(self.proj[0], nn.Identity)
        if projected:
            wp = self.proj[0]._weight_for(torch.float32, ca + cb)
            sp, tp = self.proj[1].folded()
            if self._wired(m, ca, cb, cout):
                h, p = ops.res_conv(xa, w1, nbr, xb=skip, bn_scale=s1, bn_shift=t1, act=ops.ACT_RELU, w_proj=wp,
                                    proj_scale=sp, proj_shift=tp, row_order=order)
            else:
                both = xa if skip is None else torch.cat((xa, skip), dim=1)
                h = ops.gemm(both, w1, nbr=nbr, kvol=27, row_order=order, bn_scale=s1, bn_shift=t1, act=ops.ACT_RELU)
                p = ops.gemm(both, wp, bn_scale=sp, bn_shift=tp)       # the 1x1 conv: a plain GEMM, no table
        else:
            assert skip is None
            h = ops.gemm(xa, w1, nbr=nbr, kvol=27, row_order=order, bn_scale=s1, bn_shift=t1, act=ops.ACT_RELU)
            p = xa
        if self._wired(m, cout, 0, cout):
            out = ops.res_conv(h, w2, nbr, bn_scale=s2, bn_shift=t2, res=p, act=ops.ACT_RELU, row_order=order)
        else:
            y = ops.gemm(h, w2, nbr=nbr, kvol=27, row_order=order, bn_scale=s2, bn_shift=t2)
            out = ops.add_act(y, p, ops.ACT_RELU)
        return x.replace_feature(out)

    def forward(self, x, skip=None):
        """x: SparseConvTensor.  skip (optional, (m, C_skip)): the block input is cat(x.features, skip) (:272)."""
        if self.fused and not self.training and self._fusable():
            return self._forward_fused(x, skip)
        if skip is not None:
            x = x.replace_feature(torch.cat((x.features, skip), dim=1))
        residual = x
        out = self.conv1(x)
        out = out.replace_feature(self.bn1(out.features, act=ops.ACT_RELU))
        out = self.conv2(out)
        out = out.replace_feature(self.bn2(out.features))
        out = out.replace_feature(out.features + self.proj(residual).features)
        return out.replace_feature(self.relu(out.features))


class _Final(SubMConv3d):
    """`final` (:221-227): SubMConv3d(kernel_size=1, bias=True), a plain GEMM without a neighbour table."""

    def forward(self, x):
        if self.training:
            w = self.weight.view(self.out_channels, self.in_channels)
            return x.replace_feature(A.linear(x.features, w, self.bias))
        feat = x.features
        pad = (-feat.shape[1]) % 4
        if pad:
            feat = torch.nn.functional.pad(feat, (0, pad)).contiguous()
        w = self._weight_for(torch.float32, feat.shape[1])
        return x.replace_feature(ops.gemm(feat, w, bias=self.bias.detach().float()))


class _Identity(nn.Identity):
    """spconv.pytorch.Identity"""


@MODELS.register_module("SpUNet-v1m1")
class SpUNetBase(nn.Module):
    def __init__(self, in_channels, num_classes, base_channels=32, channels=(32, 64, 128, 256, 256, 128, 96, 96),
                 layers=(2, 3, 4, 6, 2, 2, 2, 2), enc_mode=False):
        super().__init__()
        assert len(layers) % 2 == 0
        assert len(layers) == len(channels)
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.base_channels = base_channels
        self.channels = channels
        self.layers = layers
        self.num_stages = len(layers) // 2
        self.enc_mode = enc_mode

        norm_fn = partial(BatchNorm1d, eps=1e-3, momentum=0.01)
        block = BasicBlock

        self.conv_input = SparseSequential(
            SubMConv3d(in_channels, base_channels, kernel_size=5, padding=1, bias=False, indice_key="stem"),
            norm_fn(base_channels),
            ReLU(),
        )
        enc_channels = base_channels
        dec_channels = channels[-1]
        self.down = nn.ModuleList()
        self.up = nn.ModuleList()
        self.enc = nn.ModuleList()
        self.dec = nn.ModuleList() if not self.enc_mode else None
        for s in range(self.num_stages):
            self.down.append(SparseSequential(
                SparseConv3d(enc_channels, channels[s], kernel_size=2, stride=2, bias=False, indice_key=f"spconv{s + 1}"),
                norm_fn(channels[s]),
                ReLU(),
            ))
            self.enc.append(SparseSequential(OrderedDict(
                (f"block{i}", block(channels[s], channels[s], norm_fn=norm_fn, indice_key=f"subm{s + 1}"))
                for i in range(layers[s]))))
            if not self.enc_mode:
                self.up.append(SparseSequential(
                    SparseInverseConv3d(channels[len(channels) - s - 2], dec_channels, kernel_size=2, bias=False,
                                        indice_key=f"spconv{s + 1}"),
                    norm_fn(dec_channels),
                    ReLU(),
                ))
                self.dec.append(SparseSequential(OrderedDict(
                    (f"block{i}", block(dec_channels + enc_channels if i == 0 else dec_channels, dec_channels,
                                        norm_fn=norm_fn, indice_key=f"subm{s}"))
                    for i in range(layers[len(channels) - s - 1]))))
            enc_channels = channels[s]
            dec_channels = channels[len(channels) - s - 2]
        final_in_channels = channels[-1] if not self.enc_mode else channels[self.num_stages - 1]
        self.final = (_Final(final_in_channels, num_classes, kernel_size=1, padding=1, bias=True)
                      if num_classes > 0 else _Identity())
        self.apply(self._init_weights)

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

    def set_fused(self, fused):
        """fused = False: eval runs the training path's torch composition (running-statistic BatchNorm) instead of the
        fused kernels - what the fused path is tested against."""
        for m in self.modules():
            if hasattr(m, "fused"):
                m.fused = bool(fused)
        return self

    def set_res_conv(self, mode):
        """None: res_conv_wired decides per shape (the default); True: ptv3_res_conv wherever it is capable; False:
        ptv3_gemm + cat + add_act everywhere.  Fused eval only."""
        for m in self.modules():
            if isinstance(m, BasicBlock):
                m.res_conv = mode
        return self

    def backbone(self, input_dict, taps=None):
        """-> (SparseConvTensor of the last stage, scene ends as a device tensor for that tensor's rows).  One host
        read here (spatial shape and offsets) and one per stage (the coarse row count)."""
        grid = input_dict["grid_coord"]
        offset = input_dict["offset"]
        head = torch.cat([grid.max(dim=0).values.long(), offset.long()]).tolist()     # the forward's entry read
        shape, ends = [v + MARGIN for v in head[:3]], head[3:]
        check_extent(type(self).__name__, shape, self.num_stages)
        batch = offset2batch(offset.long(), ends[-1])
        x = SparseConvTensor(features=input_dict["feat"].float().contiguous(),
                             indices=torch.cat([batch.unsqueeze(-1), grid], dim=1).int().contiguous(),
                             spatial_shape=shape, batch_size=len(ends))
        x = self.conv_input(x)
        skips = [x]
        if taps is not None:
            taps.append(x)
        for s in range(self.num_stages):
            x = self.down[s](x)
            for blk in self.enc[s]:
                x = blk(x)
            skips.append(x)
            if taps is not None:
                taps.append(x)
        x = skips.pop(-1)
        if self.enc_mode:
            # coarse rows are sorted by (b, x, y, z): scene k ends where the first row of a later scene stands
            scenes = torch.arange(1, len(ends) + 1, device=x.indices.device, dtype=torch.int32)
            return x, torch.searchsorted(x.indices[:, 0].contiguous(), scenes).long()
        for s in reversed(range(self.num_stages)):
            x = self.up[s](x)
            skip = skips.pop(-1).features
            for i, blk in enumerate(self.dec[s]):
                x = blk(x, skip) if i == 0 else blk(x)
            if taps is not None:
                taps.append(x)
        return x, offset

    def forward(self, input_dict):
        x, ends = self.backbone(input_dict)
        x = self.final(x) if isinstance(self.final, _Final) else x
        if self.enc_mode:
            feat = x.features.contiguous()
            return A.scene_mean(feat, ends) if self.training else ops.scene_mean(feat, ends)
        return x.features
