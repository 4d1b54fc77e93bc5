"""SpUNet-v1m3 (the sparse-CNN U-Net with prompt-driven normalisation, the backbone of Point Prompt Training) on MI355X.

Counterpart of the reference's pointcept/models/sparse_unet/spconv_unet_v1m3_pdnorm.py:25-429: the same classes
(PDBatchNorm :25-74, BasicBlock :77-146, SPConvDown :149-176, SPConvUp :179-205, SPConvPatchEmbedding :208-227, SpUNetBase
:230-429), constructor keywords, defaults and attribute names, therefore the same state_dict keys, shapes, dtypes and
order.  The convolutions, the strided pair, the residual-block kernel and its wiring rule, `final` and the per-scene mean
are SpUNet-v1m1's (spconv_unet_v1m1_base.py here); what is new is the normalisation.

PDBatchNorm (:63-74) is one BatchNorm per dataset condition and, with adaptive=True, `bn(x) * (1 + scale) + shift` with
(shift, scale) = Linear(SiLU(context)).chunk(2).  Since BN_affine(x) (1 + scale) + shift = xhat gamma (1 + scale) +
beta (1 + scale) + shift, a PDBatchNorm is a plain BatchNorm with the affine pair
    gamma_eff = gamma (1 + scale),   beta_eff = beta (1 + scale) + shift
and the context is one row, the same for every layer: all pairs are known before the first convolution runs.  The
one-launch modulation path computes them for all layers at the top of the forward (csrc/pdnorm.hip):
  training, or set_fused(False): one taped call (ptv3_hip.autograd.PDNormModulationFn), then every PDBatchNorm is the
    existing BatchNormActFn with its slice as weight / bias, the active BatchNorm's running buffers and sync_group, ReLU
    fused;
  eval, fused: one fold launch gives the (scale, shift) pairs of the conv epilogues, cached per condition on the storages
    and versions of what they depend on; the blocks then run exactly as SpUNet-v1m1's fused blocks do.
With the path off (set_modulation(False)) every layer composes its own pair from ops that predate the kernel (SiLU, the
M = 1 GEMM of the library's Linear, the element-wise products).  Which of the two runs by default is MODULATION_WIRED
below, decided by measurement per use.

Differences from the reference, on purpose:
  * `input_dict["condition"]` may be a string or a list whose first entry counts (as PDNorm.active here).  The reference
    takes condition[0] unconditionally (:395), which after its DefaultSegmentor has unwrapped the list is the first
    CHARACTER of the name; with a list the two agree.
  * zero_init=True with norm_adaptive=False is an AttributeError at construction there (:386-389, no `modulation`); a
    ValueError here.
  * a context of more than one row is refused (PPT passes (1, context_channels); more rows would not broadcast against
    the features there either unless their count matched).
fp32 like SpUNet-v1m1; under autocast the features are upcast.
"""
from collections import OrderedDict
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from ptv3_hip import ops
from ptv3_hip import autograd as A
from pointcept.models.builder import MODELS
from pointcept.models.utils.misc import offset2batch
from pointcept.models.utils.hip_layers import BatchNorm1d, Linear, ReLU, check_sync_batchnorm
from pointcept.models.utils.sparse import (SparseConvTensor, SubMConv3d, SparseConv3d, SparseInverseConv3d,
                                           SparseSequential, _ParamCache)
from pointcept.models.oacnns.oacnns_v1m1_base import check_extent
from pointcept.models.keypoint_ptv3_plus import PointwiseConv3d
from pointcept.models.sparse_unet.spconv_unet_v1m1_base import MARGIN, res_conv_wired, _Final, _Identity

# Whether the one-launch modulation path is the default, per use.  The rule is the project's: on only where it measured
# ahead of the per-layer composition by more than the spread between the two recorded runs (tools/bench_spunet_pdnorm.py,
# profiles/spunet_pdnorm/).  MI355X, fp32, one launch / per layer, ms, run 1 | run 2:
#   calls alone, 59 layers, Cc = 256: taped forward 0.265 | 0.266 / 3.28 | 3.72, backward 1.17 | 0.96 / 6.36 | 6.61,
#     eval fold 0.228 | 0.219 / 4.39 | 4.41 (33 layers, Cc = 24: 6.0x and up)
#   PPT_SPUNET_SCANNET_CFG at 8 x 20 000 sites: training step 50.08 | 50.87 / 56.40 | 56.23 (1.12x, spread 1.6 %);
#     first eval forward 9.31 | 9.21 / 13.01 | 12.36 (1.37x, spread 5 %); steady eval forward 9.06 | 8.98 / 9.01 | 8.97
# All three comparisons are ahead by more than the spread: both uses are on.
MODULATION_WIRED = {"train": True, "eval": True}


def parse_condition(condition):
    """a string, or a list / tuple whose first entry counts"""
    return condition if isinstance(condition, str) else condition[0]


def condition_key(condition):
    """the condition as part of a cache key.  Always part of it, also with decouple=False: under PPT the context is a
    different row of embedding_table.weight per condition while the table, the `source`, is the same tensor."""
    return None if condition is None else parse_condition(condition)


class Prompt:
    """what one forward hands to every PDBatchNorm: the condition, the context row, what the context was computed from
    (`source`: with the condition, the cache key of the folds; the cache entries keep a reference to it, so that its
    address cannot be handed to another tensor while they live) and, on the one-launch path, every layer's pair"""
    __slots__ = ("condition", "context", "source", "pairs", "folded")

    def __init__(self, condition, context, source=None):
        self.condition, self.context, self.source = condition, context, source if source is not None else context
        self.pairs = None      # [(gamma_eff, beta_eff)] by slot: training / composition
        self.folded = None     # [(scale, shift)] by slot: fused eval


class PDBatchNorm(nn.Module):
    def __init__(self, num_features, context_channels=256, eps=1e-3, momentum=0.01,
                 conditions=("ScanNet", "S3DIS", "Structured3D"), decouple=True, adaptive=False, affine=True):
        super().__init__()
        self.conditions = conditions
        self.decouple = decouple
        self.adaptive = adaptive
        self.affine = affine
        self.num_features = num_features
        if self.decouple:
            self.bns = nn.ModuleList([BatchNorm1d(num_features=num_features, eps=eps, momentum=momentum, affine=affine)
                                      for _ in conditions])
        else:
            self.bn = BatchNorm1d(num_features=num_features, eps=eps, momentum=momentum, affine=affine)
        if self.adaptive:
            self.modulation = nn.Sequential(nn.SiLU(), Linear(context_channels, 2 * num_features, bias=True))
        self.slot = None           # position among the model's PDBatchNorms (SpUNetBase sets it)
        self._cache = _ParamCache()
        self._unit = {}

    def active(self, condition):
        """the BatchNorm of the condition (looked up on every call: adopt_sync_batchnorm swaps the slots)"""
        if not self.decouple:
            return self.bn
        condition = parse_condition(condition) if condition is not None else None
        if condition not in self.conditions:
            raise KeyError(f"PDBatchNorm: condition {condition!r} is not one of {tuple(self.conditions)}")
        return self.bns[list(self.conditions).index(condition)]

    def tensors(self, index):
        """(W, b, gamma, beta, running_mean, running_var) of condition `index`, None where there is none.  Read straight
        from the module dictionaries, not through nn.Module's attribute lookup: the model asks every layer on every
        forward, and the steady eval forward of the ScanNet config measured 9.27 ms with attribute lookups (and 60
        capability queries) against 9.06 ms with these (tools/bench_spunet_pdnorm.py, 8 x 20 000 sites)."""
        mods = self._modules
        bn = mods["bns"]._modules[str(index)] if self.decouple else mods["bn"]
        lin = mods["modulation"]._modules["1"]._parameters
        p, b = bn._parameters, bn._buffers
        return lin["weight"], lin["bias"], p["weight"], p["bias"], b["running_mean"], b["running_var"]

    def _units(self, ref):
        key = (ref.device, ref.dtype)
        if key not in self._unit:
            self._unit[key] = (torch.ones(self.num_features, device=ref.device, dtype=torch.float32),
                               torch.zeros(self.num_features, device=ref.device, dtype=torch.float32))
        return self._unit[key]

    def _context(self, context):
        if context is None:
            raise ValueError("PDBatchNorm(adaptive=True) needs `context` (input_dict['context'], (1, context_channels))")
        if context.dim() != 2 or context.shape[0] != 1:
            raise ValueError(f"PDBatchNorm: `context` must be one row (1, context_channels), got {tuple(context.shape)}")
        return context.float()

    def pair(self, bn, context):
        """per-layer composition of (gamma_eff, beta_eff) from SiLU, the library's Linear and element-wise products"""
        shift, scale = self.modulation[1](F.silu(self._context(context))).chunk(2, dim=1)
        one_plus = 1.0 + scale
        if bn.weight is not None:
            return (bn.weight * one_plus).view(-1), (bn.bias * one_plus + shift).view(-1)
        return one_plus.reshape(-1), shift.reshape(-1)

    def folded(self, prompt):
        """eval: the (scale, shift) pair of the conv epilogues"""
        if prompt.folded is not None:
            return prompt.folded[self.slot]
        bn = self.active(prompt.condition)
        if not self.adaptive and bn.weight is not None:
            return bn.folded()
        deps = [bn.running_mean, bn.running_var] + [p for p in (bn.weight, bn.bias) if p is not None]
        if self.adaptive:
            deps += [self.modulation[1].weight, self.modulation[1].bias, prompt.source]

        def make():
            w, b = self.pair(bn, prompt.context) if self.adaptive else self._units(bn.running_mean)
            scale = w.float() * torch.rsqrt(bn.running_var.float() + bn.eps)
            return scale.contiguous(), (b.float() - bn.running_mean.float() * scale).contiguous(), prompt.source
        return self._cache.get(("fold", condition_key(prompt.condition)), deps, make)[:2]

    def forward(self, feat, condition=None, context=None, act=ops.ACT_NONE, prompt=None):
        """feat (n, C).  The reference's signature (feat, condition, context); `prompt` carries the same two and the
        pairs of the one-launch path, `act` is fused into the BatchNorm's kernels."""
        if prompt is None:
            prompt = Prompt(condition, context)
        bn = self.active(prompt.condition)
        if not self.adaptive and bn.weight is not None:
            return bn(feat, act=act)              # exactly the active BatchNorm1d
        if self.adaptive:
            w, b = prompt.pairs[self.slot] if prompt.pairs is not None else self.pair(bn, prompt.context)
        else:
            w, b = self._units(feat)
        if bn.training and bn.track_running_stats and bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        return A.batch_norm_act(feat.float(), bn, act, weight=w.contiguous(), bias=b.contiguous())


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, in_channels, embed_channels, stride=1, norm_fn=None, indice_key=None, bias=False):
        super().__init__()
        assert norm_fn is not None
        self.in_channels = in_channels
        self.embed_channels = embed_channels
        if in_channels == embed_channels:
            self.proj = SparseSequential(nn.Identity())
        else:
            # the 1x1 conv as a linear layer on the rows (spconv's (out, 1, 1, 1, in) parameter, no neighbour table)
            self.proj_conv = PointwiseConv3d(in_channels, embed_channels, kernel_size=1, bias=False)
            self.proj_norm = norm_fn(embed_channels)
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

    def _forward_fused(self, x, prompt, skip):
        """SpUNet-v1m1's fused block with the folded pairs of the PDBatchNorms: two launches where wired"""
        xa = x.features
        m, ca = xa.shape
        cb = 0 if skip is None else skip.shape[1]
        cout = self.embed_channels
        nbr = x.neighbors(3, self.conv1.indice_key)
        order = x.row_order
        s1, t1 = self.bn1.folded(prompt)
        s2, t2 = self.bn2.folded(prompt)
        w1 = self.conv1._weight_for(torch.float32, ca + cb)
        w2 = self.conv2._weight_for(torch.float32, cout)
        if self.in_channels != self.embed_channels:
            wp = self.proj_conv._weight_for(torch.float32, ca + cb)
            sp, tp = self.proj_norm.folded(prompt)
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

    def forward(self, x, prompt, skip=None):
        """x: SparseConvTensor.  skip (optional, (m, C_skip)): the block input is cat(x.features, skip) (:421)."""
        if self.fused and not self.training and self._fusable():
            return self._forward_fused(x, prompt, skip)
        if skip is not None:
            x = x.replace_feature(torch.cat((x.features, skip), dim=1))
        residual = x
        out = self.conv1(x)
        out = out.replace_feature(self.bn1(out.features, act=ops.ACT_RELU, prompt=prompt))
        out = self.conv2(out)
        out = out.replace_feature(self.bn2(out.features, prompt=prompt))
        if self.in_channels == self.embed_channels:
            res = self.proj(residual).features
        else:
            res = self.proj_norm(self.proj_conv(residual).features, prompt=prompt)
        out = out.replace_feature(out.features + res)
        return out.replace_feature(self.relu(out.features))


class _ConvNormAct(nn.Module):
    """conv -> PDBatchNorm -> ReLU (:171-176); fused eval: the pair and the ReLU ride in the conv's epilogue"""

    def forward(self, x, prompt):
        if self.fused and not self.training:
            s, t = self.bn.folded(prompt)
            return self.conv(x, bn_scale=s, bn_shift=t, act=ops.ACT_RELU)
        out = self.conv(x)
        return out.replace_feature(self.bn(out.features, act=ops.ACT_RELU, prompt=prompt))


class SPConvDown(_ConvNormAct):
    def __init__(self, in_channels, out_channels, indice_key, kernel_size=2, bias=False, norm_fn=None):
        super().__init__()
        self.conv = SparseConv3d(in_channels, out_channels, kernel_size=kernel_size, stride=kernel_size, bias=bias,
                                 indice_key=indice_key)
        self.bn = norm_fn(out_channels)
        self.relu = ReLU()
        self.fused = True


class SPConvUp(_ConvNormAct):
    def __init__(self, in_channels, out_channels, indice_key, kernel_size=2, bias=False, norm_fn=None):
        super().__init__()
        self.conv = SparseInverseConv3d(in_channels, out_channels, kernel_size=kernel_size, bias=bias,
                                        indice_key=indice_key)
        self.bn = norm_fn(out_channels)
        self.relu = ReLU()
        self.fused = True


class SPConvPatchEmbedding(_ConvNormAct):
    def __init__(self, in_channels, out_channels, kernel_size=5, norm_fn=None):
        super().__init__()
        self.conv = SubMConv3d(in_channels, out_channels, kernel_size=kernel_size, padding=1, bias=False,
                               indice_key="stem")
        self.bn = norm_fn(out_channels)
        self.relu = ReLU()
        self.fused = True


@MODELS.register_module("SpUNet-v1m3")
class SpUNetBase(nn.Module):
    def __init__(self, in_channels, num_classes=0, base_channels=32, context_channels=256,
                 channels=(32, 64, 128, 256, 256, 128, 96, 96), layers=(2, 3, 4, 6, 2, 2, 2, 2), enc_mode=False,
                 conditions=("ScanNet", "S3DIS", "Structured3D"), zero_init=True, norm_decouple=True, norm_adaptive=True,
                 norm_affine=False):
        super().__init__()
        assert len(layers) % 2 == 0
        assert len(layers) == len(channels)
        if zero_init and not norm_adaptive:
            raise ValueError("SpUNet-v1m3: zero_init=True zeroes the modulation, which norm_adaptive=False does not "
                             "build; pass zero_init=False with norm_adaptive=False")
        self.in_channels = in_channels
        self.num_classes = num_classes
        self.base_channels = base_channels
        self.channels = channels
        self.layers = layers
        self.num_stages = len(layers) // 2
        self.enc_mode = enc_mode
        self.conditions = conditions
        self.zero_init = zero_init
        self.context_channels = context_channels
        self.norm_decouple, self.norm_adaptive, self.norm_affine = norm_decouple, norm_adaptive, norm_affine

        norm_fn = partial(PDBatchNorm, eps=1e-3, momentum=0.01, conditions=conditions,
                          context_channels=context_channels, decouple=norm_decouple, adaptive=norm_adaptive,
                          affine=norm_affine)
        block = BasicBlock

        self.conv_input = SPConvPatchEmbedding(in_channels, base_channels, kernel_size=5, norm_fn=norm_fn)
        enc_channels = base_channels
        dec_channels = channels[-1]
        self.down = nn.ModuleList()
        self.up = nn.ModuleList()
        self.enc = nn.ModuleList()
        self.dec = nn.ModuleList() if not self.enc_mode else None
        for s in range(self.num_stages):
            self.down.append(SPConvDown(enc_channels, channels[s], kernel_size=2, bias=False,
                                        indice_key=f"spconv{s + 1}", norm_fn=norm_fn))
            self.enc.append(SparseSequential(OrderedDict(
                (f"block{i}", block(channels[s], channels[s], norm_fn=norm_fn, indice_key=f"subm{s + 1}"))
                for i in range(layers[s]))))
            if not self.enc_mode:
                self.up.append(SPConvUp(channels[len(channels) - s - 2], dec_channels, kernel_size=2, bias=False,
                                        indice_key=f"spconv{s + 1}", norm_fn=norm_fn))
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

        self.fused = True
        self.modulation_path = None      # None: MODULATION_WIRED decides; True / False: one launch / per layer
        self._tables = {}                # condition index -> ops.pdnorm_table
        self._folds = {}                 # condition index -> (versions, [(scale, shift)])
        for i, m in enumerate(self.pdnorms()):
            m.slot = i

    def _init_weights(self, m):
        # :373-389, in the reference's order: apply() reaches a PDBatchNorm after its Linear and its BatchNorms
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, SubMConv3d):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.BatchNorm1d):
            if m.affine:
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)
        elif isinstance(m, PDBatchNorm):
            if self.zero_init:
                nn.init.constant_(m.modulation[-1].weight, 0)
                nn.init.constant_(m.modulation[-1].bias, 0)

    def pdnorms(self):
        """every PDBatchNorm in module order: the layer order of the packed modulation"""
        return [m for m in self.modules() if isinstance(m, PDBatchNorm)]

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

    def set_modulation(self, mode):
        """None: MODULATION_WIRED decides per use (the default); True: all layers' modulation in one launch
        (ptv3_pdnorm_fwd / _bwd) wherever the kernel is capable; False: every layer composes its own."""
        self.modulation_path = mode
        return self

    # ---- the one-launch modulation path --------------------------------------------------------------------------
    def _one_launch(self, use, context):
        if not self.norm_adaptive:
            return False
        on = MODULATION_WIRED[use] if self.modulation_path is None else bool(self.modulation_path)
        if not (on and context.is_cuda):
            return False
        capable = self.__dict__.get("_pd_capable")
        if capable is None:      # the widths are fixed at construction
            capable = self.__dict__["_pd_capable"] = all(ops.pdnorm_capable(m.num_features, self.context_channels)
                                                         for m in self._pds())
        return capable

    def _pds(self):
        pds = self.__dict__.get("_pd_list")
        if pds is None:
            pds = self.__dict__["_pd_list"] = self.pdnorms()
        return pds

    def _layers(self, condition):
        index = list(self.conditions).index(condition) if self.norm_decouple else 0
        return [m.tensors(index) for m in self._pds()]

    def _table(self, condition, layers):
        """the device table of pointers for this condition; rebuilt only when a tensor it points at was replaced"""
        key = (parse_condition(condition) if self.norm_decouple else None, layers[0][0].device)
        tab = self._tables.get(key)
        if tab is None or tab.key != ops.pdnorm_table_key(layers):
            with torch.no_grad():
                tab = self._tables[key] = ops.pdnorm_table([tuple(None if t is None else t.detach() for t in ly)
                                                            for ly in layers])
        return tab

    def _pairs(self, prompt):
        """training / composition: every layer's (gamma_eff, beta_eff) in one taped call"""
        layers = self._layers(prompt.condition)
        tab = self._table(prompt.condition, layers)
        params = [ly[0] for ly in layers] + [ly[1] for ly in layers]
        if tab.affine:
            params += [ly[2] for ly in layers] + [ly[3] for ly in layers]
        ge, be = A.pdnorm_modulation(tab, prompt.context, params)
        return list(zip(ge, be))

    def _folded(self, prompt):
        """fused eval: every layer's (scale, shift) from one fold launch, cached on what it depends on"""
        layers = self._layers(prompt.condition)
        ver = tuple((t.data_ptr(), t._version) for ly in layers for t in ly if t is not None) + \
            ((prompt.source.data_ptr(), prompt.source._version),)
        key = (condition_key(prompt.condition), layers[0][0].device)
        hit = self._folds.get(key)
        if hit is None or hit[0] != ver:
            tab = self._table(prompt.condition, layers)
            with torch.no_grad():
                s, t, _ = ops.pdnorm_fwd(tab, prompt.context.detach().float().contiguous().view(-1), fold=True,
                                         eps=self._pds()[0].active(prompt.condition).eps, save=False)
                pairs = list(zip(s.split(tab.width_list), t.split(tab.width_list)))
                if any(c % 4 for c in tab.width_list):
                    # ptv3_res_conv reads its pair 16 bytes at a time: behind a width that is no multiple of 4 the
                    # slices of the packed buffer no longer start on such a boundary, so they get storage of their own
                    pairs = [(a.clone(), b.clone()) for a, b in pairs]
            # the entry keeps the source alive: its address stands in `ver`
            hit = self._folds[key] = (ver, pairs, prompt.source)
        return hit[1]

    def modulation_pairs(self, condition, context):
        """every layer's (gamma_eff, beta_eff) through the one-launch path, taped (tests and tools)"""
        return self._pairs(Prompt(condition, context))

    def modulation_folds(self, condition, context, source=None):
        """every layer's folded (scale, shift) through the one-launch path and its cache (tests and tools)"""
        return self._folded(Prompt(condition, context, source))

    def forget_modulation(self):
        """empties the fold caches of both paths: the next eval forward is a "first" one again"""
        self._folds.clear()
        for m in self._pds():
            m._cache = _ParamCache()

    def _prompt(self, input_dict):
        condition = input_dict["condition"] if "condition" in input_dict.keys() else None
        if self.norm_decouple:
            if condition is None:
                raise KeyError("SpUNet-v1m3: input_dict has no 'condition'")
            condition = parse_condition(condition)
            if condition not in self.conditions:
                raise KeyError(f"SpUNet-v1m3: condition {condition!r} is not one of {tuple(self.conditions)}")
        context = input_dict["context"] if "context" in input_dict.keys() else None
        source = input_dict["context_source"] if "context_source" in input_dict.keys() else None
        if self.norm_adaptive:
            if context is None:
                raise ValueError("SpUNet-v1m3(norm_adaptive=True) needs input_dict['context'], one row of "
                                 "context_channels (PPT's embedding_table(condition))")
            if context.dim() != 2 or context.shape[0] != 1 or context.shape[1] != self.context_channels:
                raise ValueError(f"SpUNet-v1m3: input_dict['context'] must be (1, {self.context_channels}), got "
                                 f"{tuple(context.shape)}")
        prompt = Prompt(condition, context, source)
        if self.norm_adaptive:
            fused_eval = self.fused and not self.training
            if fused_eval and self._one_launch("eval", context):
                prompt.folded = self._folded(prompt)
            elif not fused_eval and self._one_launch("train", context):
                prompt.pairs = self._pairs(prompt)
        return prompt

    def backbone(self, input_dict, taps=None):
        """-> (SparseConvTensor of the last stage, scene ends as a device tensor for that tensor's rows).  One host
        read here (spatial shape and offsets) and one per stage (the coarse row count)."""
        check_sync_batchnorm(self)
        prompt = self._prompt(input_dict)
        grid = input_dict["grid_coord"]
        offset = input_dict["offset"]
        head = torch.cat([grid.max(dim=0).values.long(), offset.long()]).tolist()     # the forward's entry read
        shape, ends = [v + MARGIN for v in head[:3]], head[3:]
        check_extent(type(self).__name__, shape, self.num_stages)
        batch = offset2batch(offset.long(), ends[-1])
        x = SparseConvTensor(features=input_dict["feat"].float().contiguous(),
                             indices=torch.cat([batch.unsqueeze(-1), grid], dim=1).int().contiguous(),
                             spatial_shape=shape, batch_size=len(ends))
        x = self.conv_input(x, prompt)
        skips = [x]
        if taps is not None:
            taps.append(x)
        for s in range(self.num_stages):
            x = self.down[s](x, prompt)
            for blk in self.enc[s]:
                x = blk(x, prompt)
            skips.append(x)
            if taps is not None:
                taps.append(x)
        x = skips.pop(-1)
        if self.enc_mode:
            # coarse rows are sorted by (b, x, y, z): scene k ends where the first row of a later scene stands
            scenes = torch.arange(1, len(ends) + 1, device=x.indices.device, dtype=torch.int32)
            return x, torch.searchsorted(x.indices[:, 0].contiguous(), scenes).long()
        for s in reversed(range(self.num_stages)):
            x = self.up[s](x, prompt)
            skip = skips.pop(-1).features
            for i, blk in enumerate(self.dec[s]):
                x = blk(x, prompt, skip) if i == 0 else blk(x, prompt)
            if taps is not None:
                taps.append(x)
        return x, offset

    def forward(self, input_dict, taps=None):
        with torch.autocast(device_type=input_dict["feat"].device.type, enabled=False):
            x, ends = self.backbone(input_dict, taps)
            x = self.final(x) if isinstance(self.final, _Final) else x
            if self.enc_mode:
                feat = x.features.contiguous()
                return A.scene_mean(feat, ends) if self.training else ops.scene_mean(feat, ends)
            return x.features
