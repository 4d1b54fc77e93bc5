"""Submanifold sparse convolution on MI355X: the stand-in for `spconv.pytorch` on the PTv3 path.

The reference builds `spconv.SparseConvTensor` in Point.sparsify (models/utils/structure.py:111-146)
and runs `spconv.SubMConv3d` in Embedding / Block.cpe (point_transformer_v3m1_base.py:277-284,499-506).
spconv 2.3.6 is a CUDA-only wheel; here the same two names are backed by libptv3_hip.so:
a site hash + neighbour table per (indice_key, kernel_size) and the implicit-GEMM kernel.
Weight layout (out, k, k, k, in) and correlation offset order follow spconv 2.x ("parity
unpinned" for loading real spconv checkpoints - the wheel cannot be run here).
OA-CNNs (models/oacnns/oacnns_v1m1_base.py:130-141, 184-194) adds `SparseConv3d` / `SparseInverseConv3d` for kernel 2 /
stride 2 and `SparseSequential`: no hash there, a sorted parent key and an (m_out, 8) child table.
"""
import math

import torch
import torch.nn as nn

from ptv3_hip import ops
from ptv3_hip import autograd as A


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size, _shared=None, _strided=None):
        self.features = features
        self.indices = indices  # (n, 4) int32 [batch, x, y, z]
        self.spatial_shape = spatial_shape
        self.batch_size = batch_size
        # neighbour tables are shared by every tensor derived through replace_feature (spconv's indice_dict)
        self._shared = _shared if _shared is not None else {"table": None, "nbr": {}, "row_order": None}
        # plans of the strided convs by indice_key, shared by every level of one forward (SparseInverseConv3d looks
        # its down conv up here); each level has its own neighbour tables in `_shared`
        self._strided = _strided if _strided is not None else {}

    def replace_feature(self, feature):
        return SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size, self._shared, self._strided)

    def neighbors(self, ksize, indice_key=None):
        key = (indice_key, ksize) if indice_key is not None else ("_k", ksize)
        if key not in self._shared["nbr"]:
            nbr, table = ops.subm_neighbors(self.indices, ksize, self._shared["table"])
            self._shared["table"] = table
            self._shared["nbr"][key] = nbr
        return self._shared["nbr"][key]

    @property
    def row_order(self):
        return self._shared["row_order"]

    @row_order.setter
    def row_order(self, v):
        self._shared["row_order"] = v


class _ParamCache:
    """Casts / re-lays-out parameters once per parameter version (eval: once)."""

    def __init__(self):
        self._c = {}

    def get(self, key, params, fn):
        ver = tuple((p.data_ptr(), p._version) for p in params)
        hit = self._c.get(key)
        if hit is None or hit[0] != ver:
            with torch.no_grad():
                hit = (ver, fn())
            self._c[key] = hit
        return hit[1]


class SubMConv3d(nn.Module):
    """spconv.pytorch.SubMConv3d(in, out, kernel_size, bias=..., indice_key=...) on the HIP path."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1,
                 bias=True, indice_key=None, algo=None, **kwargs):
        super().__init__()
        assert stride == 1 and dilation == 1 and groups == 1, "only the configuration PTv3 uses"
        assert isinstance(kernel_size, int) and kernel_size % 2 == 1
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, kernel_size
        self.indice_key = indice_key
        k = kernel_size
        self.weight = nn.Parameter(torch.empty(out_channels, k, k, k, in_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()
        self._cache = _ParamCache()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.in_channels * self.kernel_size ** 3
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)

    def _weight_for(self, dtype, cin_pad):
        def make():
            w = self.weight.detach()
            if cin_pad != self.in_channels:
                w = torch.nn.functional.pad(w, (0, cin_pad - self.in_channels))
            return w.reshape(self.out_channels, -1).to(dtype).contiguous()
        return self._cache.get(("w", dtype, cin_pad), [self.weight], make)

    def forward(self, x: SparseConvTensor, bn_scale=None, bn_shift=None, act=ops.ACT_NONE):
        if self.training:
            if bn_scale is not None or act != ops.ACT_NONE:
                raise NotImplementedError("training-mode SubMConv3d: BN / activation epilogues are eval-only fusions")
            nbr = x.neighbors(self.kernel_size, self.indice_key)
            return x.replace_feature(A.subm_conv(x.features, self.weight, self.bias, nbr, x.row_order))
        feat = x.features
        cin = feat.shape[1]
        gran = ops.k_granule(feat.dtype)
        cin_pad = (cin + gran - 1) // gran * gran
        if cin_pad != cin:  # kernel wants 16-byte K granularity: zero-pad features and weights alike
            feat = torch.nn.functional.pad(feat, (0, cin_pad - cin)).contiguous()
        nbr = x.neighbors(self.kernel_size, self.indice_key)
        w = self._weight_for(feat.dtype, cin_pad)
        bias = None if self.bias is None else self.bias.detach().float()
        out = ops.gemm(feat, w, bias=bias, nbr=nbr, kvol=self.kernel_size ** 3, row_order=x.row_order,
                       bn_scale=bn_scale, bn_shift=bn_shift, act=act)
        return x.replace_feature(out)


def _only_2(v, what):
    vals = (v,) * 3 if isinstance(v, int) else tuple(v)
    if vals != (2, 2, 2):
        raise NotImplementedError(f"{what}={v}: only 2 is implemented (the OA-CNNs / SpUNet down-sampling pair)")


class SparseConv3d(nn.Module):
    """spconv.pytorch.SparseConv3d(in, out, kernel_size=2, stride=2, indice_key=...): every fine site has one coarse
    parent (b, x>>1, y>>1, z>>1) and one tap, the output shape is (S - 2) // 2 + 1 per axis and a site whose parent
    falls outside it contributes nothing.  Coarse rows are ordered by (b, x, y, z) (spconv's order is unspecified;
    parity with the wheel unpinned).  Eval: ptv3_down2_conv with the BatchNorm / ReLU epilogue; training, or
    fused = False: gather by the child table and the taped Linear."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, bias=True,
                 indice_key=None, algo=None, **kwargs):
        super().__init__()
        _only_2(kernel_size, "kernel_size")
        _only_2(stride, "stride")
        if padding != 0 or dilation != 1 or groups != 1:
            raise NotImplementedError("SparseConv3d: padding, dilation and groups are not implemented")
        if in_channels % 4:
            raise NotImplementedError("SparseConv3d: in_channels must be a multiple of 4")
        self.in_channels, self.out_channels, self.kernel_size, self.stride = in_channels, out_channels, 2, 2
        self.indice_key = indice_key
        self.weight = nn.Parameter(torch.empty(out_channels, 2, 2, 2, in_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.fused = True
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1 / math.sqrt(self.in_channels * 8)
            nn.init.uniform_(self.bias, -bound, bound)

    def _epilogue(self, bn_scale, bn_shift):
        """the conv's own bias rides in the epilogue's shift"""
        if self.bias is None:
            return bn_scale, bn_shift
        b = self.bias.detach().float()
        if bn_scale is None:
            return torch.ones_like(b), b.contiguous()
        return bn_scale, (bn_shift + b * bn_scale).contiguous()

    def _compose(self, feat, plan):
        child = plan.long_indices()[0]
        padded = torch.cat([feat, feat.new_zeros(1, feat.shape[1])])      # row n: the missing child
        rows = padded.index_select(0, child.reshape(-1)).view(plan.m_out, 8 * self.in_channels)
        return A.linear(rows, self.weight.view(self.out_channels, 8 * self.in_channels), self.bias)

    def forward(self, x: SparseConvTensor, bn_scale=None, bn_shift=None, act=ops.ACT_NONE):
        plan = ops.down2_plan(x.indices, x.spatial_shape, x.batch_size)
        if self.indice_key is not None:
            x._strided[self.indice_key] = (plan, x)
        feat = x.features.float().contiguous()
        if self.training or not self.fused:
            if bn_scale is not None or act != ops.ACT_NONE:
                raise NotImplementedError("SparseConv3d: BN / activation epilogues belong to the fused eval path")
            out = self._compose(feat, plan)
        else:
            scale, shift = self._epilogue(bn_scale, bn_shift)
            out = ops.down2_conv(feat, self.weight.detach(), plan, scale, shift, act)
        return SparseConvTensor(out, plan.coarse, plan.out_shape, x.batch_size, None, x._strided)


class SparseInverseConv3d(nn.Module):
    """spconv.pytorch.SparseInverseConv3d(in, out, kernel_size=2, indice_key=...): out[i] = W[:, tap(i), :] y[parent(i)]
    on the fine sites of the SparseConv3d that ran under the same indice_key, in their own order; a site that had no
    parent gets zero (plus the bias).  Rows are processed sorted by tap, so a row costs one tap of multiply work."""

    def __init__(self, in_channels, out_channels, kernel_size, indice_key=None, bias=True, algo=None, **kwargs):
        super().__init__()
        _only_2(kernel_size, "kernel_size")
        if indice_key is None:
            raise ValueError("SparseInverseConv3d needs the indice_key of its SparseConv3d")
        if in_channels % 4:
            raise NotImplementedError("SparseInverseConv3d: in_channels must be a multiple of 4")
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, 2
        self.indice_key = indice_key
        self.weight = nn.Parameter(torch.empty(out_channels, 2, 2, 2, in_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.fused = True
        self.reset_parameters()

    reset_parameters = SparseConv3d.reset_parameters
    _epilogue = SparseConv3d._epilogue

    def _compose(self, feat, plan):
        _, parent, rows, inv = plan.long_indices()
        w = self.weight.view(self.out_channels, 8, self.in_channels)
        ts = plan.tap_start
        parts = []
        for t in range(8):          # per tap the parents are distinct: the gather's backward adds nothing twice
            if ts[t + 1] > ts[t]:
                src = feat.index_select(0, parent.index_select(0, rows[ts[t]:ts[t + 1]]))
                parts.append(A.linear(src, w[:, t], self.bias))
        if plan.dropped:
            zero = feat.new_zeros(plan.dropped, self.out_channels)
            parts.append(zero if self.bias is None else zero + self.bias)
        return torch.cat(parts).index_select(0, inv)

    def forward(self, x: SparseConvTensor, bn_scale=None, bn_shift=None, act=ops.ACT_NONE):
        if self.indice_key not in x._strided:
            raise KeyError(f"SparseInverseConv3d: no SparseConv3d ran under indice_key {self.indice_key!r}")
        plan, fine = x._strided[self.indice_key]
        feat = x.features.float().contiguous()
        if feat.shape[0] != plan.m_out:
            raise RuntimeError("SparseInverseConv3d: the input is not on the coarse sites of its indice_key")
        if self.training or not self.fused:
            if bn_scale is not None or act != ops.ACT_NONE:
                raise NotImplementedError("SparseInverseConv3d: BN / activation epilogues belong to the fused eval path")
            out = self._compose(feat, plan)
        else:
            scale, shift = self._epilogue(bn_scale, bn_shift)
            out = ops.up2_conv(feat, self.weight.detach(), plan, scale, shift, act)
        return SparseConvTensor(out, fine.indices, fine.spatial_shape, fine.batch_size, fine._shared, x._strided)


def is_spconv_module(module):
    return isinstance(module, (SubMConv3d, SparseConv3d, SparseInverseConv3d))


class SparseSequential(nn.Sequential):
    """spconv.pytorch.SparseSequential: sparse convs take the SparseConvTensor, every other module its feature matrix.
    Eval with fused = True: a BatchNorm1d and a ReLU that follow a conv run in the conv kernel's epilogue."""

    def __init__(self, *args):
        super().__init__(*args)
        self.fused = True

    def forward(self, x):
        mods = list(self)
        fold = self.fused and not self.training
        i = 0
        while i < len(mods):
            m = mods[i]
            if is_spconv_module(m):
                kw = {}
                if fold and i + 1 < len(mods) and hasattr(mods[i + 1], "folded"):
                    kw["bn_scale"], kw["bn_shift"] = mods[i + 1].folded()
                    i += 1
                if fold and i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU):
                    kw["act"] = ops.ACT_RELU
                    i += 1
                x = m(x, **kw)
            elif isinstance(x, SparseConvTensor):
                x = x.replace_feature(m(x.features))
            else:
                x = m(x)
            i += 1
        return x
