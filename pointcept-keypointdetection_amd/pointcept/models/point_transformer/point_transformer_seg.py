"""PointTransformerLayer, TransitionDown and Bottleneck of Point Transformer V1 on MI355X.

Counterpart of the reference's pointcept/models/point_transformer/point_transformer_seg.py:19-120, 123-205, 320-370:
same constructors, attribute names and state_dict keys, and the same `[p, x, o]` list passed from module to module
(coordinates (n, 3), features (n, c), int32 cumulative scene ends (b)).

`.eval()` (with `fused = True`, the default): farthest point sampling, kNN, grouping, the linear layers with their
folded BatchNorm and the whole vector attention run as HIP kernels of libptv3_hip.so.  The list may carry a fourth
entry, a SceneOffsets with the scene ends as host integers; with it a forward reads nothing back from the device.
`.train()` (or `fused = False`): the torch composition of the reference's formulas over the HIP kNN and the taped HIP
grouping, with batch-statistic BatchNorm; farthest point sampling carries no gradient.
"""
import torch
import torch.nn as nn

import pointops
from pointops import _C
from ptv3_hip import ops
from pointcept.models.utils.sparse import _ParamCache
from .utils import LayerNorm1d


class SceneOffsets:
    """Cumulative scene ends as an int32 device tensor AND as host integers, one object per resolution level; it also
    keeps the level's kNN rows so that the Bottlenecks of one stage search once."""

    def __init__(self, host, dev):
        self.host, self.dev = list(host), dev
        self.next = None
        self.knn = {}

    @classmethod
    def read(cls, offset):
        """One read of the offsets from the device."""
        return cls(offset.tolist(), offset.int().contiguous())

    @classmethod
    def chain(cls, host, device, strides):
        """All levels of an encoder (floor division of every scene's size per stride) with one host-to-device copy."""
        levels = [list(host)]
        for s in strides:
            levels.append(_strided(levels[-1], s))
        dev = torch.tensor(levels, dtype=torch.int32, device=device)
        out = [cls(h, dev[i]) for i, h in enumerate(levels)]
        for a, b in zip(out, out[1:]):
            a.next = b
        return out

    def down(self, stride):
        host = _strided(self.host, stride)
        if self.next is None or self.next.host != host:
            self.next = SceneOffsets(host, torch.tensor(host, dtype=torch.int32, device=self.dev.device))
        return self.next

    def knn_rows(self, nsample, p):
        """Self-neighbours of the level's coordinates `p`; kept for as long as the caller passes the same tensor."""
        hit = self.knn.get(nsample)
        if hit is None or hit[0] is not p:
            hit = self.knn[nsample] = (p, _knn(nsample, p, self, p, self))
        return hit[1]


def _strided(ends, stride):
    out, total, prev = [], 0, 0
    for e in ends:
        total += (e - prev) // stride
        prev = e
        out.append(total)
    return out


def _knn(nsample, xyz, so, new_xyz, new_so):
    """pointops.knn_query's rows without its read-back of the offsets (the host copies were checked already)."""
    if so.host[-1] != xyz.shape[0] or new_so.host[-1] != new_xyz.shape[0]:
        raise ValueError(f"offsets end at {so.host[-1]} / {new_so.host[-1]} for {xyz.shape[0]} / {new_xyz.shape[0]} rows")
    m = new_xyz.shape[0]
    idx = torch.zeros((m, nsample), dtype=torch.int32, device=xyz.device)
    dist2 = torch.zeros((m, nsample), dtype=torch.float32, device=xyz.device)
    _C.knn_query_cuda(m, nsample, xyz.contiguous(), new_xyz.contiguous(), so.dev, new_so.dev, idx, dist2)
    return idx


def _linear(x, lin, cache, **epilogue):
    """ops.gemm with the weight padded to the kernel's K granularity (4 fp32 values)."""
    pad = (-x.shape[1]) % ops.k_granule(torch.float32)
    w = cache.get(("w", id(lin)), [lin.weight],
                  lambda: nn.functional.pad(lin.weight.detach().float(), (0, pad)).contiguous())
    if pad:
        x = nn.functional.pad(x, (0, pad))
    bias = None if lin.bias is None else cache.get(("b", id(lin)), [lin.bias], lambda: lin.bias.detach().float().contiguous())
    return ops.gemm(x.contiguous(), w, bias=bias, **epilogue)


def _folded(bn, cache, lin=None):
    params = [bn.weight, bn.bias, bn.running_mean, bn.running_var] + ([] if lin is None else [lin.bias])
    return cache.get(("bn", id(bn)), params, lambda: ops.fold_batchnorm(bn, None if lin is None else lin.bias))


def _scene_state(pxo):
    return pxo[3] if len(pxo) > 3 and pxo[3] is not None else SceneOffsets.read(pxo[2])


def _norm_mlp(width_in, hidden, width_out):
    """Linear, LayerNorm1d, ReLU, Linear as a list: module indices 0..3 of linear_p and 2..5 of linear_w."""
    return [nn.Linear(width_in, hidden), LayerNorm1d(hidden), nn.ReLU(inplace=True), nn.Linear(hidden, width_out)]


class PointTransformerLayer(nn.Module):
    def __init__(self, in_planes, out_planes, share_planes=8, nsample=16):
        super().__init__()
        cs = out_planes // share_planes    # channels of one share group = width of the attention weights
        # the reference keeps a separate q / k width that always equals out_planes
        self.mid_planes = self.out_planes = out_planes
        self.share_planes, self.nsample = share_planes, nsample
        for name in ("linear_q", "linear_k", "linear_v"):
            setattr(self, name, nn.Linear(in_planes, out_planes))
        self.linear_p = nn.Sequential(*_norm_mlp(3, 3, out_planes))
        self.linear_w = nn.Sequential(LayerNorm1d(out_planes), nn.ReLU(inplace=True), *_norm_mlp(out_planes, cs, cs))
        self.softmax = nn.Softmax(dim=1)   # over the neighbour slots
        self.fused = True
        self._cache = _ParamCache()

    def forward(self, pxo) -> torch.Tensor:
        p, x, o = pxo[:3]
        if self.training or not self.fused:
            return self.compose(p, x, o)
        if self.share_planes != 8:
            raise NotImplementedError("PointTransformerLayer: the fused eval kernel has 8 share groups")
        so = _scene_state(pxo)
        cache = self._cache
        x_q, x_k, x_v = (_linear(x, lin, cache) for lin in (self.linear_q, self.linear_k, self.linear_v))
        f = lambda t: cache.get(("f", id(t)), [t], lambda: t.detach().float().contiguous())   # noqa: E731
        lp, lw = self.linear_p, self.linear_w
        s_p, t_p = _folded(lp[1], cache, lp[0])
        s_c, t_c = _folded(lw[0], cache)
        s_w, t_w = _folded(lw[3], cache, lw[2])
        return ops.vector_attention(x_q, x_k, x_v, p.contiguous(), so.knn_rows(self.nsample, p), f(lp[0].weight), s_p,
                                    t_p, f(lp[3].weight), f(lp[3].bias), s_c, t_c, f(lw[2].weight), s_w, t_w,
                                    f(lw[5].weight), f(lw[5].bias))

    def compose(self, p, x, o):
        """point_transformer_seg.py:87-120 as torch ops over the HIP neighbour search and the taped HIP row gather."""
        p = p.contiguous()
        rows, _ = pointops.knn_query(self.nsample, p, o)                           # (n, ns), -1 = missing
        n, ns = rows.shape
        groups, cs = self.share_planes, self.out_planes // self.share_planes
        q = self.linear_q(x)
        k = pointops.grouping2(self.linear_k(x).contiguous(), rows)                # (n, ns, c); zero row for -1
        v = pointops.grouping2(self.linear_v(x).contiguous(), rows)
        present = (rows >= 0).to(p.dtype).unsqueeze(-1)
        pos = self.linear_p((pointops.grouping2(p, rows) - p.unsqueeze(1)) * present)   # (n, ns, c)
        # mid_planes == out_planes: the reference's sum over (i j) -> j has a single term
        w = self.softmax(self.linear_w(k - q.unsqueeze(1) + pos))                  # (n, ns, c / share)
        return ((v + pos).view(n, ns, groups, cs) * w.unsqueeze(2)).sum(1).view(n, groups * cs)


class TransitionDown(nn.Module):
    def __init__(self, in_planes, out_planes, stride=1, nsample=16):
        super().__init__()
        self.stride, self.nsample = stride, nsample
        strided = stride != 1     # a strided stage reads every neighbour's offset in front of its features
        self.linear = nn.Linear(in_planes + 3 * strided, out_planes, bias=False)
        if strided:
            self.pool = nn.MaxPool1d(nsample)
        self.bn, self.relu = nn.BatchNorm1d(out_planes), nn.ReLU(inplace=True)
        self.fused = True
        self._cache = _ParamCache()

    def forward(self, pxo):
        p, x, o = pxo[:3]
        so = _scene_state(pxo) if len(pxo) > 3 or self.stride != 1 else None
        fused = self.fused and not self.training
        if self.stride == 1:
            if fused:
                scale, shift = _folded(self.bn, self._cache)
                x = _linear(x, self.linear, self._cache, bn_scale=scale, bn_shift=shift, act=ops.ACT_RELU)
            else:
                x = self.relu(self.bn(self.linear(x)))
            return [p, x, o, so]
        nso = so.down(self.stride)
        idx = ops.farthest_point_sampling(p.contiguous(), so.dev, nso.dev, so.host, nso.host)
        n_p = p[idx.long(), :]
        knn = _knn(self.nsample, p, so, n_p, nso)
        x = pointops.grouping(knn, x.contiguous(), p.contiguous(), n_p, with_xyz=True)     # (m, nsample, 3 + c)
        m, ns, width = x.shape
        if fused:
            scale, shift = _folded(self.bn, self._cache)
            x = _linear(x.view(m * ns, width), self.linear, self._cache, bn_scale=scale, bn_shift=shift,
                        act=ops.ACT_RELU)
            x = x.view(m, ns, -1).max(dim=1).values
        else:
            x = self.bn(self.linear(x).flatten(0, 1))          # batch statistics over every (sample, neighbour) row
            x = self.pool(self.relu(x).view(m, ns, -1).transpose(1, 2)).flatten(1)
        return [n_p, x, nso.dev, nso]


class Bottleneck(nn.Module):
    expansion = 1

    def __init__(self, in_planes, planes, share_planes=8, nsample=16):
        super().__init__()
        width = planes * self.expansion
        self.linear1, self.bn1 = nn.Linear(in_planes, planes, bias=False), nn.BatchNorm1d(planes)
        self.transformer, self.bn2 = PointTransformerLayer(planes, planes, share_planes, nsample), nn.BatchNorm1d(planes)
        self.linear3, self.bn3 = nn.Linear(planes, width, bias=False), nn.BatchNorm1d(width)
        self.relu = nn.ReLU(inplace=True)
        self.fused = True
        self._cache = _ParamCache()

    def forward(self, pxo):
        p, x, o = pxo[:3]
        so = pxo[3] if len(pxo) > 3 else None
        identity = x
        if self.fused and not self.training:
            cache = self._cache
            s1, t1 = _folded(self.bn1, cache)
            s2, t2 = _folded(self.bn2, cache)
            s3, t3 = _folded(self.bn3, cache)
            x = _linear(x, self.linear1, cache, bn_scale=s1, bn_shift=t1, act=ops.ACT_RELU)
            x = ops.affine_act(self.transformer([p, x, o, so]), s2, t2, ops.ACT_RELU)
            x = _linear(x, self.linear3, cache, bn_scale=s3, bn_shift=t3, res=identity.contiguous())
            x = ops.affine_act(x, None, None, ops.ACT_RELU)
        else:
            y = torch.relu(self.bn1(self.linear1(x)))
            y = torch.relu(self.bn2(self.transformer([p, y, o, so])))
            x = torch.relu(identity + self.bn3(self.linear3(y)))
        return [p, x, o, so]
