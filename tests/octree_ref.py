"""CPU restatement of what OctFormer takes from ocnn, dwconv and torch_scatter, in plain torch.

Neither ocnn nor dwconv is installed where the fixtures are built, so these stand-ins are written from the published
sources (ocnn-pytorch: ocnn/octree/{points,octree,shuffled_key}.py, ocnn/nn/{octree_conv,octree_pad,octree_interp,
octree_drop}.py, ocnn/modules/modules.py; octformer: dwconv) and PARITY WITH THE PACKAGES IS UNPINNED.  They serve two
ends: tests/golden/make_golden_keypoint_octformer.py puts them into sys.modules so that the reference's own model files
import and run on the CPU, and the tests compare ops.octree_build and the kernels' tables against them.  Only
nempty=True, the mode the fork uses, is restated: every tensor of a depth has one row per non-empty node, in key order.

Restated rules:
  cells      p = points (already coord / scale_factor), cell = floor((p + 1) * 2^(depth-1)) in fp32; -1 <= p < 1 or ValueError
  keys       key = scene << 48 | interleave(x, y, z), x in the highest bit of each triple; the nodes of depth d are the
             sorted unique leaf keys with the 48 cell bits >> 3 (depth - d) under the scene id
  features   the mean of the point features of a leaf
  conv       weights (kdim, cin, cout); kernel [3]: tap (dx+1)*9 + (dy+1)*3 + (dz+1), a missing neighbour adds nothing;
             kernel [2] stride 2: a parent sums its children, tap (x&1)*4 + (y&1)*2 + (z&1)
  deconv     kernel [3] stride 2, weights (27, cout, cin): the transpose of the stride-2 3^3 convolution whose window of
             parent P covers the fine cells 2P + {-1, 0, 1}: fine cell 2P + o receives x[P] @ weights[tap(o)].T
  dwconv     weights (27, 1, C): out[i] = sum_t weights[t, 0] * x[neighbour t of i]
  upsample   nearest: a node's row goes to its non-empty children;  interp nearest: a point takes its leaf's row
  drop path  one keep decision per scene, scaled by 1 / keep; identity in eval and at rate 0
  BatchNorm  ocnn.modules uses eps 1e-3 and momentum 0.01
"""
import sys
import types

import torch
import torch.nn as nn

BN_EPS, BN_MOMENTUM = 1e-3, 0.01


def xyz2key(x, y, z, b, depth):
    key = torch.zeros_like(x, dtype=torch.int64)
    for i in range(depth):
        bit = 1 << i
        key |= ((x.long() & bit) << (2 * i + 2)) | ((y.long() & bit) << (2 * i + 1)) | ((z.long() & bit) << (2 * i))
    return key | (torch.as_tensor(b).long() << 48)


def key2xyz(key, depth):
    x, y, z = (torch.zeros_like(key) for _ in range(3))
    for i in range(depth):
        x |= ((key >> (3 * i + 2)) & 1) << i
        y |= ((key >> (3 * i + 1)) & 1) << i
        z |= ((key >> (3 * i)) & 1) << i
    return x, y, z, key >> 48


def cells(points, depth):
    p = points.float()
    if not bool(((p >= -1) & (p < 1)).all()):
        raise ValueError("a point lies outside -1 <= p < 1 (the octree's domain)")
    return torch.floor((p + 1.0) * float(2 ** (depth - 1))).long()


class Points:
    def __init__(self, points, normals=None, features=None, labels=None, batch_id=None, batch_size=1):
        self.points, self.normals, self.features, self.batch_id, self.batch_size = points, normals, features, batch_id, batch_size


class Octree:
    def __init__(self, depth, full_depth=2, batch_size=1, device="cpu", **kwargs):
        self.depth, self.full_depth, self.batch_size, self.device = depth, full_depth, batch_size, device
        self.keys, self.parent, self.children, self.neighs, self.features = {}, {}, {}, {}, {}
        self.nnum = self.nnum_nempty = torch.zeros(depth + 1, dtype=torch.int32)
        self.leaf = None

    def build_octree(self, point_cloud):
        d = self.depth
        c = cells(point_cloud.points, d)
        b = point_cloud.batch_id.view(-1)
        key = xyz2key(c[:, 0], c[:, 1], c[:, 2], b, d)
        self.keys[d], self.leaf = torch.unique(key, sorted=True, return_inverse=True)
        for k in range(d - 1, 0, -1):
            up = ((self.keys[k + 1] >> 48) << 48) | ((self.keys[k + 1] & ((1 << 48) - 1)) >> 3)   # the scene id stays
            self.keys[k], self.parent[k + 1] = torch.unique(up, sorted=True, return_inverse=True)
            child = torch.full((len(self.keys[k]), 8), -1, dtype=torch.int64)
            child[self.parent[k + 1], self.keys[k + 1] & 7] = torch.arange(len(self.keys[k + 1]))
            self.children[k] = child
        self.nnum = self.nnum_nempty = torch.tensor([0] + [len(self.keys[k]) for k in range(1, d + 1)], dtype=torch.int32)
        f = point_cloud.features
        total = f.new_zeros((len(self.keys[d]), f.shape[1])).index_add_(0, self.leaf, f)
        self.features[d] = total / torch.bincount(self.leaf, minlength=len(total)).to(f.dtype).unsqueeze(1)
        return self.leaf

    def key(self, depth, nempty=True):
        assert nempty
        return self.keys[depth]

    def batch_id(self, depth, nempty=True):
        assert nempty
        return self.keys[depth] >> 48

    def xyzb(self, depth):
        return key2xyz(self.keys[depth], depth)

    def search_xyzb(self, x, y, z, b, depth):
        """row of the cell at `depth`, -1 where it is empty or outside the grid"""
        top = 1 << depth
        ok = (x >= 0) & (x < top) & (y >= 0) & (y < top) & (z >= 0) & (z < top)
        key = xyz2key(x.clamp(0, top - 1), y.clamp(0, top - 1), z.clamp(0, top - 1), b, depth)
        keys = self.keys[depth]
        pos = torch.searchsorted(keys, key).clamp(max=len(keys) - 1)
        return torch.where(ok & (keys[pos] == key), pos, torch.full_like(pos, -1))

    def construct_all_neigh(self):
        for d in range(1, self.depth + 1):
            x, y, z, b = self.xyzb(d)
            cols = [self.search_xyzb(x + dx, y + dy, z + dz, b, d) for dx in (-1, 0, 1) for dy in (-1, 0, 1)
                    for dz in (-1, 0, 1)]
            self.neighs[d] = torch.stack(cols, dim=1)

    def deconv_pairs(self, depth):
        """(parent row at depth, tap, fine row at depth + 1) of the stride-2 3^3 window 2P + {-1, 0, 1}"""
        x, y, z, b = self.xyzb(depth)
        rows = torch.arange(len(x))
        out = []
        for t, (dx, dy, dz) in enumerate((a, c, e) for a in (-1, 0, 1) for c in (-1, 0, 1) for e in (-1, 0, 1)):
            fine = self.search_xyzb(2 * x + dx, 2 * y + dy, 2 * z + dz, b, depth + 1)
            ok = fine >= 0
            out.append(torch.stack([rows[ok], torch.full_like(rows[ok], t), fine[ok]], dim=1))
        return torch.cat(out)


def _gather(x, idx):
    xp = torch.cat([x, x.new_zeros((1,) + tuple(x.shape[1:]))])
    return xp[torch.where(idx >= 0, idx, torch.full_like(idx, len(x)))]


class OctreeConv(nn.Module):
    deconv = False

    def __init__(self, in_channels, out_channels, kernel_size=(3,), stride=1, nempty=False, direct_method=False,
                 use_bias=False, max_buffer=int(2e8)):
        super().__init__()
        assert nempty, "only nempty=True is restated"
        self.k, self.stride = list(kernel_size)[0], stride
        assert (self.k, stride, self.deconv) in ((3, 1, False), (2, 2, False), (3, 2, True))
        cin, cout = (out_channels, in_channels) if self.deconv else (in_channels, out_channels)
        self.weights = nn.Parameter(torch.empty(self.k ** 3, cin, cout))
        nn.init.xavier_uniform_(self.weights)
        self.bias = nn.Parameter(torch.zeros(out_channels)) if use_bias else None
        self.out_channels = out_channels

    def forward(self, data, octree, depth):
        if self.deconv:
            pairs = octree.deconv_pairs(depth)
            contrib = torch.einsum("ec,eoc->eo", data[pairs[:, 0]], self.weights[pairs[:, 1]])
            out = data.new_zeros((len(octree.keys[depth + 1]), self.out_channels)).index_add_(0, pairs[:, 2], contrib)
        else:
            table = octree.neighs[depth] if self.k == 3 else octree.children[depth - 1]
            out = torch.einsum("ntc,tco->no", _gather(data, table), self.weights)
        return out if self.bias is None else out + self.bias


class OctreeDeconv(OctreeConv):
    deconv = True


class OctreeDWConv(nn.Module):
    def __init__(self, in_channels, kernel_size=(3,), nempty=False, use_bias=False):
        super().__init__()
        assert nempty and list(kernel_size) == [3] and not use_bias
        self.weights = nn.Parameter(torch.empty(27, 1, in_channels))
        nn.init.xavier_uniform_(self.weights)

    def forward(self, data, octree, depth):
        return (_gather(data, octree.neighs[depth]) * self.weights[:, 0]).sum(1)


class OctreeConvBnRelu(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=(3,), stride=1, nempty=False):
        super().__init__()
        self.conv = OctreeConv(in_channels, out_channels, kernel_size, stride, nempty)
        self.bn = nn.BatchNorm1d(out_channels, BN_EPS, BN_MOMENTUM)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, data, octree, depth):
        return self.relu(self.bn(self.conv(data, octree, depth)))


class OctreeDeconvBnRelu(nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size=(3,), stride=1, nempty=False):
        super().__init__()
        self.deconv = OctreeDeconv(in_channels, out_channels, kernel_size, stride, nempty)
        self.bn = nn.BatchNorm1d(out_channels, BN_EPS, BN_MOMENTUM)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, data, octree, depth):
        return self.relu(self.bn(self.deconv(data, octree, depth)))


class OctreeUpsample(nn.Module):
    def __init__(self, method="nearest", nempty=False):
        super().__init__()
        assert method == "nearest" and nempty

    def forward(self, data, octree, depth, target_depth=None):
        target_depth = depth + 1 if target_depth is None else target_depth
        for d in range(depth, target_depth):
            data = data[octree.parent[d + 1]]
        return data


class OctreeInterp(nn.Module):
    def __init__(self, method="nearest", nempty=False, bound_check=False, rescale_pts=True):
        super().__init__()
        assert method == "nearest" and nempty

    def forward(self, data, octree, depth, pts, rescale_pts=True):
        c = torch.floor((pts[:, :3].float() + 1.0) * float(2 ** (depth - 1))).long()
        idx = octree.search_xyzb(c[:, 0], c[:, 1], c[:, 2], pts[:, 3].long(), depth)
        return _gather(data, idx)


class OctreeDropPath(nn.Module):
    def __init__(self, drop_prob=0.0, nempty=False, scale_by_keep=True):
        super().__init__()
        self.drop_prob, self.scale_by_keep = drop_prob, scale_by_keep

    def forward(self, data, octree, depth, batch_id=None):
        if self.drop_prob <= 0.0 or not self.training:
            return data
        keep = 1.0 - self.drop_prob
        mask = torch.floor(keep + torch.rand(octree.batch_size, 1, dtype=data.dtype))
        if keep > 0.0 and self.scale_by_keep:
            mask = mask / keep
        return data * mask[octree.batch_id(depth, True)]


def scatter_mean(src, index, dim=0):
    assert dim == 0
    b = int(index.max()) + 1
    total = src.new_zeros((b,) + tuple(src.shape[1:])).index_add_(0, index, src)
    return total / torch.bincount(index, minlength=b).clamp(min=1).to(src.dtype).view(-1, *([1] * (src.dim() - 1)))


def install_standins():
    """ocnn, dwconv and torch_scatter.scatter_mean as far as the reference's OctFormer files use them"""
    ocnn = types.ModuleType("ocnn")
    octree, nn_, modules = (types.ModuleType("ocnn." + n) for n in ("octree", "nn", "modules"))
    octree.Octree, octree.Points, octree.key2xyz, octree.xyz2key = Octree, Points, key2xyz, xyz2key
    nn_.OctreeConv, nn_.OctreeDeconv, nn_.OctreeUpsample, nn_.OctreeInterp = OctreeConv, OctreeDeconv, OctreeUpsample, OctreeInterp
    nn_.OctreeDropPath = OctreeDropPath
    modules.OctreeConvBnRelu, modules.OctreeDeconvBnRelu = OctreeConvBnRelu, OctreeDeconvBnRelu
    ocnn.octree, ocnn.nn, ocnn.modules = octree, nn_, modules
    dw = types.ModuleType("dwconv")
    dw.OctreeDWConv = OctreeDWConv
    sys.modules.update({"ocnn": ocnn, "ocnn.octree": octree, "ocnn.nn": nn_, "ocnn.modules": modules, "dwconv": dw})
    ts = sys.modules.setdefault("torch_scatter", types.ModuleType("torch_scatter"))
    ts.scatter_mean = scatter_mean


class Levels:
    """An Octree of this file in the attribute names of ptv3_hip.ops.OctreeLevels, for running the package's torch
    composition on the CPU (data_dict["octree"])."""

    def __init__(self, octree, min_depth):
        from ptv3_hip import ops
        self.depth, self.min_depth, self.batch_size = octree.depth, min_depth, octree.batch_size
        ds = range(min_depth, octree.depth + 1)
        self.keys = {d: octree.keys[d] for d in ds}
        self.nnum = {d: len(octree.keys[d]) for d in ds}
        self.xyz = {d: torch.stack(octree.xyzb(d)[:3], dim=1).int() for d in ds}
        self.batch = {d: (octree.keys[d] >> 48).int() for d in ds}
        self.parent = {d: octree.parent[d] for d in ds if d > min_depth}
        self.children = {d: octree.children[d].int() for d in ds if d < octree.depth}
        self.leaf, self.features = octree.leaf, octree.features[octree.depth]
        self._nbr = {d: octree.neighs[d].int() for d in ds}
        self._deconv, self._down = {}, {}
        self.neighbors = types.MethodType(ops.OctreeLevels.neighbors, self)
        self.deconv_table = types.MethodType(ops.OctreeLevels.deconv_table, self)
