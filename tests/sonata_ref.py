"""Yardstick of the Sonata self-distillation loss (csrc/sonata_loss.hip, pointcept/models/sonata): the reference's literal
formulation (pointcept/models/sonata/sonata_v1m1_base.py:267-291 and :443-454) restated in plain torch, in whatever
dtype and on whatever device its inputs have - float64 on the CPU is the yardstick, float32 on the device the run whose
error sets the kernels' bound.  
  sinkhorn_knopp   exp, the division by the total, three rounds of row sum / divide / column sum / divide, the final * n
  pair_loss        -sum_k target log_softmax(student / tau) per pair
  scene_mean       segment_coo(reduce="mean") with dim_size = index.max() + 1 as torch_scatter documents it: a scene
                   without a pair below the last one that has any counts with 0, the ones behind it do not exist
  loss             the mean over those scenes
  sweeps           the K-vectors A_i, u_i of the three sweeps and the row scale d of the scaling form, read off the
                   literal iteration's own row and column sums (so that a kernel sweep can be checked on its own)
  dstudent         the analytic gradient to the student logits
"""
import torch


def sinkhorn_knopp(feat, temp, num_iter=3):
    """(M, K) assignment; rows sum to one"""
    q = torch.exp(feat / temp).t()
    n, k = q.shape[1], q.shape[0]
    q = q / q.sum()
    for _ in range(num_iter):
        q = q / q.sum(dim=1, keepdim=True) / k
        q = q / q.sum(dim=0, keepdim=True) / n
    q = q * n
    return q.t()


def pair_loss(target, student, tau):
    return -torch.sum(target * torch.log_softmax(student / tau, dim=-1), dim=-1)


def scene_mean(values, scene):
    """per-scene means over scene ids 0 .. scene.max(); an empty scene in between is 0"""
    size = int(scene.max()) + 1
    total = torch.zeros(size, dtype=values.dtype, device=values.device).index_add_(0, scene, values)
    count = torch.zeros(size, dtype=values.dtype, device=values.device).index_add_(0, scene, torch.ones_like(values))
    return total / count.clamp(min=1), count


def scene_of(rows, offset):
    """scene id of student rows under cumulative ends `offset`"""
    return torch.bucketize(rows, offset.to(rows.device), right=True)


def loss(x, idx_t, s, idx_s, offset_s, temp, tau):
    """the scalar loss of one pairing, its (M, K) target, and the per-pair losses"""
    if idx_t.numel() == 0:
        return x.new_zeros(()), x.new_zeros((0, x.shape[1])), x.new_zeros((0,))
    target = sinkhorn_knopp(x[idx_t], temp)
    per_pair = pair_loss(target, s[idx_s], tau)
    means, _ = scene_mean(per_pair, scene_of(idx_s, offset_s))
    return means.mean(), target, per_pair


def sweeps(x, idx_t, temp, n_total=None):
    """([(A_i, u_i)] for i = 1, 2, 3, d_3) in the notation of DESIGN.md section 25, read off the LITERAL iteration, so that
    one kernel sweep can be checked on its own and a float32 run of this function carries the literal formulation's
    float32 error.  With E = exp(x[idx_t] / temp): the literal matrix is E u_{i-1} / (n d_{i-1}) before the i-th row
    normalisation (E / total for i = 1), so its row sum is R_i = u_{i-1} A_i with A_i = sum_m E / (n d_{i-1}), hence
    u_i = u_{i-1} / (K R_i) from u_0 = 1 / total and A_i = 1 / (K u_i); its column sum after that normalisation is
    c_i = d_i / (n d_{i-1}) (d_1 itself for i = 1), hence d_i = c_i n d_{i-1}."""
    q = torch.exp(x[idx_t] / temp).t()
    n = q.shape[1] if n_total is None else n_total
    k = q.shape[0]
    total = q.sum()
    q = q / total
    u, d, out = 1.0 / total, None, []
    for i in range(3):
        r = q.sum(dim=1, keepdim=True)
        u = u / (k * r[:, 0])
        out.append((1.0 / (k * u), u))
        q = q / r / k
        c = q.sum(dim=0, keepdim=True)
        d = c[0] if i == 0 else c[0] * n * d
        q = q / c / n
    return out, d


def pair_stats(x, idx_t, s, idx_s, temp, tau):
    """(d, lse) per pair as the kernels hand them to the backward: d = E u_3, lse = logsumexp(s / tau)"""
    _, d = sweeps(x, idx_t, temp)
    return d, torch.logsumexp(s[idx_s] / tau, dim=-1)


def dstudent(x, idx_t, s, idx_s, offset_s, temp, tau, dloss=1.0):
    """(Ns, K) gradient of `loss` to the student logits; zeros in unmatched rows"""
    ds = torch.zeros_like(s)
    if idx_t.numel() == 0:
        return ds
    target = sinkhorn_knopp(x[idx_t], temp)
    scene = scene_of(idx_s, offset_s)
    _, count = scene_mean(torch.ones_like(target[:, 0]), scene)
    g = dloss / (count[scene] * count.shape[0])
    p = torch.softmax(s[idx_s] / tau, dim=-1)
    ds[idx_s] = g[:, None] * (p * target.sum(1, keepdim=True) - target) / tau
    return ds
