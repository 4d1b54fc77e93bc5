"""Yardstick of Concerto's image branch (csrc/concerto.hip, pointcept/models/concerto): the reference's literal formulation
(pointcept/models/concerto/concerto_v1m1_base.py:545-570 and :786-842) restated in plain torch, in whatever dtype and on
whatever device its inputs have - float64 on the CPU is the yardstick, float32 on the device the run whose error sets the
kernels' bound.
  segment_sum      torch_scatter.segment_csr(reduce="sum") as documented
  pool_level       one level of pool_corr: the children sorted by cluster, per image the count of the children with both
                   entries set (0 -> 100000), the sums with every -1 entry set to 0, the quotient, -1 where nothing counted
  pool_corr        the levels from fine to coarse
  feature_index    the valid (row, view) pairs (ANY entry != -1) and the dense patch index of each
  patch_mean_dense scatter_mean of the gathered rows into ALL images * patch_h * patch_w rows (zeros where empty)
  cos_loss         the shift over the channels, CosineSimilarity(dim=1, eps=1e-6), 10 * mean(1 - cos)
  enc2d_loss       gather, dense scatter_mean, the projection over every row, the select of the occupied rows, the loss
"""
import torch


def segment_sum(src, idx_ptr):
    idx_ptr = idx_ptr.long()
    seg = torch.repeat_interleave(torch.arange(idx_ptr.shape[0] - 1, device=src.device), idx_ptr[1:] - idx_ptr[:-1])
    return torch.zeros((idx_ptr.shape[0] - 1,) + src.shape[1:], dtype=src.dtype, device=src.device).index_add_(0, seg, src)


def pool_level(corr, inverse, idx_ptr):
    """(n_in, V, 2) -> (n_out, V, 2)"""
    n_out = idx_ptr.shape[0] - 1
    if corr.shape[1] == 0:
        return -torch.ones((n_out, 0, 2), dtype=corr.dtype, device=corr.device)
    _, indices = torch.sort(inverse, stable=True)
    minus = torch.full((2,), -1, dtype=corr.dtype, device=corr.device)
    out = []
    for image in range(corr.shape[1]):
        both = torch.all(corr[:, image] != minus, dim=1).to(corr.dtype)
        counts = segment_sum(both[indices], idx_ptr)
        counts[counts == 0] = 100000
        filled = corr[:, image].clone()
        filled[filled == -1] = 0
        mean = segment_sum(filled[indices], idx_ptr) / counts.unsqueeze(1)
        mean[counts == 100000] = -1
        out.append(mean)
    return torch.stack(out, dim=1)


def pool_corr(corr, levels):
    """levels: (inverse, idx_ptr) of every pooling, fine to coarse"""
    for inverse, idx_ptr in levels:
        corr = pool_level(corr, inverse, idx_ptr)
    return corr


def feature_index(corr, rows, scene, img_num, patch_h, patch_w):
    """(r, v, index): the pairs with ANY entry != -1 among corr[rows] in (row, view) order, and the patch of each"""
    sub = corr[rows]
    minus = torch.full((2,), -1, dtype=corr.dtype, device=corr.device)
    r, v = torch.where(torch.any(sub != minus, dim=2))
    base = (torch.cumsum(img_num, 0) - img_num).to(corr.device)[scene[r]]
    c = sub[r, v].long()
    index = base * patch_h * patch_w + v * patch_h * patch_w + c[:, 0] * patch_w + c[:, 1]
    return r, v, index


def patch_mean_dense(gathered, index, n_patches):
    total = torch.zeros((n_patches, gathered.shape[1]), dtype=gathered.dtype, device=gathered.device).index_add_(0, index, gathered)
    count = torch.zeros(n_patches, dtype=gathered.dtype, device=gathered.device).index_add_(
        0, index, torch.ones(index.shape[0], dtype=gathered.dtype, device=gathered.device))
    return total / count.clamp(min=1).unsqueeze(1)


def cosines(a, b, shift=True):
    """cos per row of b (the encoder's rows) against a (the projected rows)"""
    if shift:
        b = b - b.mean(dim=-1, keepdim=True)
        a = a - a.mean(dim=-1, keepdim=True)
    return torch.nn.CosineSimilarity(dim=1, eps=1e-6)(b, a)


def cos_loss(a, b, shift=True):
    return (1 - cosines(a, b, shift)).mean() * 10


def enc2d_loss(feat, corr, rows, scene, feature2d, weight, bias, img_num, patch_h, patch_w, shift=True):
    """dict(loss, patch_ids, patch_mean (U, C), projected (U, D), encoder_rows (U, D)) by the dense formulation"""
    r, _, index = feature_index(corr, rows, scene, img_num, patch_h, patch_w)
    dense = patch_mean_dense(feat[rows][r], index, feature2d.shape[0])
    projected = torch.nn.functional.linear(dense, weight, bias)
    patch_ids = torch.unique(index)
    a, b = projected[patch_ids], feature2d[patch_ids]
    return dict(loss=cos_loss(a, b, shift), patch_ids=patch_ids, patch_mean=dense[patch_ids], projected=a, encoder_rows=b)
