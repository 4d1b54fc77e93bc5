"""Plain statement of the weight-gradient GEMM ptv3_gemm_tn (csrc/backward.hip), shared by
tests/test_gemm_tn_reference_cpu.py (which holds it to torch autograd of oracle.ptv3.subm_conv3d / F.linear) and
tests/test_hip_gemm_tn.py (which holds the kernel to it)."""
import torch


def ref_gemm_tn(dy, x, nbr=None):
    """-> (dw (cout, kvol*cin), db (cout)), in int64 for integer inputs and in float64 otherwise:
    dw[o, t*cin + c] = sum over rows i with nbr[i, t] >= 0 of dy[i, o] * x[nbr[i, t], c]   (nbr None: dy^T x),
    db[o] = sum_i dy[i, o].  Columns of a tap that no row has stay zero."""
    acc = torch.float64 if dy.is_floating_point() else torch.int64
    dy, x = dy.detach().cpu().to(acc), x.detach().cpu().to(acc)
    cout, cin = dy.shape[1], x.shape[1]
    if nbr is None:
        return dy.t() @ x, dy.sum(0)
    nbr = nbr.detach().cpu().long()
    kvol = nbr.shape[1]
    dw = torch.zeros(cout, kvol, cin, dtype=acc)
    for t in range(kvol):
        rows = torch.nonzero(nbr[:, t] >= 0)[:, 0]
        if rows.numel():
            dw[:, t] = dy[rows].t() @ x[nbr[rows, t]]
    return dw.reshape(cout, kvol * cin), dy.sum(0)


def synth_nbr(m, kvol, gen, absent_tap=None):
    """(m, kvol) int32 neighbour table for the kernel alone: random rows in [0, m), about half the entries absent (-1)
    and tap `absent_tap` (default: the middle one) absent for every row.  Not symmetric: gemm_tn does not need that."""
    nbr = torch.randint(0, m, (m, kvol), generator=gen, dtype=torch.int32)
    nbr[torch.rand(m, kvol, generator=gen) < 0.5] = -1
    nbr[:, kvol // 2 if absent_tap is None else absent_tap] = -1
    return nbr
