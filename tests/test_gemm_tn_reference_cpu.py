"""CPU checks of tests/gemm_tn_ref.py, the statement tests/test_hip_gemm_tn.py holds ptv3_gemm_tn to: against float64
torch autograd of oracle.ptv3.subm_conv3d (neighbour table by dictionary lookup, tap d = (a k + b) k + c as in
test_subm_conv_vs_oracle) and of F.linear.  This pins the (cout, tap, cin) layout the GPU tests rely on."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_tn_ref import ref_gemm_tn, synth_nbr  # noqa: E402

F = torch.nn.functional


def _dict_neighbors(indices, k):
    sites = {tuple(r): i for i, r in enumerate(indices.tolist())}
    nbr = torch.full((indices.shape[0], k ** 3), -1, dtype=torch.int32)
    for i, (bb, x, y, z) in enumerate(indices.tolist()):
        for d in range(k ** 3):
            a, b_, c = d // (k * k) - k // 2, (d // k) % k - k // 2, d % k - k // 2
            nbr[i, d] = sites.get((bb, x + a, y + b_, z + c), -1)
    return nbr


@pytest.mark.parametrize("k,sizes,seed", [(3, [600, 300], 0), (5, [250, 150], 1)])
def test_reference_matches_autograd_of_the_oracle_conv(k, sizes, seed):
    from oracle import ptv3 as O
    import ptv3_scenes as S
    cin, cout = 8, 20
    data = S.make_batch(sizes, in_channels=cin, extent=40, seed=seed)
    gc, off = data["grid_coord"], data["offset"]
    n = gc.shape[0]
    batch = torch.repeat_interleave(torch.arange(2), torch.diff(off, prepend=torch.zeros(1, dtype=torch.long)))
    indices = torch.cat([batch[:, None], gc], 1).int()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, generator=g, dtype=torch.float64)
    w = torch.randn(cout, k, k, k, cin, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(cout, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(n, cout, generator=g, dtype=torch.float64)
    O.subm_conv3d(x, indices, w, b).backward(dy)
    nbr = _dict_neighbors(indices, k)
    absent = (nbr < 0).float().mean().item()
    assert 0.3 < absent < 1.0 and (nbr[:, k ** 3 // 2] == torch.arange(n)).all()   # a real table: holes, centre = self
    dw, db = ref_gemm_tn(dy, x, nbr)
    assert dw.dtype == torch.float64 and dw.shape == (cout, k ** 3 * cin) and db.shape == (cout,)
    # both sides are float64 sums of <= n products of N(0, 1) pairs in different orders
    assert (dw.reshape(w.shape) - w.grad).abs().max().item() < 1e-12
    assert (db - b.grad).abs().max().item() < 1e-12


def test_reference_matches_autograd_of_linear():
    g = torch.Generator().manual_seed(2)
    m, cin, cout = 300, 6, 13
    x = torch.randn(m, cin, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(cout, generator=g, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(m, cout, generator=g, dtype=torch.float64)
    F.linear(x, w, b).backward(dy)
    dw, db = ref_gemm_tn(dy, x)
    assert dw.shape == (cout, cin)
    assert (dw - w.grad).abs().max().item() < 1e-12 and (db - b.grad).abs().max().item() < 1e-12


def test_reference_on_integers_is_int64_and_agrees_with_the_float64_form():
    g = torch.Generator().manual_seed(3)
    m, cin, cout, kvol = 257, 4, 8, 27
    dy = torch.randint(-3, 4, (m, cout), generator=g)
    x = torch.randint(-3, 4, (m, cin), generator=g)
    nbr = synth_nbr(m, kvol, g)
    assert (nbr[:, kvol // 2] == -1).all() and 0.4 < (nbr < 0).float().mean().item() < 0.65
    dw, db = ref_gemm_tn(dy, x, nbr)
    assert dw.dtype == torch.int64 and db.dtype == torch.int64
    dwf, dbf = ref_gemm_tn(dy.double(), x.double(), nbr)
    assert torch.equal(dw.double(), dwf) and torch.equal(db.double(), dbf)
    assert (dw.view(cout, kvol, cin)[:, kvol // 2] == 0).all() and dw.abs().max() > 0
    # one entry by hand
    o, t, c = 5, 3, 2
    want = sum(int(dy[i, o]) * int(x[nbr[i, t], c]) for i in range(m) if nbr[i, t] >= 0)
    assert int(dw[o, t * cin + c]) == want
