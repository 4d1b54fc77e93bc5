"""ptv3_res_conv on the GPU against a float64 gather composition written here.

Sites: one seeded set of 300 voxels of a 10^3 box plus six isolated voxels whose only neighbour is themselves; the
neighbour table comes from ops.subm_neighbors.  Every result is judged by `_within_4x` of test_hip_keypoint_oacnns.py:
its distance to the float64 composition is at most 4x the distance of the same composition evaluated by torch in fp32 on
the device (and never needs to beat one fp32 rounding)."""
import itertools

import numpy as np
import pytest
import torch

from test_hip_keypoint_oacnns import _within_4x

pytestmark = pytest.mark.gpu

CASES = [(16, 0, 16), (32, 0, 32), (96, 0, 96), (96, 32, 96), (128, 64, 128), (256, 128, 256), (4, 4, 8),
         (16, 16, 16),   # one 16-wide column block, the projection and more than 16 K steps together
         (32, 32, 64)]   # the 64-wide column block, which none of the cases above takes
N_BOX, N_ISOLATED = 300, 6
CENTRE = 13


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


_SITES = {}


def _sites(dev, rows=None):
    """(indices (m, 4) int32 on the device, nbr (m, 27)) of the first `rows` sites; the isolated voxels come first, so
    every row count holds some.  Built once per row count."""
    from ptv3_hip import ops
    if "all" not in _SITES:
        rs = np.random.RandomState(17)
        cells = rs.permutation(1000)[:N_BOX]
        box = np.stack([cells // 100, cells // 10 % 10, cells % 10], axis=1) + 3
        lone = np.stack([20 + 3 * np.arange(N_ISOLATED), np.full(N_ISOLATED, 40), np.full(N_ISOLATED, 7)], axis=1)
        rest = np.concatenate([lone[1:], box])[rs.permutation(N_BOX + N_ISOLATED - 1)]
        xyz = np.concatenate([lone[:1], rest])                      # row 0 is isolated: the one-row case
        _SITES["all"] = np.concatenate([np.zeros((len(xyz), 1), dtype=np.int64), xyz], axis=1)
        _SITES["lone"] = {tuple(v) for v in lone.tolist()}
    m = len(_SITES["all"]) if rows is None else rows
    if m not in _SITES:
        idx = torch.from_numpy(_SITES["all"][:m]).int().to(dev)
        nbr = ops.subm_neighbors(idx, 3)[0]
        lone = torch.tensor([tuple(v) in _SITES["lone"] for v in _SITES["all"][:m, 1:].tolist()])
        host = nbr.cpu()
        assert torch.equal(host[:, CENTRE], torch.arange(m, dtype=torch.int32))
        assert ((host[lone] >= 0).sum(1) == 1).all() and lone.sum() >= 1
        _SITES[m] = (idx, nbr, lone)
    return _SITES[m]


def _operands(ca, cb, cout, m):
    gen = torch.Generator().manual_seed(1000 * ca + 10 * cb + cout)
    cin = ca + cb
    x = torch.randn(N_BOX + N_ISOLATED, cin, generator=gen)[:m]
    res = torch.randn(N_BOX + N_ISOLATED, cout, generator=gen)[:m]
    w = torch.randn(cout, 27, cin, generator=gen) / (27 * cin) ** 0.5
    wp = torch.randn(cout, cin, generator=gen) / cin ** 0.5
    vec = [torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.3,
           torch.rand(cout, generator=gen) + 0.5, torch.randn(cout, generator=gen) * 0.3]
    return x.contiguous(), res.contiguous(), w, wp, vec


def _raw(x, w, wp, nbr):
    """(conv sums (m, cout), projection sums (m, cout)) of the gather composition in x's dtype, on x's device"""
    m, cin = x.shape
    idx = torch.where(nbr >= 0, nbr, m).long().to(x.device)
    rows = torch.cat([x, x.new_zeros(1, cin)])[idx.reshape(-1)].view(m, 27 * cin)
    return rows @ w.reshape(w.shape[0], -1).T, x @ wp.T


def _finish(y, p, vec, res, relu):
    out = y * vec[0] + vec[1]
    if res is not None:
        out = out + res
    return (torch.relu(out) if relu else out), p * vec[2] + vec[3]


def _run(dev, ca, cb, cout, m, nbr, ops_kw, with_res, with_proj, relu, order=None):
    from ptv3_hip import ops
    x, res, w, wp, vec = ops_kw
    xd = x.to(dev)
    xa = xd[:, :ca].contiguous()
    xb = xd[:, ca:].contiguous() if cb else None
    kw = dict(xb=xb, bn_scale=vec[0].to(dev), bn_shift=vec[1].to(dev), res=res.to(dev) if with_res else None,
              act=ops.ACT_RELU if relu else ops.ACT_NONE, row_order=order)
    if with_proj:
        kw.update(w_proj=wp.to(dev), proj_scale=vec[2].to(dev), proj_shift=vec[3].to(dev))
    got = ops.res_conv(xa, w.to(dev), nbr, **kw)
    return got if with_proj else (got, None)


@pytest.mark.parametrize("ca,cb,cout", CASES)
def test_epilogue_grid(dev, ca, cb, cout):
    """{res, no res} x {proj, no proj} x {ReLU, none} on all rows; one float64 and one fp32 composition per case."""
    from ptv3_hip import ops
    assert ops.res_conv_capable(N_BOX + N_ISOLATED, ca, cb, cout)
    idx, nbr, lone = _sites(dev)
    m = idx.shape[0]
    opd = _operands(ca, cb, cout, m)
    x, res, w, wp, vec = opd
    y64, p64 = _raw(x.double(), w.double(), wp.double(), nbr.cpu())
    y32, p32 = _raw(x.to(dev), w.to(dev), wp.to(dev), nbr)
    v64, vd = [v.double() for v in vec], [v.to(dev) for v in vec]
    for with_res, with_proj, relu in itertools.product((True, False), repeat=3):
        out, proj = _run(dev, ca, cb, cout, m, nbr, opd, with_res, with_proj, relu)
        ref, pref = _finish(y64, p64, v64, res.double() if with_res else None, relu)
        base, pbase = _finish(y32, p32, vd, res.to(dev) if with_res else None, relu)
        what = f"{ca}+{cb}->{cout} res={with_res} proj={with_proj} relu={relu}"
        _within_4x(out, base, ref, what)
        if with_proj:
            _within_4x(proj, pbase, pref, what + " [proj]")
            both = x.to(dev)
            plain = ops.gemm(both, wp.to(dev), bn_scale=vd[2], bn_shift=vd[3])
            _within_4x(proj, plain, pref, what + " [proj vs ops.gemm]")
    # an isolated site's output is its centre tap alone
    out, _ = _run(dev, ca, cb, cout, m, nbr, opd, False, False, False)
    centre = (x.double() @ w[:, CENTRE].double().T) * v64[0] + v64[1]
    centre32 = (x.to(dev) @ w[:, CENTRE].to(dev).T) * vd[0] + vd[1]
    _within_4x(out[lone.to(dev)], centre32[lone.to(dev)], centre[lone], f"{ca}+{cb}->{cout} isolated sites")


@pytest.mark.parametrize("ca,cb,cout", CASES)
def test_row_counts_and_row_order(dev, ca, cb, cout):
    """1, 63, 64, 65 and all rows (partial and multiple tiles), each with and without row_order, with residual,
    projection and ReLU; row_order changes which tile a row sits in, not its value."""
    for rows in (1, 63, 64, 65, None):
        idx, nbr, _ = _sites(dev, rows)
        m = idx.shape[0]
        opd = _operands(ca, cb, cout, m)
        x, res, w, wp, vec = opd
        ref, pref = _finish(*_raw(x.double(), w.double(), wp.double(), nbr.cpu()), [v.double() for v in vec],
                            res.double(), True)
        base, pbase = _finish(*_raw(x.to(dev), w.to(dev), wp.to(dev), nbr), [v.to(dev) for v in vec], res.to(dev), True)
        order = torch.from_numpy(np.random.RandomState(m).permutation(m)).int().to(dev)
        plain = _run(dev, ca, cb, cout, m, nbr, opd, True, True, True)
        moved = _run(dev, ca, cb, cout, m, nbr, opd, True, True, True, order=order)
        for tag, (out, proj) in (("", plain), (" row_order", moved)):
            _within_4x(out, base, ref, f"{ca}+{cb}->{cout} m={m}{tag}")
            _within_4x(proj, pbase, pref, f"{ca}+{cb}->{cout} m={m}{tag} [proj]")
        assert torch.equal(plain[0], moved[0]) and torch.equal(plain[1], moved[1])


def test_residual_is_added_before_the_relu(dev):
    """A negative pre-activation that the residual lifts above zero survives: relu(y + res), not relu(y) + res."""
    ca, cb, cout = 32, 0, 32
    idx, nbr, _ = _sites(dev)
    m = idx.shape[0]
    x, res, w, wp, vec = _operands(ca, cb, cout, m)
    res = torch.full_like(res, 10.0)
    y64, _ = _raw(x.double(), w.double(), wp.double(), nbr.cpu())
    pre = y64 * vec[0].double() + vec[1].double()
    lifted = pre < -0.1
    assert lifted.sum() > 100 and (pre > -9.0).all()
    out, _ = _run(dev, ca, cb, cout, m, nbr, (x, res, w, wp, vec), True, False, True)
    out = out.double().cpu()
    assert (out[lifted] < 9.95).all()                                   # relu(y) + res would be exactly 10 there
    assert (out - (pre + 10.0)).abs().max().item() < 1e-4


def test_capable_and_entry_agree(dev):
    """A shape reported as 0 is refused with a message and not run; a shape reported as 1 runs."""
    from ptv3_hip import ops
    idx, nbr, _ = _sites(dev, 64)
    for ca, cb, cout in ((16, 0, 516), (1024, 4, 16), (16, 0, 16)):
        capable = ops.res_conv_capable(64, ca, cb, cout)
        xa = torch.zeros(64, ca, device=dev)
        xb = torch.zeros(64, cb, device=dev) if cb else None
        w = torch.zeros(cout, 27, ca + cb, device=dev)
        if capable:
            assert tuple(ops.res_conv(xa, w, nbr, xb=xb).shape) == (64, cout)
        else:
            with pytest.raises(RuntimeError, match="not served"):
                ops.res_conv(xa, w, nbr, xb=xb)
    assert not ops.res_conv_capable(64, 16, 0, 16, kvol=125)
    nbr5 = ops.subm_neighbors(idx, 5)[0]
    with pytest.raises(RuntimeError, match="kvol=125"):
        ops.res_conv(torch.zeros(64, 16, device=dev), torch.zeros(16, 125, 16, device=dev), nbr5)
    torch.cuda.synchronize()
