"""ptv3_res_conv at a row count that selects the two-row-tile kernels (128-point workgroups), which the 306-site cases of
test_hip_res_conv.py never reach: 70 000 seeded sites of a 60^3 box (the switch is at 65 409 rows for one column block).

Every row of every case is judged by `_within_4x` against a float64 gather composition (evaluated on the device, in row
chunks), twice: with fp32 torch on the device as the yardstick, as in test_hip_res_conv.py, and with the library's own
ops (ptv3_gemm, the table-free ptv3_gemm for the projection, ptv3_add_act) as the yardstick - the path the kernel
replaces in the model.
The last test runs the default-wired BasicBlocks of the fork config's finest level at this size: res_conv_wired is True
there and the blocks call ops.res_conv."""
import numpy as np
import pytest
import torch

from test_hip_keypoint_oacnns import _within_4x, FP32_TOL

pytestmark = pytest.mark.gpu

ROWS = 70000
# (ca, cb, cout, projection, residual): the two shapes the model wires, one 128-wide and one 64-wide column block
CASES = [(96, 32, 96, True, False), (96, 0, 96, False, True), (64, 64, 128, True, True), (32, 32, 64, True, True)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


_SITES = {}


def _sites(dev):
    from ptv3_hip import ops
    if not _SITES:
        rs = np.random.RandomState(5)
        cells = rs.permutation(60 ** 3)[:ROWS]
        xyz = np.stack([cells // 3600, cells // 60 % 60, cells % 60], axis=1) + 2
        idx = torch.from_numpy(np.concatenate([np.zeros((ROWS, 1), dtype=np.int64), xyz], axis=1)).int().to(dev)
        nbr = ops.subm_neighbors(idx, 3)[0]
        _SITES.update(idx=idx, nbr=nbr)
    return _SITES["idx"], _SITES["nbr"]


def _compose(x, w, wp, nbr, vec, res, chunk=10000):
    """relu(conv * s + t (+ res)) and projection * s + t for all rows, in x's dtype on x's device, `chunk` rows at a time"""
    m, cin = x.shape
    pad = torch.cat([x, x.new_zeros(1, cin)])
    wm = w.reshape(w.shape[0], -1).T.contiguous()
    outs = []
    for r0 in range(0, m, chunk):
        nb = nbr[r0:r0 + chunk]
        g = pad[torch.where(nb >= 0, nb, m).long().reshape(-1)].view(nb.shape[0], 27 * cin)
        out = g @ wm * vec[0] + vec[1]
        if res is not None:
            out = out + res[r0:r0 + chunk]
        outs.append(torch.relu(out))
    return torch.cat(outs), x @ wp.T * vec[2] + vec[3]


@pytest.mark.parametrize("ca,cb,cout,with_proj,with_res", CASES)
def test_two_row_tiles(dev, ca, cb, cout, with_proj, with_res):
    from ptv3_hip import ops
    idx, nbr = _sites(dev)
    assert ops.res_conv_row_tiles(ROWS, cout) == 2 and ops.res_conv_row_tiles(306, cout) == 1
    assert ops.res_conv_capable(ROWS, ca, cb, cout)
    cin = ca + cb
    gen = torch.Generator().manual_seed(100 * ca + cb + cout)
    x = torch.randn(ROWS, cin, generator=gen).to(dev)
    res = torch.randn(ROWS, cout, generator=gen).to(dev)
    w = (torch.randn(cout, 27, cin, generator=gen) / (27 * cin) ** 0.5).to(dev)
    wp = (torch.randn(cout, cin, generator=gen) / cin ** 0.5).to(dev)
    vec = [(torch.rand(cout, generator=gen) + 0.5).to(dev), (torch.randn(cout, generator=gen) * 0.3).to(dev),
           (torch.rand(cout, generator=gen) + 0.5).to(dev), (torch.randn(cout, generator=gen) * 0.3).to(dev)]
    xa, xb = x[:, :ca].contiguous(), (x[:, ca:].contiguous() if cb else None)
    kw = dict(xb=xb, bn_scale=vec[0], bn_shift=vec[1], res=res if with_res else None, act=ops.ACT_RELU)
    if with_proj:
        kw.update(w_proj=wp, proj_scale=vec[2], proj_shift=vec[3])
    got = ops.res_conv(xa, w, nbr, **kw)
    out, proj = got if with_proj else (got, None)

    # the path the kernel replaces
    y = ops.gemm(x, w.reshape(cout, -1), nbr=nbr, kvol=27, bn_scale=vec[0], bn_shift=vec[1],
                 act=ops.ACT_NONE if with_res else ops.ACT_RELU)
    plain = ops.add_act(y, res, ops.ACT_RELU) if with_res else y
    ref, pref = _compose(x.double(), w.double(), wp.double(), nbr, [v.double() for v in vec],
                         res.double() if with_res else None)
    base, pbase = _compose(x, w, wp, nbr, vec, res if with_res else None)
    what = f"{ca}+{cb}->{cout} rows={ROWS}"
    _within_4x(out, base, ref, what + " vs torch fp32")
    _within_4x(out, plain, ref, what + " vs ptv3_gemm path")
    if with_proj:
        _within_4x(proj, pbase, pref, what + " [proj] vs torch fp32")
        _within_4x(proj, ops.gemm(x, wp, bn_scale=vec[2], bn_shift=vec[3]), pref, what + " [proj] vs ptv3_gemm")


def test_default_wiring_calls_the_kernel(dev, monkeypatch):
    """The finest decoder stage of the fork config (a 96+32 -> 96 front and a 96 -> 96 block) at 70 000 sites:
    res_conv_wired says yes, the default-wired blocks run ops.res_conv (2 + 1 launches), and their output agrees with
    the same blocks on ptv3_gemm + cat + add_act within the fp32 budget of the model tests."""
    from functools import partial
    from ptv3_hip import ops
    from pointcept.models.sparse_unet.spconv_unet_v1m1_base import BasicBlock, res_conv_wired
    from pointcept.models.utils.hip_layers import BatchNorm1d
    from pointcept.models.utils.sparse import SparseConvTensor
    idx, nbr = _sites(dev)
    assert res_conv_wired(ROWS, 96, 32, 96) and res_conv_wired(ROWS, 96, 0, 96)
    assert not res_conv_wired(ROWS, 32, 0, 32) and not res_conv_wired(6000, 96, 32, 96)     # unwired; K would be split
    torch.manual_seed(11)
    norm_fn = partial(BatchNorm1d, eps=1e-3, momentum=0.01)
    blocks = [BasicBlock(128, 96, norm_fn=norm_fn, indice_key="subm0").to(dev).eval(),
              BasicBlock(96, 96, norm_fn=norm_fn, indice_key="subm0").to(dev).eval()]
    for b in blocks:
        for m in b.modules():
            if isinstance(m, BatchNorm1d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.data.normal_(1, 0.1)
                m.bias.data.normal_(0, 0.1)
            elif hasattr(m, "weight") and m.weight.dim() == 5:
                m.weight.data.normal_(0, (1.0 / m.weight[0].numel()) ** 0.5)
    up, skip = torch.randn(ROWS, 96, device=dev), torch.randn(ROWS, 32, device=dev)

    def run():
        x = SparseConvTensor(up, idx, [64, 64, 64], 1)
        with torch.no_grad():
            return blocks[1](blocks[0](x, skip)).features
    calls, inner = [], ops.res_conv

    def counting(*a, **k):
        calls.append(ops.res_conv_row_tiles(a[0].shape[0], a[1].shape[0]))
        return inner(*a, **k)
    monkeypatch.setattr(ops, "res_conv", counting)
    wired = run()
    assert calls == [2, 2, 2], calls            # front (conv1 + proj), its tail, the plain block's tail: two row tiles each
    del calls[:]
    for b in blocks:
        b.res_conv = False
    plain = run()
    assert not calls
    err, scale = (wired - plain).abs().max().item(), plain.abs().max().item()
    print(f"default wiring - parent ops {err:.3e} at scale {scale:.3e}")
    assert err < FP32_TOL * scale
