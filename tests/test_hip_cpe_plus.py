"""The two bottleneck-CPE kernels of PT-v3m1-Plus on the GPU (csrc/cpe_plus.hip): ptv3_subm_conv_ln and
ptv3_rows_linear_ln against the float64 statements of tests/cpe_plus_ref.py.

Accuracy rule (the convention of test_hip_keypoint_oacnns.py): the kernel's largest error against
float64 is at most 4x the largest error of the existing composition in the same dtype (ptv3_gemm -> ptv3_layernorm ->
ReLU) against float64, both measured here on inputs already rounded to that dtype.  The bound never falls under one
rounding of the output dtype at the output's scale (finfo(dtype).eps * max|ref|), which no result in that dtype can
beat.  Exact cases: zero input, run-to-run bits, refused shapes."""
import pytest
import torch

from cpe_plus_ref import ref_subm_conv_ln, ref_rows_linear_ln

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _within_4x(got, comp, ref, what):
    err = (got.double().cpu() - ref).abs().max().item()
    base = (comp.double().cpu() - ref).abs().max().item()
    floor = torch.finfo(got.dtype).eps * ref.abs().max().item()
    print(f"{what}: kernel error {err:.3e}, composition error {base:.3e}, floor {floor:.3e}")
    assert err <= max(4 * base, floor), (what, err, base, floor)


# ------------------------------------------------------------------------------------------------
# site sets: (n, 4) int32 [batch, x, y, z], built once; neighbour tables per (set, kernel size) on the device
# ------------------------------------------------------------------------------------------------
_SITES, _NBR = {}, {}


def _site_sets():
    if not _SITES:
        g = torch.Generator().manual_seed(24)
        r = torch.arange(7)
        cube = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3) + 3
        cells = torch.nonzero(torch.rand(24, 24, 24, generator=g) < 0.03)
        cells = cells[torch.randperm(cells.shape[0], generator=g)]          # no spatial order in the row order
        assert 257 <= cells.shape[0] <= 600

        def with_batch(xyz, b=0):
            return torch.cat([torch.full((xyz.shape[0], 1), b), xyz], 1).int()

        _SITES["cube7"] = with_batch(cube)
        _SITES["scatter"] = with_batch(cells)
        _SITES["two_scenes"] = torch.cat([with_batch(cells[:150], 0), with_batch(cells[:150], 1)])
        _SITES["lone"] = with_batch(torch.tensor([[5, 6, 7]]))
        for m in (1, 63, 64, 65, 257):
            _SITES[f"scatter[:{m}]"] = with_batch(cells[:m])
    return _SITES


def _nbr(dev, name, ksize):
    from ptv3_hip import ops
    key = (name, ksize)
    if key not in _NBR:
        sites = _site_sets()[name].to(dev)
        nbr, _ = ops.subm_neighbors(sites, ksize)
        host = nbr.cpu()
        kvol, n = ksize ** 3, sites.shape[0]
        assert (host[:, kvol // 2] == torch.arange(n, dtype=torch.int32)).all()   # the centre tap is the site itself
        if name == "cube7":
            assert (host >= 0).all(1).any() if ksize == 3 else (host >= 0).all(1).sum() == 27
        if name == "lone":
            assert (host >= 0).sum() == 1
        if name == "two_scenes":      # no tap crosses from one scene to the other
            hit = host >= 0
            src_scene = (torch.arange(n) >= 150).view(-1, 1).expand_as(host)
            assert ((host >= 150) == src_scene)[hit].all()
        if name == "scatter":
            assert (host >= 0).float().mean() < 0.1
        _NBR[key] = nbr
    return _NBR[key]


def _conv_inputs(m, c, kvol, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, c, generator=g).to(dtype).to(dev)
    w = (torch.randn(c, kvol, c, generator=g) / (c * min(kvol, 8)) ** 0.5).to(dtype).to(dev)
    bias = (0.2 * torch.randn(c, generator=g)).to(dev)
    gamma = (1 + 0.2 * torch.randn(c, generator=g)).to(dev)
    beta = (0.3 * torch.randn(c, generator=g)).to(dev)
    return x, w, bias, gamma, beta


def _conv_composition(x, w, nbr, bias, gamma, beta, row_order):
    from ptv3_hip import ops
    kvol = nbr.shape[1]
    y = ops.gemm(x, w.reshape(w.shape[0], -1), bias=bias, nbr=nbr, kvol=kvol, row_order=row_order)
    return ops.affine_act(ops.layernorm(y, gamma, beta, EPS), None, None, ops.ACT_RELU)


@pytest.mark.parametrize("ordered", [False, True], ids=["natural", "row_order"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("kvol", [27, 125])
@pytest.mark.parametrize("c", [16, 32, 64, 128])
def test_subm_conv_ln_vs_float64(dev, c, kvol, dtype, ordered):
    from ptv3_hip import ops
    assert ops.subm_conv_ln_capable(c, kvol, dtype)
    ksize = round(kvol ** (1 / 3))
    for si, (name, sites) in enumerate(_site_sets().items()):
        m = sites.shape[0]
        nbr = _nbr(dev, name, ksize)
        x, w, bias, gamma, beta = _conv_inputs(m, c, kvol, dtype, dev, seed=1000 * c + kvol + si)
        row_order = None
        if ordered:
            row_order = torch.randperm(m, generator=torch.Generator().manual_seed(si)).int().to(dev)
        got = ops.subm_conv_ln(x, w, nbr, bias, gamma, beta, EPS, ops.ACT_RELU, row_order=row_order)
        ref = ref_subm_conv_ln(x, w, nbr, bias, gamma, beta, EPS)
        comp = _conv_composition(x, w, nbr, bias, gamma, beta, row_order)
        _within_4x(got, comp, ref, f"subm_conv_ln c={c} kvol={kvol} {dtype} {name}")
        again = ops.subm_conv_ln(x, w, nbr, bias, gamma, beta, EPS, ops.ACT_RELU, row_order=row_order)
        assert torch.equal(got, again), "two calls must give identical bits"


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("c,kvol", [(16, 125), (32, 125), (128, 27)])
def test_subm_conv_ln_two_row_tiles_per_wave(dev, c, kvol, dtype):
    """From 32768 rows on a wave carries two row tiles (the other instantiation of the kernel): a 40^3 box at 55 %
    occupancy, one row short of a tile multiple; float64 on a sample of the rows (every row's bits against a rerun)."""
    from ptv3_hip import ops
    g = torch.Generator().manual_seed(40)
    cells = torch.nonzero(torch.rand(40, 40, 40, generator=g) < 0.55)
    m = 32768 + 31
    assert cells.shape[0] >= m
    sites = torch.cat([torch.zeros(m, 1, dtype=torch.long), cells[torch.randperm(cells.shape[0], generator=g)[:m]]], 1)
    nbr, _ = ops.subm_neighbors(sites.int().to(dev), round(kvol ** (1 / 3)))
    x, w, bias, gamma, beta = _conv_inputs(m, c, kvol, dtype, dev, seed=c + kvol)
    got = ops.subm_conv_ln(x, w, nbr, bias, gamma, beta, EPS, ops.ACT_RELU)
    comp = _conv_composition(x, w, nbr, bias, gamma, beta, None)
    rows = torch.cat([torch.randperm(m, generator=g)[:1500], torch.arange(m - 40, m)])
    ref = ref_subm_conv_ln(x, w, nbr, bias, gamma, beta, EPS, rows=rows)
    _within_4x(got[rows.to(dev)], comp[rows.to(dev)], ref, f"subm_conv_ln two tiles c={c} kvol={kvol} {dtype}")
    assert torch.equal(got, ops.subm_conv_ln(x, w, nbr, bias, gamma, beta, EPS, ops.ACT_RELU))


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("c,kvol", [(16, 125), (16, 27), (128, 125)])
def test_subm_conv_ln_zero_input_gives_act_beta(dev, c, kvol, dtype):
    from ptv3_hip import ops
    nbr = _nbr(dev, "scatter", round(kvol ** (1 / 3)))
    m = nbr.shape[0]
    _, w, _, gamma, beta = _conv_inputs(m, c, kvol, dtype, dev, seed=3)
    got = ops.subm_conv_ln(torch.zeros(m, c, dtype=dtype, device=dev), w, nbr, None, gamma, beta, EPS, ops.ACT_RELU)
    assert torch.equal(got, torch.relu(beta).to(dtype).expand(m, c))


@pytest.mark.parametrize("c,kvol", [(24, 27), (16, 343), (256, 27)])
def test_subm_conv_ln_refuses_unserved_shapes(dev, c, kvol):
    from ptv3_hip import ops
    assert not ops.subm_conv_ln_capable(c, kvol, torch.float32)
    m = 40
    x = torch.randn(m, c, device=dev)
    w = torch.randn(c, kvol, c, device=dev)
    nbr = torch.full((m, kvol), -1, dtype=torch.int32, device=dev)
    vec = torch.ones(c, device=dev)
    out = torch.full((m, c), 7.0, device=dev)
    with pytest.raises(RuntimeError, match="subm_conv_ln"):
        ops.subm_conv_ln(x, w, nbr, vec, vec, vec, EPS, ops.ACT_RELU, out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ------------------------------------------------------------------------------------------------
# rows_linear_ln
# ------------------------------------------------------------------------------------------------
# 32769: the first row count past the two-row-tile threshold, one row into the last tile
ROWS = (1, 15, 16, 17, 4097, 32769)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("c,cout", [(16, 16), (32, 32), (64, 16), (128, 32), (256, 64), (512, 128)])
def test_rows_linear_ln_vs_float64(dev, c, cout, dtype, with_bias):
    from ptv3_hip import ops
    assert ops.rows_linear_ln_capable(c, cout, dtype)
    g = torch.Generator().manual_seed(c * 7 + cout)
    w = (torch.randn(cout, c, generator=g) / c ** 0.5).to(dtype).to(dev)
    bias = (0.2 * torch.randn(cout, generator=g)).to(dev) if with_bias else None
    gamma = (1 + 0.2 * torch.randn(cout, generator=g)).to(dev)
    beta = (0.3 * torch.randn(cout, generator=g)).to(dev)
    for m in ROWS:
        x = torch.randn(m, c, generator=g).to(dtype).to(dev)
        got = ops.rows_linear_ln(x, w, bias, gamma, beta, EPS, ops.ACT_RELU)
        comp = ops.affine_act(ops.layernorm(ops.gemm(x, w, bias=bias), gamma, beta, EPS), None, None, ops.ACT_RELU)
        ref = ref_rows_linear_ln(x, w, bias, gamma, beta, EPS)
        _within_4x(got, comp, ref, f"rows_linear_ln {c}->{cout} m={m} {dtype}")
        assert torch.equal(got, ops.rows_linear_ln(x, w, bias, gamma, beta, EPS, ops.ACT_RELU))


@pytest.mark.parametrize("c,cout", [(24, 16), (64, 256), (1024, 64), (64, 48)])
def test_rows_linear_ln_refuses_unserved_shapes(dev, c, cout):
    from ptv3_hip import ops
    assert not ops.rows_linear_ln_capable(c, cout, torch.float32)
    x = torch.randn(33, c, device=dev)
    w = torch.randn(cout, c, device=dev)
    vec = torch.ones(cout, device=dev)
    out = torch.full((33, cout), 7.0, device=dev)
    with pytest.raises(RuntimeError, match="rows_linear_ln"):
        ops.rows_linear_ln(x, w, None, vec, vec, EPS, ops.ACT_RELU, out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()
