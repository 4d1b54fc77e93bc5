"""GPU parity of ptv3_gemm_tn (csrc/backward.hip), the weight-gradient GEMM dW = dY^T . gather(X) with the bias
gradient from the same pass, called directly: against the plain statement of tests/gemm_tn_ref.py (itself held to
torch autograd by tests/test_gemm_tn_reference_cpu.py).

The shapes walk the kernel's launch-dependent paths: the packed tap path (kvol > 1, cin in 4 ... 32: a 64-column
tile spans 64 / cin taps), the plain conv path (one launch row per tap), partial 16 x 16 fragments and tiles, the
direct write (m <= 256) against row chunks -> slabs -> slab_sum split into dW and db, a last chunk of one row, and
more than 112 slabs.  Small-integer inputs make every product and partial sum an integer below 2^24, exact in fp32
in any summation order and exactly representable in bf16, so those cases are compared with torch.equal."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gemm_tn_ref import ref_gemm_tn, synth_nbr  # noqa: E402

pytestmark = pytest.mark.gpu

F = torch.nn.functional
TOL = 1e-4                  # the training path's budget (test_hip_backward.py): err <= 1e-4 * max(1, max|ref|)
BF16_STORE_TOL = 2.0 ** -7  # a result stored in bf16 (test_layernorm_backward_with_residual_gradient)
DTYPES = [torch.float32, torch.bfloat16]

# (m, cout, cin, kvol)
EXACT_SHAPES = [
    (1, 4, 4, 1),            # one row
    (255, 20, 36, 1),        # partial fragments both ways
    (256, 64, 64, 1),        # full tile, the last m written directly
    (257, 20, 36, 1),        # first slabbed m: a chunk of one row; the dW | db split (720) inside a reduction block
    (257, 68, 100, 1),       # two partial tiles each way
    (513, 132, 132, 1),      # three tiles each way
    (40001, 32, 32, 1),      # 157 slabs: slab_sum's unrolled loop and its tail
    (257, 32, 4, 27),        # packed, 16 taps per tile, last tile 44 columns
    (300, 20, 8, 27),        # packed, cin 8
    (1000, 64, 16, 27),      # packed, cin 16
    (5003, 32, 32, 27),      # packed, cin 32
    (700, 36, 8, 125),       # packed, k = 5
    (40001, 16, 32, 27),     # packed, 105 slabs
    (257, 32, 48, 27),       # plain conv: cin does not divide 64
    (1000, 48, 64, 27),      # plain conv
    (900, 68, 96, 27),       # plain conv, two column tiles, partial
    (300, 64, 128, 27),      # plain conv, two full column tiles
]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen)


@functools.lru_cache(maxsize=None)
def _int_case(m, cout, cin, kvol, dy_max=3, x_max=3):
    """int64 dy, x in [-max, max], the synthetic table and the int64 reference; built once, read by every dtype"""
    g = torch.Generator().manual_seed(m * 131 + cout * 17 + cin + kvol + dy_max + 7 * x_max)
    dy, x = _ints((m, cout), -dy_max, dy_max, g), _ints((m, cin), -x_max, x_max, g)
    nbr = synth_nbr(m, kvol, g) if kvol > 1 else None
    assert m * dy_max * max(x_max, 1) < 2 ** 24          # every partial sum of dw and db, in any order
    return (dy, x, nbr) + ref_gemm_tn(dy, x, nbr)


def _decode(got, ref, cin):
    bad = torch.nonzero(got != ref)
    o, col = bad[0].tolist()
    return (f"{bad.shape[0]} of {ref.numel()} entries differ, first (o, tap, c) = ({o}, {col // cin}, {col % cin}): "
            f"got {got[o, col].item()} want {ref[o, col].item()}")


def _check_exact(dev, dtype, with_bias, dy, x, nbr, dw_ref, db_ref):
    from ptv3_hip import ops
    kvol = 1 if nbr is None else nbr.shape[1]
    res = ops.gemm_tn(dy.to(dtype).to(dev), x.to(dtype).to(dev), None if nbr is None else nbr.to(dev), kvol,
                      with_bias=with_bias)
    dw, db = res if with_bias else (res, None)
    assert dw.dtype == torch.float32 and dw.shape == dw_ref.shape
    dw = dw.cpu().double()
    assert torch.equal(dw, dw_ref.double()), _decode(dw, dw_ref.double(), x.shape[1])
    if with_bias:
        assert db.dtype == torch.float32 and torch.equal(db.cpu().double(), db_ref.double()), "db"


# ------------------------------------------------------------------------------------------------
# a. small integers: exact in both dtypes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,cout,cin,kvol", EXACT_SHAPES)
def test_small_integers_are_exact(dev, m, cout, cin, kvol, dtype, with_bias):
    _check_exact(dev, dtype, with_bias, *_int_case(m, cout, cin, kvol))


# ------------------------------------------------------------------------------------------------
# b. one operand fills the mantissa: fails if either operand loses significant bits on its way to the matrix core
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", ["dy", "x"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,cout,cin,kvol", [(4000, 68, 100, 1), (1000, 64, 16, 27)])
def test_wide_mantissa_integers_are_exact(dev, m, cout, cin, kvol, dtype, wide):
    # |sum| <= 2047 * 4000 < 2^23 (fp32); bf16 holds the integers up to 256 exactly
    big = 2047 if dtype == torch.float32 else 255
    dy, x, nbr, dw, db = _int_case(m, cout, cin, kvol, *((big, 1) if wide == "dy" else (1, big)))
    assert (dy if wide == "dy" else x).abs().max().item() == big
    _check_exact(dev, dtype, True, dy, x, nbr, dw, db)


# ------------------------------------------------------------------------------------------------
# c. every output element is written: NaN-filled outputs, one tap absent for every row
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,cout,cin,kvol", [(257, 32, 4, 27), (300, 64, 128, 27)])
def test_no_output_element_is_left_unwritten(dev, m, cout, cin, kvol, dtype):
    from ptv3_hip import ops
    from ptv3_hip.lib import lib
    dy, x, nbr, dw_ref, db_ref = _int_case(m, cout, cin, kvol)
    assert (nbr[:, kvol // 2] < 0).all()
    dyd, xd, nbrd = dy.to(dtype).to(dev), x.to(dtype).to(dev), nbr.to(dev)
    # ops.gemm_tn with the outputs filled first (it allocates with torch.empty: a skipped store could read as zero)
    dw = torch.full((cout, kvol * cin), float("nan"), dtype=torch.float32, device=dev)
    db = torch.full((cout,), float("nan"), dtype=torch.float32, device=dev)
    nb = lib.ptv3_gemm_tn_workspace_bytes(m, cout, cin, kvol)
    ws = torch.empty(max(int(nb), 1), dtype=torch.uint8, device=dev)
    lib.check(lib.ptv3_gemm_tn(dyd.data_ptr(), xd.data_ptr(), nbrd.data_ptr(), dw.data_ptr(), db.data_ptr(), m, cout,
                               cin, kvol, ops._dt(dyd), ws.data_ptr(), nb, ops._stream()), "ptv3_gemm_tn")
    assert not torch.isnan(dw).any() and not torch.isnan(db).any()
    assert (dw.view(cout, kvol, cin)[:, kvol // 2] == 0).all()
    assert torch.equal(dw.cpu().double(), dw_ref.double()), _decode(dw.cpu().double(), dw_ref.double(), cin)
    assert torch.equal(db.cpu().double(), db_ref.double())


# ------------------------------------------------------------------------------------------------
# d. random floats against float64; the same call twice is bitwise the same
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float_case(m, cout, cin, kvol):
    g = torch.Generator().manual_seed(m + cout + cin + kvol)
    dy, x = torch.randn(m, cout, generator=g), torch.randn(m, cin, generator=g)
    return dy, x, synth_nbr(m, kvol, g) if kvol > 1 else None


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,cout,cin,kvol", [(257, 68, 100, 1), (5003, 32, 32, 27), (900, 68, 96, 27),
                                             (40001, 32, 32, 1)])
def test_random_floats_vs_float64_and_run_to_run(dev, m, cout, cin, kvol, dtype):
    """bf16: the reference is taken on the bf16-rounded inputs; products of bf16 pairs are exact in fp32 and the
    accumulators are fp32, so bf16 is held to the fp32 budget, not to the 3e-2 of the whole-model checks."""
    from ptv3_hip import ops
    dy, x, nbr = _float_case(m, cout, cin, kvol)
    dy, x = dy.to(dtype), x.to(dtype)
    dw_ref, db_ref = ref_gemm_tn(dy.double(), x.double(), nbr)
    args = (dy.to(dev), x.to(dev), None if nbr is None else nbr.to(dev), kvol)
    dw, db = ops.gemm_tn(*args, with_bias=True)
    dw2, db2 = ops.gemm_tn(*args, with_bias=True)
    worst = 0.0
    for got, ref in ((dw, dw_ref), (db, db_ref)):
        worst = max(worst, (got.cpu().double() - ref).abs().max().item() / max(1.0, ref.abs().max().item()))
    print(f"gemm_tn {m}x{cout}x{cin}x{kvol} {str(dtype)[6:]}: worst err / scale {worst:.3e}")
    assert worst <= TOL
    assert torch.equal(dw, dw2) and torch.equal(db, db2)     # fixed chunks, ordered sums, no atomics


# ------------------------------------------------------------------------------------------------
# e. through autograd, on real scenes: row_order, bf16 convolutions, channel counts off the granules
# ------------------------------------------------------------------------------------------------
def _close(got, ref, tol, what):
    scale = max(1.0, ref.abs().max().item())
    err = (got.detach().cpu().double() - ref).abs().max().item()
    assert err <= tol * scale, f"{what}: err {err:.3e} vs scale {scale:.3e}"


def _leaf(t, dev=None, dtype=None):
    t = t.clone()
    if dev is not None:
        t = t.to(dev)
    if dtype is not None:
        t = t.to(dtype)
    return t.requires_grad_(True)


@functools.lru_cache(maxsize=None)
def _conv_case(cin, cout, k, dtype):
    """two scenes (~1500 sites), random x / w / b / dy and float64 autograd of the oracle's conv on the values the
    kernels see: x, dy and the weight rounded to `dtype`, the bias left in fp32"""
    from oracle import ptv3 as O
    import ptv3_scenes as S
    data = S.make_batch([1000, 500], in_channels=cin, extent=40, seed=cin + k)
    gc, off = data["grid_coord"], data["offset"]
    n = gc.shape[0]
    batch = torch.repeat_interleave(torch.arange(2), torch.diff(off, prepend=torch.zeros(1, dtype=torch.long)))
    indices = torch.cat([batch[:, None], gc], 1).int()
    g = torch.Generator().manual_seed(cout)
    x = torch.randn(n, cin, generator=g).to(dtype)
    w = torch.randn(cout, k, k, k, cin, generator=g) / (cin * 9) ** 0.5
    b = torch.randn(cout, generator=g)
    dy = torch.randn(n, cout, generator=g).to(dtype)
    xr, wr, br = _leaf(x.double()), _leaf(w.to(dtype).double()), _leaf(b.double())
    O.subm_conv3d(xr, indices, wr, br).backward(dy.double())
    return indices, x, w, b, dy, xr.grad, wr.grad, br.grad


def _conv_grads(dev, case, nbr, row_order):
    from ptv3_hip import autograd as A
    _, x, w, b, dy = case[:5]
    xd, wd, bd = _leaf(x, dev), _leaf(w, dev), _leaf(b, dev)
    A.subm_conv(xd, wd, bd, nbr, row_order).backward(dy.to(dev))
    assert xd.grad.dtype == x.dtype and wd.grad.dtype == torch.float32 and wd.grad.shape == w.shape
    assert bd.grad.shape == b.shape
    return xd.grad, wd.grad, bd.grad


@pytest.mark.parametrize("cin,cout,k", [(8, 20, 3), (48, 36, 3)])
def test_subm_conv_backward_with_a_row_order(dev, cin, cout, k):
    from ptv3_hip import ops
    case = _conv_case(cin, cout, k, torch.float32)
    nbr, _ = ops.subm_neighbors(case[0].to(dev), k)
    n = case[1].shape[0]
    order = torch.randperm(n, generator=torch.Generator().manual_seed(n)).int().to(dev)
    plain, ordered = _conv_grads(dev, case, nbr, None), _conv_grads(dev, case, nbr, order)
    for got, other, ref, what in zip(ordered, plain, case[5:], ("dx", "dw", "db")):
        _close(got, ref, TOL, what)
        _close(other, ref, TOL, what + " (row_order=None)")
        assert torch.equal(got, other), f"{what} depends on the visiting order"


@pytest.mark.parametrize("cin,cout,k", [(6, 20, 3), (16, 32, 5)])
def test_subm_conv_backward_bf16(dev, cin, cout, k):
    """dw / db leave fp32 accumulators over exact products: 1e-4 of scale against the reference on the rounded
    values; dx is stored in bf16.  cin = 6 is padded to the K granule (8) and sliced off again."""
    from ptv3_hip import ops
    case = _conv_case(cin, cout, k, torch.bfloat16)
    nbr, _ = ops.subm_neighbors(case[0].to(dev), k)
    dx, dw, db = _conv_grads(dev, case, nbr, None)
    _close(dw, case[6], TOL, "dw")
    _close(db, case[7], TOL, "db")
    _close(dx, case[5], BF16_STORE_TOL, "dx")


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_backward_off_the_granules(dev, dtype):
    """cout = 13, cin = 6: dy is padded to a multiple of 4 and x to the K granule; both paddings come off again"""
    from ptv3_hip import autograd as A
    m, cin, cout = 300, 6, 13
    g = torch.Generator().manual_seed(13)
    x = torch.randn(m, cin, generator=g).to(dtype)
    w, b = torch.randn(cout, cin, generator=g) / cin ** 0.5, torch.randn(cout, generator=g)
    dy = torch.randn(m, cout, generator=g).to(dtype)
    xr, wr, br = _leaf(x.double()), _leaf(w.to(dtype).double()), _leaf(b.double())
    F.linear(xr, wr, br).backward(dy.double())
    xd, wd, bd = _leaf(x, dev), _leaf(w, dev), _leaf(b, dev)
    A.linear(xd, wd, bd).backward(dy.to(dev))
    assert wd.grad.shape == (13, 6) and bd.grad.shape == (13,) and xd.grad.shape == (m, 6)
    assert wd.grad.dtype == torch.float32 and xd.grad.dtype == dtype
    _close(wd.grad, wr.grad, TOL, "dw")
    _close(bd.grad, br.grad, TOL, "db")
    _close(xd.grad, xr.grad, TOL if dtype == torch.float32 else BF16_STORE_TOL, "dx")


# ------------------------------------------------------------------------------------------------
# f. edges of the entry point
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kvol", [1, 27])
def test_no_rows_gives_zero_gradients(dev, kvol, dtype):
    from ptv3_hip import ops
    dy, x = torch.zeros(0, 20, dtype=dtype, device=dev), torch.zeros(0, 8, dtype=dtype, device=dev)
    nbr = torch.zeros(0, kvol, dtype=torch.int32, device=dev) if kvol > 1 else None
    dw, db = ops.gemm_tn(dy, x, nbr, kvol, with_bias=True)
    assert dw.shape == (20, kvol * 8) and db.shape == (20,)
    assert (dw == 0).all() and (db == 0).all()
    assert (ops.gemm_tn(dy, x, nbr, kvol) == 0).all()


def test_bad_arguments_are_refused(dev):
    from ptv3_hip import ops
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.gemm_tn(z(5, 6), z(5, 8))
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.gemm_tn(z(5, 8, dtype=torch.bfloat16), z(5, 6, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.gemm_tn(z(5, 8), z(5, 6), z(5, 27, dtype=torch.int32), 27)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.gemm_tn(z(5, 8), z(5, 8), z(4, 27, dtype=torch.int32), 27)
    with pytest.raises(RuntimeError, match="shape mismatch"):
        ops.gemm_tn(z(5, 8), z(4, 8))
