"""GPU tests of the LayerNorm and GELU kernels in every variant the launchers can choose, against the float64 references
and the derived per-element bound E of tests/norm_ref.py (tests/test_norm_reference_cpu.py shows E is a bound, that it
is not slack, and which seeded defect each input family catches):

A. ops.layernorm: every lanes-per-row variant, ragged and full multi-chunk rows, row counts around the rows-per-block
   edges, seven input families, fp32 and bf16, the four call forms (plain, res, chained second norm, both);
B. ops.layernorm_slabs: split-K slab input, x = T(bias + slabs in slab order);
C. ops.layernorm_bwd: the packed kernel and NC = 1, 2, 4, 8, 16, both col_chunks regimes, with and without `add`, and
   the autograd wrapper at Swin3D's widths;
D. GELU / ReLU forward and derivative over every finite bf16 value and a dense fp32 grid on [-12, 12], against the
   accuracy figures the source comments claim (1.5e-7 for the erf, 3.1e-4 for the polynomial of the bf16 wide kernels);
E. the LayerNorm prologues of ops.rows_linear and the LayerNorm epilogue of ops.rows_linear_ln through identity weights
   (the GEMM is then exact), with the fused kernels' own summation depths;
and ops.cast bit for bit.

Pass criterion unless stated: |got - ref64| <= 4 E + one output ulp per element; the output ulp is 0 for fp32 and the
bf16 ulp of the reference for bf16 (the factor and the ulp are those of tests/test_hip_window_attn_paths.py).  The
references and bounds are evaluated in torch float64 on the device from the formulas of norm_ref (they are written with
operators only); bf16 cases round the inputs to bf16 first.  The reference of a chained second norm (y2, and `out` of
the ln0 + shortcut prologue) is taken from the kernel's own stored y / f1, which is what that norm reads: a one-ulp flip
in y is not charged to it.

Every test prints, per output, the largest err / E (bf16: the largest (err - ulp) / E, negative when the output
rounding alone covers the error); D prints the largest error and where.

Largest figures on an MI355X (one run).  fp32: err / E; bf16: (err - ulp) / E.  The bound allows 4.
  group  output            fp32                           bf16
  A      y                 0.979 (c 192)                  0.106
  A      y2                0.492                          0.079
  B      y / y2            0.959 / 0.497                  0.095 / 0.024
  C      dx                0.999 (every width, see below) 0.248 (c 3)
  C      dgamma / dbeta    0.312 / 0.076                  0.254 / 0.017
  C      autograd          -                              y 0.087 dx 0.082 dgamma 0.067 dbeta 0.011
  E      rows_linear       out 0.460 f1 0.924 out2 0.482  out 0.005 f1 0.022 out2 0.010
  E      rows_linear_ln    out 0.476 relu 0.476           out 0.056
dx reaches 0.99 in the `outlier` and `huge` families with `add`: rstd is 1e-4 there, so dx = add + rstd t is one rounded
addition and its u |dx| is all of E (the emulation on the CPU shows the same 0.97 .. 0.99).
  D  erf GELU value (affine_act and the GEMM epilogue, fp32): largest error 4.59e-7 at x = 3.04 (two ulps of the result);
     closest to the bound (|x| / 2) (1.5e-7 + 4 u) + 2 u |ref| at x = -0.067: 0.95 of it, i.e. the erf is off by 3.7e-7
     there: the 1.5e-7 of the formula plus the fp32 roundings of 1 - p e near 0; with a scale in front 0.985 at x = 0.069.
     bf16: 0.50 of the bound.
  D  erf GELU derivative (act_bwd): fp32 largest error 2.51e-7, 0.65 of (1.5e-7 + 4 u) / 2 + 6 u (|ref| + |z pdf|); no term
     for exp2 was needed.  bf16: 0.50.
  D  polynomial GELU of the bf16 wide kernels: 3.04e-4 beyond the output ulp, at x = -3.8125 (documented: 3.1e-4).
No figure above 4, no documented accuracy exceeded."""
import math

import numpy as np
import pytest
import torch

import norm_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 4.0
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)
EPS = R.EPS
SEED = 20
U = R.U


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _name(dt):
    return "fp32" if dt == F32 else "bf16"


class _Worst:
    """largest (err - floor) / E per output name"""

    def __init__(self):
        self.v = {}

    def add(self, name, r):
        self.v[name] = max(self.v.get(name, -math.inf), r)

    def line(self):
        return " ".join(f"{k} {v:.3f}" for k, v in self.v.items())


def _check(tag, name, got, ref, E, dt, worst):
    """per element: |got - ref| <= 4 E + (bf16: one bf16 ulp of ref)"""
    got = got.double()
    assert got.shape == ref.shape, (tag, name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{tag} {name}: non-finite output"
    err = (got - ref).abs()
    floor = R.ulp(ref, True) if dt == BF16 else torch.zeros_like(ref)
    worst.add(name, ((err - floor) / E.clamp_min(1e-300)).max().item())    # E = 0: dgamma at c = 1 (xhat is exactly 0)
    bad = err > MARGIN * E + floor
    if bad.any():
        i = torch.nonzero(bad)[0].tolist()
        j = tuple(i)
        raise AssertionError(f"{tag} {name}: {int(bad.sum())} elements outside 4 E + ulp; first at {i}: "
                             f"got {got[j].item():.9g} ref {ref[j].item():.9g} err {err[j].item():.3e} "
                             f"E {E[j].item():.3e} floor {floor[j].item():.3e} "
                             f"worst (err - floor) / E {((err - floor) / E.clamp_min(1e-300)).max().item():.2f}")


def _dev(d, dev, dt, mats=("x", "res", "dy", "add")):
    """a norm_ref input dict on the device: matrices in dt, vectors fp32"""
    return {k: torch.from_numpy(v).to(dev).to(dt if k in mats else F32) for k, v in d.items()}


# ------------------------------------------------------------------------------------------------
# A. ops.layernorm
# ------------------------------------------------------------------------------------------------
def _forward_forms(tag, call, t, m, ref, E, dt, worst, depth=None):
    """the four call forms of a forward at the first m rows; ref / E: (plain, with res) of all rows.
    call(res, gamma2, beta2) -> y or (y, y2)"""
    res = t["res"][:m].contiguous()
    for with_res in (False, True):
        for chained in (False, True):
            out = call(res if with_res else None, t["gamma2"] if chained else None, t["beta2"] if chained else None)
            y = out[0] if chained else out
            form = f"{tag} m {m} res {int(with_res)} chained {int(chained)}"
            _check(form, "y", y, ref[with_res][:m], E[with_res][:m], dt, worst)
            if chained:
                ref2 = R.layernorm_f64(y, t["gamma2"], t["beta2"], EPS)
                E2 = R.forward_bound(y, t["gamma2"], t["beta2"], EPS, depth=depth, depth_q=depth)
                _check(form, "y2", out[1], ref2, E2, dt, worst)


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("c", R.FWD_WIDTHS)
def test_layernorm_forward(dev, c, dt):
    from ptv3_hip import ops
    worst = _Worst()
    mmax = max(R.FWD_ROWS)
    for fam in R.FAMILIES:
        # rows are independent: one reference for the largest row count serves the smaller ones
        t = _dev(R.make_inputs(fam, mmax, c, SEED, dt == BF16), dev, dt)
        ref = [R.layernorm_f64(t["x"], t["gamma"], t["beta"], EPS, r) for r in (None, t["res"])]
        E = [R.forward_bound(t["x"], t["gamma"], t["beta"], EPS, r) for r in (None, t["res"])]
        for m in R.FWD_ROWS:
            x = t["x"][:m].contiguous()
            _forward_forms(f"A {fam} c {c} {_name(dt)}",
                           lambda r, g2, b2: ops.layernorm(x, t["gamma"], t["beta"], EPS, r, g2, b2), t, m, ref, E, dt, worst)
    print(f"\nNORMPATH A layernorm c {c} lpr {R.forward_lpr(c)} {_name(dt)}: {worst.line()}", end="")


def test_layernorm_forward_edges(dev):
    from ptv3_hip import ops
    from ptv3_hip.lib import lib
    for dt in DTYPES:
        for c, m in ((4, 257), (48, 17), (1028, 5)):
            t = _dev(R.make_inputs("randn", m, c, SEED, dt == BF16), dev, dt)
            # an output with rows to spare: the rows at and beyond m keep their canary
            y = torch.full((m + 300, c), -768.0, dtype=dt, device=dev)
            y2 = torch.full((m + 300, c), -768.0, dtype=dt, device=dev)
            lib.check(lib.ptv3_layernorm(t["x"].data_ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), None, y.data_ptr(),
                                         t["gamma2"].data_ptr(), t["beta2"].data_ptr(), y2.data_ptr(), m, c, EPS,
                                         ops._dt(t["x"]), ops._stream()), "ptv3_layernorm")
            want = ops.layernorm(t["x"], t["gamma"], t["beta"], EPS, None, t["gamma2"], t["beta2"])
            assert torch.equal(y[:m], want[0]) and torch.equal(y2[:m], want[1])
            assert (y[m:] == -768.0).all() and (y2[m:] == -768.0).all()
        g = torch.ones(8, device=dev)
        out = ops.layernorm(torch.empty((0, 8), dtype=dt, device=dev), g, g, EPS, None, g, g)
        assert out[0].shape == (0, 8) and out[1].shape == (0, 8)
        for c in (6, 2052):
            g = torch.ones(c, device=dev)
            with pytest.raises(RuntimeError, match="must be a multiple of 4, <= 2048"):
                ops.layernorm(torch.zeros((3, c), dtype=dt, device=dev), g, g)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# B. ops.layernorm_slabs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("c", R.SLAB_WIDTHS)
def test_layernorm_slabs(dev, c, dt):
    from ptv3_hip import ops
    worst = _Worst()
    m = 257
    for splits in R.SLAB_SPLITS:
        for fam in R.FAMILIES:
            d = R.make_inputs(fam, m, c, SEED + splits, False)
            g = np.random.default_rng([SEED, splits, c])
            bias = (0.25 * g.standard_normal(c)).astype(np.float32)
            # slabs whose sum is the family's x up to fp32 rounding; x itself is DEFINED as the kernel documents it:
            # bias + slab 0 + slab 1 + ... in fp32, rounded to the output type
            slabs = g.standard_normal((splits, m, c)).astype(np.float32) * np.abs(d["x"]).mean().astype(np.float32)
            slabs[0] = d["x"] - bias - slabs[1:].sum(axis=0, dtype=np.float32)
            d["x"] = R.slab_input(slabs, bias, dt == BF16)
            if dt == BF16:
                d["res"] = R.round_bf16(d["res"])
            t = _dev(d, dev, dt)
            slab_t = torch.from_numpy(slabs).to(dev)
            bias_t = torch.from_numpy(bias).to(dev)
            ref = [R.layernorm_f64(t["x"], t["gamma"], t["beta"], EPS, r) for r in (None, t["res"])]
            E = [R.forward_bound(t["x"], t["gamma"], t["beta"], EPS, r) for r in (None, t["res"])]
            for rows in (1, m):
                sl = slab_t[:, :rows].contiguous()
                _forward_forms(f"B {fam} c {c} splits {splits} {_name(dt)}",
                               lambda r, g2, b2: ops.layernorm_slabs(sl, splits, rows, c, bias_t, dt, t["gamma"],
                                                                     t["beta"], EPS, r, g2, b2),
                               t, rows, ref, E, dt, worst)
    print(f"\nNORMPATH B layernorm_slabs c {c} {_name(dt)}: {worst.line()}", end="")


# ------------------------------------------------------------------------------------------------
# C. ops.layernorm_bwd
# ------------------------------------------------------------------------------------------------
def _check_bwd(tag, got, t, add, dt, worst):
    ref = R.layernorm_bwd_f64(t["x"], t["dy"], t["gamma"], EPS, add)
    E = R.backward_bound(t["x"], t["dy"], t["gamma"], EPS, add)
    _check(tag, "dx", got[0], ref[0], E[0], dt, worst)
    _check(tag, "dgamma", got[1], ref[1], E[1], F32, worst)
    _check(tag, "dbeta", got[2], ref[2], E[2], F32, worst)


@pytest.mark.parametrize("c", R.BWD_WIDTHS)
def test_layernorm_backward(dev, c):
    from ptv3_hip import ops
    for dt in DTYPES:
        worst = _Worst()
        for m in R.BWD_ROWS:
            for fam in R.FAMILIES:
                t = _dev(R.make_bwd_inputs(fam, m, c, SEED, dt == BF16), dev, dt)
                tag = f"C {fam} c {c} ({R.backward_variant(c)}) m {m} {_name(dt)}"
                plain = ops.layernorm_bwd(t["x"], t["dy"], t["gamma"], EPS)
                _check_bwd(tag, plain, t, None, dt, worst)
                added = ops.layernorm_bwd(t["x"], t["dy"], t["gamma"], EPS, add=t["add"])
                _check_bwd(tag + " add", added, t, t["add"], dt, worst)
                assert torch.equal(plain[1], added[1]) and torch.equal(plain[2], added[2]), tag
        print(f"\nNORMPATH C layernorm_bwd c {c} variant {R.backward_variant(c)} {_name(dt)}: {worst.line()}", end="")


def test_layernorm_backward_edges(dev):
    from ptv3_hip import ops
    for dt in DTYPES:
        g = torch.ones(1025, device=dev)
        z = torch.zeros((3, 1025), dtype=dt, device=dev)
        with pytest.raises(RuntimeError, match=r"outside \[1,1024\]"):
            ops.layernorm_bwd(z, z, g, EPS)
        for c in (48, 64):
            e = torch.empty((0, c), dtype=dt, device=dev)
            dx, dg, db = ops.layernorm_bwd(e, e, torch.ones(c, device=dev), EPS)
            assert dx.shape == (0, c) and (dg == 0).all() and (db == 0).all()
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", R.SWIN_WIDTHS)
def test_layer_norm_autograd_swin_widths(dev, c):
    """the autograd wrapper hands the same reference's gradients back (bf16 activations, fp32 parameters)"""
    from ptv3_hip import autograd as A
    worst = _Worst()
    for fam in R.FAMILIES:
        t = _dev(R.make_bwd_inputs(fam, 301, c, SEED, True), dev, BF16)
        x = t["x"].clone().requires_grad_(True)
        w = t["gamma"].clone().requires_grad_(True)
        b = t["beta"].clone().requires_grad_(True)
        y = A.layer_norm(x, w, b, EPS)
        _check(f"C autograd {fam} c {c}", "y", y.detach(), R.layernorm_f64(t["x"], t["gamma"], t["beta"], EPS),
               R.forward_bound(t["x"], t["gamma"], t["beta"], EPS), BF16, worst)
        y.backward(t["dy"])
        _check_bwd(f"C autograd {fam} c {c}", (x.grad, w.grad, b.grad), t, None, BF16, worst)
    print(f"\nNORMPATH C autograd layer_norm c {c} bf16: {worst.line()}", end="")


# ------------------------------------------------------------------------------------------------
# D. GELU and ReLU
# ------------------------------------------------------------------------------------------------
ERF_CLAIM = 1.5e-7      # csrc/common.h, erf_fast: Abramowitz & Stegun 7.1.26
POLY_CLAIM = 3.1e-4     # csrc/block_wide.hip, gelu_poly2
TINY = 2.0 ** -149      # spacing of the fp32 subnormals: a result below 2^-126 cannot be closer than half of it
EXTREMES = np.array([1e4, -1e4, 3e38, -3e38, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 0.0, -0.0], dtype=np.float32)


def _grid(dev, dt):
    """(x (rows, 128) in dt, the same values as float64 numpy): fp32: the whole grid of norm_ref, bf16: every finite bf16"""
    v = R.gelu_grid() if dt == F32 else R.bf16_values()
    v = np.concatenate([v, EXTREMES, np.zeros(-(v.size + EXTREMES.size) % 128, dtype=np.float32)])
    if dt == BF16:
        v = R.round_bf16(v)
    return torch.from_numpy(v).to(dev).to(dt).reshape(-1, 128), v.astype(np.float64)


def _value_bound(z, ref):
    """|err| <= (|z| / 2) (1.5e-7 + 4 u) + 2 u |ref|: the erf's claimed absolute error and four roundings of its
    evaluation, times z / 2; two roundings of the products.  TINY: the fp32 format's floor for subnormal results."""
    return np.abs(z) / 2 * (ERF_CLAIM + 4 * U) + 2 * U * np.abs(ref) + TINY


def _grad_bound(z, ref):
    """(1.5e-7 + 4 u) / 2 + 6 u (|ref| + |z pdf|)"""
    return (ERF_CLAIM + 4 * U) / 2 + 6 * U * (np.abs(ref) + np.abs(R.gelu_pdf_term_f64(z))) + TINY


def _report(tag, got, ref, bound, z, floor=None):
    got = got.double().cpu().numpy().reshape(-1)
    assert np.isfinite(got).all(), f"{tag}: non-finite result"
    err = np.abs(got - ref)
    if floor is not None:
        bound = bound + floor
    i = int(np.argmax(err - (0 if floor is None else floor)))
    k = int(np.argmax(err / bound))
    print(f"\nNORMPATH D {tag}: largest err {err[i]:.3e} at x {z[i]:.6g} (beyond the output ulp: "
          f"{(err - (0 if floor is None else floor)).max():.3e}); largest err/bound {err[k] / bound[k]:.3f} "
          f"at x {z[k]:.6g}", end="")
    assert (err <= bound).all(), (f"{tag}: err {err[k]:.3e} > bound {bound[k]:.3e} at x {z[k]:.9g} "
                                  f"(got {got[k]:.9g} ref {ref[k]:.9g})")
    return got


SCALES = np.tile(np.array([0.5, 1.0, -1.0, 0.25], dtype=np.float32), 32)


def _scaled(x):
    """fp32(x * SCALES[column] + 0) as float64, and where the exact product is nonzero but rounds to zero"""
    exact = x.double().cpu().numpy() * SCALES.astype(np.float64) + 0.0
    with np.errstate(under="ignore"):
        z = exact.astype(np.float32).astype(np.float64).reshape(-1)
    return z, (exact.reshape(-1) != 0) & (z == 0)


def _zero_signs(tag, got, z):
    """a zero result of GELU carries the sign of its argument (x Phi(x) -> -0 in the negative tail)"""
    bad = (got == 0) & (np.signbit(got) != np.signbit(z))
    assert not bad.any(), (f"{tag}: wrong sign of zero at {int(bad.sum())} arguments, the first {z[bad][:6]!r} "
                           f"(positions {np.nonzero(bad)[0][:6]})")


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_gelu_value_forms(dev, dt):
    from ptv3_hip import ops
    x, z = _grid(dev, dt)
    ref = R.gelu_f64(z)
    floor = R.ulp(ref, True) if dt == BF16 else None
    got = _report(f"affine_act GELU {_name(dt)}", ops.affine_act(x, None, None, ops.ACT_GELU), ref, _value_bound(z, ref), z,
                  floor)
    _zero_signs("affine_act", got, z)
    # the GELU epilogue of the tiled GEMM: identity weight and zero bias make the product exact (checked: the plain GEMM
    # returns x; a matrix core may flush a subnormal input to zero, so the epilogue is measured on what it was given)
    eye = torch.eye(128, dtype=dt, device=dev)
    zero = torch.zeros(128, device=dev)
    zg = ops.gemm(x, eye, zero).double().cpu().numpy().reshape(-1)
    normal = np.abs(z) >= 2.0 ** -126
    assert (zg[normal] == z[normal]).all() and ((zg == z) | (zg == 0))[~normal].all()
    refg = R.gelu_f64(zg)
    got = _report(f"gemm GELU epilogue {_name(dt)}", ops.gemm(x, eye, zero, act=ops.ACT_GELU), refg,
                  _value_bound(zg, refg), zg, R.ulp(refg, True) if dt == BF16 else None)
    # the accumulator turns an input of -0 into +0: the sign of what the epilogue was given
    _zero_signs("gemm", got, zg)
    # with scale / shift: scales that are powers of two and a zero shift: x * scale + 0 is one rounding of an exact
    # product however the compiler contracts it.  Only the sign of a product that underflows to zero depends on that
    # (fused: the sign of the product; product first: -0 + 0 = +0): no sign is asked for there.
    zs, amb = _scaled(x)
    refs = R.gelu_f64(zs)
    got = _report(f"affine_act GELU scaled {_name(dt)}",
                  ops.affine_act(x, torch.from_numpy(SCALES).to(dev), torch.zeros(128, device=dev), ops.ACT_GELU), refs,
                  _value_bound(zs, refs), zs, R.ulp(refs, True) if dt == BF16 else None)
    _zero_signs("affine_act scaled", got[~amb], zs[~amb])


def test_gelu_scale_shift_columns(dev):
    """scale and shift are taken per column: multiples of 1/8 keep x * scale + shift exact however it is contracted"""
    from ptv3_hip import ops
    k = np.arange(-64, 64, dtype=np.float32)
    x = np.stack([np.roll(k, r) / 8 for r in range(9)])                        # (9, 128)
    sc = np.tile(np.array([0.5, 1.0, -2.0, 4.0], dtype=np.float32), 32)
    sh = (np.arange(128, dtype=np.float32) - 60) / 8
    z = (x.astype(np.float64) * sc + sh).reshape(-1)
    xt, sct, sht = (torch.from_numpy(a).to(dev) for a in (x, sc, sh))
    ref = R.gelu_f64(z)
    _report("affine_act GELU scale/shift columns fp32", ops.affine_act(xt, sct, sht, ops.ACT_GELU), ref,
            _value_bound(z, ref), z)
    refg = R.gelu_grad_f64(z)
    _report("act_bwd GELU scale/shift columns fp32", ops.act_bwd(torch.ones_like(xt), xt, ops.ACT_GELU, sct, sht), refg,
            _grad_bound(z, refg), z)
    relu = ops.affine_act(xt, sct, sht, ops.ACT_RELU).double().cpu().numpy().reshape(-1)
    assert (relu == np.maximum(z, 0.0)).all()
    drelu = ops.act_bwd(torch.ones_like(xt), xt, ops.ACT_RELU, sct, sht).double().cpu().numpy().reshape(-1)
    assert (drelu == (z > 0)).all()


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_gelu_derivative(dev, dt):
    """Phi(z) + z phi(z) over the grid and the finite extremes: finite and within the bound.  No sign is asked of a zero
    here: the derivative is zero only in the far negative tail, as the sum of a +0 and a -0 term."""
    from ptv3_hip import ops
    x, z = _grid(dev, dt)
    ref = R.gelu_grad_f64(z)
    floor = R.ulp(ref, True) if dt == BF16 else None
    one = torch.ones_like(x)
    _report(f"act_bwd GELU {_name(dt)}", ops.act_bwd(one, x, ops.ACT_GELU), ref, _grad_bound(z, ref), z, floor)
    zs, _ = _scaled(x)
    refs = R.gelu_grad_f64(zs)
    _report(f"act_bwd GELU scaled {_name(dt)}",
            ops.act_bwd(one, x, ops.ACT_GELU, torch.from_numpy(SCALES).to(dev), torch.zeros(128, device=dev)), refs,
            _grad_bound(zs, refs), zs, R.ulp(refs, True) if dt == BF16 else None)


def test_gelu_polynomial_of_the_wide_kernels(dev):
    """gelu_poly2 through ops.rows_linear (bf16, c = cout = 128, identity weight, zero bias, no prologue) on every finite
    bf16 value: within the claimed 3.1e-4 of the float64 GELU plus one bf16 ulp; beyond the clamp exactly x or a zero"""
    from ptv3_hip import ops
    v = R.bf16_values()
    assert v.size == 510 * 128
    x = torch.from_numpy(v).to(dev).to(BF16).reshape(510, 128)
    assert ops.rows_linear_capable(128, 128, BF16, 510)
    out = ops.rows_linear(x, torch.eye(128, dtype=BF16, device=dev), torch.zeros(128, device=dev), act=ops.ACT_GELU)
    z = v.astype(np.float64)
    ref = R.gelu_f64(z)
    got = _report("rows_linear GELU polynomial bf16", out, ref, np.full_like(ref, POLY_CLAIM), z, R.ulp(ref, True))
    inside = np.abs(z) < 2.75 * math.sqrt(2.0)
    print(f"; inside the clamp: largest err {np.abs(got - ref)[inside].max():.3e}, beyond the bf16 ulp "
          f"{(np.abs(got - ref) - R.ulp(ref, True))[inside].max():.3e} (claimed {POLY_CLAIM:.1e})", end="")
    hi, lo = z >= 2.75 * math.sqrt(2.0), z <= -2.75 * math.sqrt(2.0)
    assert (got[hi] == z[hi]).all(), "beyond the clamp GELU(x) must be x"
    assert (got[lo] == 0).all(), "beyond the clamp GELU(-x) must be a zero"
    zero = (z == 0)
    assert (got[zero] == 0).all()


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
def test_relu_exact(dev, dt):
    """ReLU and its derivative over the grid, bit for bit; max(-0, +0) may be either zero"""
    from ptv3_hip import ops
    x, z = _grid(dev, dt)
    got = ops.affine_act(x, None, None, ops.ACT_RELU)
    want = torch.where(x > 0, x, torch.zeros_like(x))
    minus0 = (x == 0) & torch.signbit(x)
    assert torch.equal(got, want)                                   # values (-0 == +0)
    assert not torch.signbit(got[~minus0]).any(), "ReLU of a nonzero or +0 input is never negative"
    assert torch.equal(got[x > 0].view(torch.int16 if dt == BF16 else torch.int32),
                       x[x > 0].view(torch.int16 if dt == BF16 else torch.int32)), "subnormals pass unchanged"
    d = ops.act_bwd(torch.ones_like(x), x, ops.ACT_RELU)
    assert torch.equal(d, (x > 0).to(dt))


# ------------------------------------------------------------------------------------------------
# E. fused LayerNorms through identity weights
# ------------------------------------------------------------------------------------------------
def _fused_inputs(fam, m, c, dt, dev):
    # offset at c = 512: the prologue's chain of c / 4 + 2 additions charges the mean of a 100 + 0.5 z row with more
    # than the conditioning cap allows (tests/test_norm_reference_cpu.py); mean 25 there
    return _dev(R.make_inputs(fam, m, c, SEED, dt == BF16, offset=25.0 if c >= 512 else 100.0), dev, dt)


@pytest.mark.parametrize("c,dt", [(128, F32), (256, F32), (128, BF16), (256, BF16), (512, BF16)],
                         ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_rows_linear_layernorm_prologues(dev, c, dt):
    from ptv3_hip import ops
    worst = _Worst()
    eye = torch.eye(c, dtype=dt, device=dev)
    zero = torch.zeros(c, device=dev)
    depth = R.prologue_depth(c)
    for fam in R.FUSED_FAMILIES:
        for m in R.FUSED_ROWS:
            assert ops.rows_linear_capable(c, c, dt, m)
            t = _fused_inputs(fam, m, c, dt, dev)
            tag = f"E rows_linear {fam} c {c} m {m} {_name(dt)}"
            out = ops.rows_linear(t["x"], eye, zero, ln=(t["gamma"], t["beta"]), eps=EPS)
            _check(tag + " ln", "out", out, R.layernorm_f64(t["x"], t["gamma"], t["beta"], EPS),
                   R.forward_bound(t["x"], t["gamma"], t["beta"], EPS, depth=depth, depth_q=depth), dt, worst)
            f1, out = ops.rows_linear(t["x"], eye, zero, ln=(t["gamma2"], t["beta2"]), ln0=(t["gamma"], t["beta"]),
                                      shortcut=t["res"], eps=EPS)
            _check(tag + " ln0", "f1", f1, R.layernorm_f64(t["x"], t["gamma"], t["beta"], EPS, t["res"]),
                   R.forward_bound(t["x"], t["gamma"], t["beta"], EPS, t["res"], depth=depth, depth_q=depth), dt, worst)
            _check(tag + " ln0", "out2", out, R.layernorm_f64(f1, t["gamma2"], t["beta2"], EPS),
                   R.forward_bound(f1, t["gamma2"], t["beta2"], EPS, depth=depth, depth_q=depth), dt, worst)
    print(f"\nNORMPATH E rows_linear prologues c {c} {_name(dt)}: {worst.line()}", end="")


@pytest.mark.parametrize("dt", DTYPES, ids=_name)
@pytest.mark.parametrize("c", (16, 32, 64, 128))
def test_rows_linear_ln_epilogue(dev, c, dt):
    from ptv3_hip import ops
    worst = _Worst()
    eye = torch.eye(c, dtype=dt, device=dev)
    depth = R.epilogue_depth(c)
    for fam in R.FUSED_FAMILIES:
        for m in R.FUSED_ROWS:
            t = _fused_inputs(fam, m, c, dt, dev)
            ref = R.layernorm_f64(t["x"], t["gamma"], t["beta"], EPS)
            E = R.forward_bound(t["x"], t["gamma"], t["beta"], EPS, depth=depth, depth_q=depth)
            tag = f"E rows_linear_ln {fam} c {c} m {m} {_name(dt)}"
            for bias in (None, torch.zeros(c, device=dev)):
                out = ops.rows_linear_ln(t["x"], eye, bias, t["gamma"], t["beta"], EPS, ops.ACT_NONE)
                _check(tag, "out", out, ref, E, dt, worst)
            out = ops.rows_linear_ln(t["x"], eye, None, t["gamma"], t["beta"], EPS, ops.ACT_RELU)
            _check(tag + " relu", "relu", out, ref.clamp_min(0.0), E, dt, worst)
    print(f"\nNORMPATH E rows_linear_ln c {c} {_name(dt)}: {worst.line()}", end="")


# ------------------------------------------------------------------------------------------------
# ops.cast
# ------------------------------------------------------------------------------------------------
def test_cast_bit_exact(dev):
    from ptv3_hip import ops
    # fp32 -> bf16: around every kind of rounding decision
    bits = []
    for hi in (0x3F80, 0x3F81, 0x0001, 0x0000, 0x7F7F, 0x7F00, 0x0080, 0x4049, 0x00FF):
        for lo in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):          # below, at (tie) and above the half way point
            bits += [(hi << 16) | lo, ((hi | 0x8000) << 16) | lo]
    bits += [0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF]
    g = np.random.default_rng(SEED)
    bits = np.concatenate([np.array(bits, dtype=np.uint32), g.integers(0, 1 << 32, 4096, dtype=np.uint32)])
    src = torch.from_numpy(bits.view(np.float32).copy())
    src = src[~torch.isnan(src)]
    ties = (src.view(torch.int32) & 0xFFFF) == 0x8000
    assert ties.any() and ((src.view(torch.int32)[ties] >> 16) & 1).unique().numel() == 2     # ties to even and to odd
    want = src.bfloat16()
    assert torch.isinf(want[src == torch.finfo(torch.float32).max]).all()
    got = ops.cast(src.to(dev), BF16).cpu()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    nan = ops.cast(torch.tensor([float("nan"), 1.0], device=dev), BF16).cpu()
    assert torch.isnan(nan[0]) and nan[1] == 1.0
    # bf16 -> fp32: every bit pattern
    allb = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
    up = ops.cast(allb.to(dev), F32).cpu()
    wantf = allb.float()
    ok = ~torch.isnan(wantf)
    assert torch.equal(up[ok].view(torch.int32), wantf[ok].view(torch.int32))
    assert torch.isnan(up[~ok]).all()
