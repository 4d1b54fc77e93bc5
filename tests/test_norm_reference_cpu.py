"""CPU checks of tests/norm_ref.py, the yardstick of tests/test_hip_norm_paths.py (no GPU):

- the fp32 emulation of the kernels' summation order stays within 1 E of the float64 reference for every input family
  and every width of the GPU file (so E is a bound, and the ratios show it is not a slack one);
- conditioning caps: E itself is small against the outputs, or 4 E would tolerate an O(1) error;
- seeded defects in the emulation exceed 4 E on at least one family (CAUGHT_BY records which);
- the width lists of the GPU file reach every kernel variant the launchers can choose.

Measured here (emulation error / E; the printed lines give it per width and family): forward y 0.09 .. 0.98 (the
largest with `small_gamma` and `tiny`), chained y2 0.12 .. 0.49, backward dx up to 0.99 (`outlier` and `huge`: rstd is
tiny there, dx = add + rstd t is the rounding of that one addition, u |dx|, which is then all of E), dgamma <= 0.16,
dbeta <= 0.07; the largest E is 0.25 of the 2^-10 cap in the forward.  Smallest err / E over the widths of a seeded defect,
per family (a defect must exceed 4):
  forward   onepass      offset 83; every other family < 1 (`huge` reaches 3.2 at c = 8)
            cplus1       every family >= 32
            bf16_stats   every family >= 107
            no_eps       const 8.3e3, tiny 4.4e7; the others < 3
            gamma_shift  every family >= 1.5e4, small_gamma 3.9e9
            skip_ragged  every family >= 70 (at the widths that have a ragged round: 48, 96, 192, 384, 1028)
  backward  cplus1       every family >= 124
            no_eps       const 9.9e9, tiny 4.3e7, offset 8.6; the others < 5
            gamma_shift  every family >= 1e5
            no_s2        every family >= 267
            add_twice    every family >= 1.2e4
"""
import numpy as np
import pytest

import norm_ref as R

FAMS = R.FAMILIES
SEED = 20


def _ratio(got, ref, E):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got.astype(np.float64) - ref) / np.maximum(E, 1e-300)     # E = 0: dgamma at c = 1
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r.max())


def _fwd_case(fam, m, c, bf16=False):
    d = R.make_inputs(fam, m, c, SEED, bf16)
    ref = R.layernorm_f64(d["x"], d["gamma"], d["beta"], res=d["res"])
    E = R.forward_bound(d["x"], d["gamma"], d["beta"], res=d["res"])
    return d, ref, E


@pytest.mark.parametrize("c", R.FWD_WIDTHS)
def test_forward_emulation_within_bound_and_caps(c):
    m = 301
    line = []
    for fam in FAMS:
        d, ref, E = _fwd_case(fam, m, c)
        y, y2 = R.layernorm_emulated(d["x"], d["gamma"], d["beta"], res=d["res"], gamma2=d["gamma2"], beta2=d["beta2"])
        r1 = _ratio(y, ref, E)
        # the chained norm: reference and bound from the stored y
        ref2 = R.layernorm_f64(y, d["gamma2"], d["beta2"])
        E2 = R.forward_bound(y, d["gamma2"], d["beta2"])
        r2 = _ratio(y2, ref2, E2)
        cap1 = E.max() / max(1.0, np.abs(ref).max())
        cap2 = E2.max() / max(1.0, np.abs(ref2).max())
        line.append(f"{fam} y {r1:.2f} y2 {r2:.2f} cap {max(cap1, cap2) * 1024:.2f}")
        assert r1 <= 1.0 and r2 <= 1.0, (fam, c, r1, r2)
        assert cap1 <= 2.0 ** -10 and cap2 <= 2.0 ** -10, (fam, c, cap1, cap2)
    print(f"\nNORMREF fwd c {c} lpr {R.forward_lpr(c)} depth {R.forward_depth(c)} (err/E, cap in units of 2^-10): "
          + "; ".join(line), end="")


@pytest.mark.parametrize("c", R.BWD_WIDTHS)
def test_backward_emulation_within_bound_and_caps(c):
    line = []
    for m in (17, 301, 4097):
        for fam in FAMS if m != 4097 else ("randn", "const"):
            d = R.make_bwd_inputs(fam, m, c, SEED)
            ref = R.layernorm_bwd_f64(d["x"], d["dy"], d["gamma"], add=d["add"])
            E = R.backward_bound(d["x"], d["dy"], d["gamma"], add=d["add"])
            got = R.layernorm_bwd_emulated(d["x"], d["dy"], d["gamma"], add=d["add"])
            rs = [_ratio(g, r, e) for g, r, e in zip(got, ref, E)]
            caps = [e.max() / max(1.0, np.abs(r).max()) for r, e in zip(ref, E)]
            line.append(f"{fam}/{m} dx {rs[0]:.2f} dg {rs[1]:.2f} db {rs[2]:.2f}")
            assert max(rs) <= 1.0, (fam, m, c, rs)
            assert caps[0] <= 2.0 ** -10 and max(caps[1:]) <= 2.0 ** -7, (fam, m, c, caps)
    print(f"\nNORMREF bwd c {c} variant {R.backward_variant(c)} (err/E): " + "; ".join(line), end="")


def test_bf16_emulation_within_bound_plus_ulp():
    """the bf16 template: inputs rounded to bf16 first, output rounded once: within E + half an output ulp"""
    for c in (48, 256, 1028):
        for fam in FAMS:
            d, ref, E = _fwd_case(fam, 65, c, bf16=True)
            y = R.layernorm_emulated(d["x"], d["gamma"], d["beta"], res=d["res"], bf16=True)
            assert (np.abs(y - ref) <= E + R.ulp(ref, True)).all(), (fam, c)


# which families a seeded defect must be caught by (err > 4 E somewhere); checked below, at every width where the
# defect changes anything
CAUGHT_BY = {
    ("fwd", "onepass"): ("offset",),
    ("fwd", "cplus1"): ("randn", "offset", "huge", "small_gamma"),
    ("fwd", "bf16_stats"): ("randn", "offset", "tiny"),
    ("fwd", "no_eps"): ("const", "tiny"),
    ("fwd", "gamma_shift"): ("randn", "small_gamma"),
    ("fwd", "skip_ragged"): ("randn", "offset", "const"),
    ("bwd", "cplus1"): ("randn", "offset"),
    ("bwd", "no_eps"): ("const", "tiny"),
    ("bwd", "gamma_shift"): ("randn", "small_gamma"),
    ("bwd", "no_s2"): ("randn", "small_gamma"),
    ("bwd", "add_twice"): ("randn", "const", "tiny"),
}


@pytest.mark.parametrize("defect", R.FWD_DEFECTS)
def test_forward_defect_exceeds_bound(defect):
    widths = [c for c in R.FWD_WIDTHS if c >= 8]
    if defect == "skip_ragged":
        widths = [c for c in R.FWD_WIDTHS if (c // 4) % R.forward_lpr(c)]
        assert set(widths) >= {48, 96, 192, 384, 1028}
    report = []
    for c in widths:
        caught = {}
        for fam in FAMS:
            d, ref, E = _fwd_case(fam, 64, c)
            y = R.layernorm_emulated(d["x"], d["gamma"], d["beta"], res=d["res"], defect=defect)
            caught[fam] = _ratio(y, ref, E)
        assert all(caught[f] > 4.0 for f in CAUGHT_BY["fwd", defect]), (defect, c, caught)
        report.append(f"c {c}: " + " ".join(f"{f} {min(r, 9.9e9):.3g}" for f, r in caught.items()))
    print(f"\nNORMREF defect fwd/{defect} err/E: " + "; ".join(report), end="")


@pytest.mark.parametrize("defect", R.BWD_DEFECTS)
def test_backward_defect_exceeds_bound(defect):
    report = []
    for c in (32, 48, 96, 192, 384, 768):
        caught = {}
        for fam in FAMS:
            d = R.make_bwd_inputs(fam, 64, c, SEED)
            ref = R.layernorm_bwd_f64(d["x"], d["dy"], d["gamma"], add=d["add"])
            E = R.backward_bound(d["x"], d["dy"], d["gamma"], add=d["add"])
            got = R.layernorm_bwd_emulated(d["x"], d["dy"], d["gamma"], add=d["add"], defect=defect)
            caught[fam] = max(_ratio(g, r, e) for g, r, e in zip(got, ref, E))
        assert all(caught[f] > 4.0 for f in CAUGHT_BY["bwd", defect]), (defect, c, caught)
        report.append(f"c {c}: " + " ".join(f"{f} {min(r, 9.9e9):.3g}" for f, r in caught.items()))
    print(f"\nNORMREF defect bwd/{defect} err/E: " + "; ".join(report), end="")


def test_fused_kernel_caps():
    """the fused kernels' longer chains (rows_linear prologue c / 4 + 2, rows_linear_ln epilogue cout / 16 + 4) at the
    shapes of group E: the same conditioning caps; the offset family takes mean 25 at c = 512"""
    shapes = [(c, R.prologue_depth(c)) for c in (128, 256, 512)] + [(c, R.epilogue_depth(c)) for c in (16, 32, 64, 128)]
    for c, depth in shapes:
        for fam in R.FUSED_FAMILIES:
            d = R.make_inputs(fam, 301, c, SEED, offset=25.0 if c >= 512 else 100.0)
            ref = R.layernorm_f64(d["x"], d["gamma"], d["beta"], res=d["res"])
            E = R.forward_bound(d["x"], d["gamma"], d["beta"], res=d["res"], depth=depth, depth_q=depth)
            cap = E.max() / max(1.0, np.abs(ref).max())
            assert cap <= 2.0 ** -10, (fam, c, depth, cap)


def test_references_run_on_torch_tensors():
    """the GPU file evaluates the same formulas in torch float64"""
    import torch
    d = R.make_bwd_inputs("offset", 33, 48, SEED)
    t = {k: torch.from_numpy(v) for k, v in d.items()}
    for f, args in ((R.layernorm_f64, ("x", "gamma", "beta")), (R.forward_bound, ("x", "gamma", "beta"))):
        a = f(*[d[k] for k in args], res=d["res"])
        b = f(*[t[k] for k in args], res=t["res"])
        assert np.allclose(a, b.numpy(), rtol=1e-12, atol=0)
    for f in (R.layernorm_bwd_f64, R.backward_bound):
        for a, b in zip(f(d["x"], d["dy"], d["gamma"], add=d["add"]), f(t["x"], t["dy"], t["gamma"], add=t["add"])):
            assert np.allclose(a, b.numpy(), rtol=1e-9, atol=0)
    v = np.array([0.0, 1e-45, 1e-39, 0.99, 1.0, 3.0, 1e30])
    assert (R.ulp(v, True) == R.ulp(torch.from_numpy(v), True).numpy()).all()
    assert R.ulp(1.0, False) == 2.0 ** -23 and R.ulp(0.99, True) == 2.0 ** -8 and R.ulp(0.0, False) == 2.0 ** -149


def test_kernel_order_bound_is_tighter_than_generic_depth():
    """depth = c would be several times looser at the wide rows"""
    d, ref, E = _fwd_case("offset", 16, 2048)
    loose = R.forward_bound(d["x"], d["gamma"], d["beta"], res=d["res"], depth=2048, depth_q=2048)
    assert np.median(loose / E) > 5.0


def test_variant_coverage():
    assert {R.forward_lpr(c) for c in R.FWD_WIDTHS} == {1, 2, 4, 8, 16, 32, 64}
    # ragged rounds (not every lane holds a chunk) and full multi-chunk rows
    assert any((c // 4) % 64 and c > 256 for c in R.FWD_WIDTHS) and R.forward_rounds(2048) == R.LN_MAXCH
    assert R.forward_rounds(1028) == 5 and R.forward_rounds(384) == 2
    assert all(c % 4 == 0 and c <= 2048 for c in R.FWD_WIDTHS)
    # rows-per-block edges at c = 4 (LPR 1: 256 rows per block)
    assert {255, 256, 257} <= set(R.FWD_ROWS)
    assert {R.backward_variant(c) for c in R.BWD_WIDTHS} == {"packed", 1, 2, 4, 8, 16}
    assert [c for c in R.BWD_WIDTHS if R.backward_variant(c) == "packed"] == [32, 64, 128, 256]
    assert {R.backward_variant(c) for c in R.SWIN_WIDTHS} == {1, 2, 4, 8}
    assert all(R.backward_variant(c) != "packed" for c in (16, 48, 512))
    # both col_chunks regimes, a partial, an exact and a ragged second chunk
    assert R.row_chunks(15) == (16, 1) and R.row_chunks(16) == (16, 1) and R.row_chunks(17) == (16, 2)
    assert R.row_chunks(4096) == (16, 256) and R.row_chunks(4097) == (20, 205)
    assert {R.row_chunks(m)[0] for m in R.BWD_ROWS} == {16, 20}
    assert max(R.BWD_ROWS) <= 4097 and max(R.FWD_WIDTHS) <= 2048


def test_gelu_reference_and_grid():
    g = R.gelu_grid()
    assert g.dtype == np.float32 and g.size == 65280 + R.DENSE_POINTS and g.size % 128 == 0
    assert np.isfinite(g).all() and R.bf16_values().size == 65280
    assert (R.round_bf16(R.bf16_values()) == R.bf16_values()).all()
    assert np.abs(g).max() > 3e38 and (np.abs(g[np.abs(g) > 0]).min() < 1e-38)
    x = np.array([-30.0, -6.0, -1.0, 0.0, 0.5, 1.0, 6.0])
    # Phi from math.erfc; the negative tail keeps its relative accuracy
    import math
    want = np.array([v * 0.5 * math.erfc(-v / math.sqrt(2.0)) for v in x])
    assert np.allclose(R.gelu_f64(x), want, rtol=1e-14, atol=0)
    assert R.gelu_f64(np.array([-30.0]))[0] < 0.0
    # derivative against a central difference of the value
    xs = np.linspace(-6, 6, 241)
    h = 1e-5
    fd = (R.gelu_f64(xs + h) - R.gelu_f64(xs - h)) / (2 * h)
    assert np.abs(fd - R.gelu_grad_f64(xs)).max() < 1e-9
