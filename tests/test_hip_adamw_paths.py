"""GPU tests of the fused AdamW step (adamw_kernel<PTRS>), the weight shadows (shadow_transpose_kernel<E>), the gradient
norm (grad_sq_kernel<PTRS>, sum_partials_kernel) and the table-building host code of ptv3_hip/optim.py, against the
float64 references and the derived per-element bounds of tests/adamw_ref.py (tests/test_adamw_reference_cpu.py shows the
bound is a bound, that it is not slack, and which seeded defect each family catches):

A. one table through FusedAdamW for eight steps: element counts on both sides of the vector trip (1024) and the block
   (4096), every multiple of 4 again with the parameter, the gradient or both one element off alignment (the scalar
   path), five gradient families x five hyperparameter families, two parameter groups, a new gradient tensor each step;
B. tables of 257, 512, 513 and 600 tensors (launches of at most 256 gradient pointers), multi-block tensors across the
   launch boundaries, parameters without a gradient, every gradient x hyperparameter family, three steps;
C. zero-element parameters first, in the middle, last, at table positions 255 and 256 and as a launch of their own,
   every family, three steps;
D. the step-lag branch: own step counts 1, 2, 3, 10, 100, 5000 in one table, loaded from a torch.optim.AdamW state dict;
E. step(grad_scale=...) with the clipping factor of grad_norm(), beside clip_grad_norm_ + torch.optim.AdamW in float64;
F. shadows in fp32 and bf16, bit for bit: partial and full 64 x 64 tiles, kvol 1, 27, 125, unshadowed tensors before,
   between and after, the bf16 rounding decisions, a torch-side in-place change;
G. grad_norm() within its derived bound; H. the rebuild triggers of FusedAdamW._build and its fast path.

Pass criterion unless stated: per element |got - ref64| <= 4 E, the margin of tests/test_hip_norm_paths.py.  The reference
is ONE float64 step from the fp32 state the optimizer held before that step, evaluated on the device in torch float64.
Every parameter is a view into one flat buffer with guard elements around it; the guards keep their canary.

Largest err / E on an MI355X (one run); the bound allows 4:
  group  p      exp_avg  exp_avg_sq
  A      0.789  0.635    0.721     p per family: fork 0.738, fork_clip 0.740, half 0.619, half_b99 0.789, nowd 0.351
  B      0.763  0.651    0.731
  C      0.741  0.627    0.727
  D      0.759  0.592    0.550     own steps 1, 2, 3, 10, 100, 5000 (half 0.637, half_b99 0.759).  With 1 - powf(beta, own)
                                   in the kernel, as it was, p stood at 4.77 in D (half), 4.81 in B and 4.25 in H, wherever a
                                   tensor ran at own step 2 (measured before the fix): outside the bound that A met at 0.79; fixed in csrc/optim.hip
  E      0.607  0.622    0.708     beside clip_grad_norm_ + float64 torch.optim.AdamW: 0.069 of 4 E + 8 u lr (1 + |p|)
  F      0.738  0.494    0.499     shadows bit for bit in every case
  H      0.682  0.491    0.498
  G      grad_norm(): 0.069 of E_norm at most (a worst-case bound of a sum of positive terms)
No figure above 4.  Before the fix of ptv3_adamw_step / ptv3_grad_sqnorm every case of C raised "gradient i is NULL"."""
import ctypes
import math

import numpy as np
import pytest
import torch

import adamw_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 4.0
SEED = 20
STEPS = 8
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


class _Worst:
    """largest err / E per output name"""

    def __init__(self):
        self.v = {}

    def add(self, name, r):
        self.v[name] = max(self.v.get(name, -math.inf), r)

    def line(self):
        return " ".join(f"{k} {v:.3f}" for k, v in self.v.items())


def _check(tag, name, got, ref, E, worst):
    got = got.double()
    assert got.shape == ref.shape, (tag, name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{tag} {name}: non-finite output"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / E.clamp_min(1e-300))     # E = 0: a zero gradient on zero moments
    worst.add(name, ratio.max().item() if ratio.numel() else 0.0)
    bad = err > MARGIN * E
    if bad.any():
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{tag} {name}: {int(bad.sum())} elements outside 4 E; first at {i}: got {got[i].item():.9g} "
                             f"ref {ref[i].item():.9g} err {err[i].item():.3e} E {E[i].item():.3e} "
                             f"worst err / E {ratio.max().item():.2f}")


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]) if ts else torch.empty(0)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


class _Run:
    """a table of adamw_ref as Parameters (views into one flat buffer; a zero-element one is torch.empty(0): its
    data_ptr() is null) in two parameter groups (first half, second half: the device table keeps the order of the
    table), stepped and checked against the one-step reference"""

    def __init__(self, dev, table, hname, seed=SEED, opt_kw=None, extra=()):
        from ptv3_hip.optim import FusedAdamW
        self.dev, self.table, self.seed = dev, list(table), seed
        h = R.HYPERS[hname]
        self.h = h
        self.b1, self.b2, self.eps = R.f32(h["betas"][0]), R.f32(h["betas"][1]), R.f32(h["eps"])
        buf, offs = R.make_params(self.table, seed)
        self.pbuf = torch.from_numpy(buf).to(dev)
        self.owned = self._mask(offs, buf.size)
        self.gown = self._mask(*R.layout(self.table, 1))
        self.params = []
        for (n, _, _), o in zip(self.table, offs):
            self.params.append(torch.nn.Parameter(self.pbuf[o:o + n] if n else torch.empty(0, device=dev)))
        self.params += list(extra)                       # stand-alone tensors (weights with a shadow) after the table
        half = (len(self.params) + 1) // 2
        self.group = [0 if i < half else 1 for i in range(len(self.params))]
        self.lr = [R.f32(h["lr"][g]) for g in self.group]
        self.wd = [R.f32(h["wd"][g]) for g in self.group]
        groups = [dict(params=self.params[:half], lr=h["lr"][0], weight_decay=h["wd"][0])]
        if self.params[half:]:
            groups.append(dict(params=self.params[half:], lr=h["lr"][1], weight_decay=h["wd"][1]))
        self.opt = FusedAdamW(groups, betas=h["betas"], eps=h["eps"], **(opt_kw or {}))
        self.count = [0] * len(self.params)              # own step counts, kept by the test
        self.keep = []                                   # earlier gradient buffers stay alive: every step sees new addresses
        self.nstep = 0

    def _mask(self, offs, total):
        own = np.zeros(total, dtype=bool)
        for (n, _, _), o in zip(self.table, offs):
            own[o:o + n] = True
        return torch.from_numpy(own).to(self.dev)

    def set_grads(self, family, skip=()):
        """a NEW gradient tensor on every parameter (as backward leaves it after zero_grad(set_to_none=True))"""
        self.nstep += 1
        buf, offs = R.make_grads(self.table, family, self.seed, self.nstep)
        gbuf = torch.from_numpy(buf).to(self.dev)
        self.keep.append(gbuf)
        for i, p in enumerate(self.params):
            if i in skip:
                p.grad = None
            elif i < len(self.table):
                n, o = self.table[i][0], offs[i]
                p.grad = gbuf[o:o + n] if n else torch.empty(0, device=self.dev)
            else:
                sc = float(R.grad_scales([(1, 0, 0)] * len(self.params), family, self.seed)[i])
                g = torch.Generator().manual_seed(self.seed * 1000 + self.nstep * 50 + i)
                p.grad = (sc * torch.randn(p.shape, generator=g)).to(self.dev)
        return gbuf

    def _vec(self, vals, live):
        n = torch.tensor([self.params[i].numel() for i in live], device=self.dev)
        return torch.repeat_interleave(torch.tensor([vals[i] for i in live], dtype=torch.float64, device=self.dev), n)

    def step(self, tag, worst, gs=1.0):
        """one optimizer step; p, exp_avg, exp_avg_sq of every parameter with a gradient within 4 E of the reference, the
        others bitwise untouched, the gradients unread-only, every version counter up"""
        live = [i for i, p in enumerate(self.params) if p.grad is not None]
        idle = [i for i in range(len(self.params)) if i not in live]
        ps = [self.params[i] for i in live]
        st = self.opt.state
        P0 = _flat(ps).clone()
        M0 = _flat([st[p]["exp_avg"] if "exp_avg" in st.get(p, {}) else torch.zeros_like(p) for p in ps]).clone()
        V0 = _flat([st[p]["exp_avg_sq"] if "exp_avg_sq" in st.get(p, {}) else torch.zeros_like(p) for p in ps]).clone()
        G = _flat([p.grad for p in ps]).clone()
        idle0 = [self.params[i].detach().clone() for i in idle]
        ver = [p._version for p in ps]
        self.opt.step(grad_scale=gs)
        for i in live:
            self.count[i] += 1
        ref = R.adamw_step_f64(P0, G, M0, V0, self._vec(self.lr, live), self._vec(self.wd, live), self.b1, self.b2,
                               self.eps, R.f32(gs), self._vec(self.count, live))
        _check(tag, "p", _flat(ps), ref["p"], ref["E_p"], worst)
        _check(tag, "exp_avg", _flat([st[p]["exp_avg"] for p in ps]), ref["m"], ref["E_m"], worst)
        _check(tag, "exp_avg_sq", _flat([st[p]["exp_avg_sq"] for p in ps]), ref["v"], ref["E_v"], worst)
        assert torch.equal(_flat([p.grad for p in ps]), G), f"{tag}: a gradient was written"
        assert all(p._version > v for p, v in zip(ps, ver)), f"{tag}: a version counter did not rise"
        for i, before in zip(idle, idle0):
            assert torch.equal(_bits(self.params[i].detach()), _bits(before)), f"{tag}: parameter {i} has no gradient"
        return ref

    def finish(self, tag):
        assert (self.pbuf[~self.owned] == float(R.CANARY)).all(), f"{tag}: a guard element of the parameter buffer changed"
        for gbuf in self.keep:
            assert (gbuf[~self.gown] == float(R.CANARY)).all(), f"{tag}: a guard element of a gradient buffer changed"
        sd = self.opt.state_dict()["state"]
        for i, c in enumerate(self.count):
            if c:
                assert float(sd[i]["step"]) == float(c), (tag, i, float(sd[i]["step"]), c)

    def state_bits(self):
        st = self.opt.state
        return [_bits(t.detach()).clone() for p in self.params if p in st
                for t in (p, st[p]["exp_avg"], st[p]["exp_avg_sq"])]


# ------------------------------------------------------------------------------------------------
# A. one table, eight steps
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hname", list(R.HYPERS))
def test_step_every_count_alignment_and_family(dev, hname):
    worst = _Worst()
    gs = R.HYPERS[hname]["gs"]
    for gname in R.GRAD_FAMILIES:
        runs = []
        for rep in range(2 if gname in ("normal", "mixed") else 1):
            run = _Run(dev, R.table_counts(), hname)
            for k in range(STEPS):
                run.set_grads(gname)
                run.step(f"A {hname} {gname} step {k + 1}", worst if rep == 0 else _Worst(), gs)
            run.finish(f"A {hname} {gname}")
            runs.append(run.state_bits())
        if len(runs) == 2:           # two identical runs are bitwise equal
            assert all(torch.equal(a, b) for a, b in zip(*runs)), f"A {hname} {gname}: two runs differ"
    print(f"\nADAMWPATH A {hname}: {worst.line()}", end="")


# ------------------------------------------------------------------------------------------------
# B. more than 256 tensors
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", R.LARGE_TABLES)
def test_step_large_tables(dev, nt):
    worst = _Worst()
    table = R.table_large(nt)
    assert R.blocks_of([n for n, _, _ in table]) > nt and len(table) == nt
    for hname in R.HYPERS:
        for gname in R.GRAD_FAMILIES:
            run = _Run(dev, table, hname)
            gs = R.HYPERS[hname]["gs"]
            # step 2: parameters without a gradient on both sides of the launch boundaries and at the table's ends; they
            # are untouched, their neighbours are right, and at step 3 they take the step-lag branch
            idle = {0, 100, 254, 255, 256, 257, nt - 1} & set(range(nt))
            for k in range(3):
                run.set_grads(gname, skip=idle if k == 1 else ())
                run.step(f"B nt {nt} {hname} {gname} step {k + 1}", worst, gs)
            assert [run.count[i] for i in sorted(idle)] == [2] * len(idle)
            run.finish(f"B nt {nt} {hname} {gname}")
    print(f"\nADAMWPATH B tensors {nt}: {worst.line()}", end="")


# ------------------------------------------------------------------------------------------------
# C. zero-element parameters
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", R.EMPTY_PLACES)
def test_step_zero_element_parameters(dev, place):
    worst = _Worst()
    table = R.table_with_empty(place)
    empty = [i for i, (n, _, _) in enumerate(table) if n == 0]
    assert empty
    for hname in R.HYPERS:
        for gname in R.GRAD_FAMILIES:
            run = _Run(dev, table, hname)
            assert all(run.params[i].data_ptr() == 0 for i in empty)
            for k in range(3):
                run.set_grads(gname)
                want = _flat([p.grad for p in run.params]).double().pow(2).sum().sqrt().item()
                got = run.opt.grad_norm().item()
                assert abs(got - want) <= R.grad_norm_bound(want, R.blocks_of([n for n, _, _ in table]))
                run.step(f"C {place} {hname} {gname} step {k + 1}", worst, R.HYPERS[hname]["gs"])
            run.finish(f"C {place} {hname} {gname}")
            sd = run.opt.state_dict()["state"]
            assert all(float(sd[i]["step"]) == 3.0 for i in empty), "an empty parameter keeps a step count, as in torch"
    print(f"\nADAMWPATH C empty {place}: {worst.line()}", end="")


def test_only_zero_element_parameters(dev):
    from ptv3_hip.optim import FusedAdamW
    p = torch.nn.Parameter(torch.empty(0, device=dev))
    p.grad = torch.empty(0, device=dev)
    opt = FusedAdamW([p], lr=1e-3)
    assert opt.grad_norm().item() == 0.0
    opt.step()
    opt.step()
    assert float(opt.state_dict()["state"][0]["step"]) == 2.0


def test_null_gradient_of_a_nonempty_tensor_is_refused(dev):
    """ptv3_adamw_step / ptv3_grad_sqnorm: a NULL gradient address passes for a tensor that owns no block only"""
    from ptv3_hip.lib import lib
    from ptv3_hip.ops import _stream
    run = _Run(dev, [(64, 0, 0), (0, 0, 0), (5000, 0, 0)], "fork")
    run.set_grads("normal")
    run.step("C refusal", _Worst())
    opt = run.opt
    before = [p.detach().clone() for p in run.params]
    lr = (ctypes.c_float * 2)(1e-3, 1e-3)
    out = torch.zeros(1, device=dev)
    for null in (0, 2):
        ptrs = [p.grad.data_ptr() for p in run.params]
        ptrs[null] = 0
        arr = (ctypes.c_void_p * 3)(*ptrs)
        rc = lib.ptv3_adamw_step(opt._table.data_ptr(), opt._nt, opt._nb, lr, lr, 2, 0.9, 0.999, 1e-8, 2, 1.0,
                                 opt._first_blocks, arr, 0, 0, _stream())
        assert rc != 0 and b"NULL" in lib.ptv3_last_error()
        rc = lib.ptv3_grad_sqnorm(opt._table.data_ptr(), opt._nt, opt._nb, opt._partial.data_ptr(), out.data_ptr(),
                                  opt._first_blocks, arr, _stream())
        assert rc != 0 and b"NULL" in lib.ptv3_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(a.detach(), b) for a, b in zip(run.params, before)), "a refused call must not launch"


# ------------------------------------------------------------------------------------------------
# D. step lag
# ------------------------------------------------------------------------------------------------
LAG_TABLE = [(1025, 0, 0), (4096, 0, 0), (64, 0, 0), (4097, 0, 0), (1020, 1, 0), (8192, 0, 0),
             (3, 0, 0), (4100, 0, 1), (12289, 0, 0), (1, 0, 0), (1024, 0, 0), (4095, 0, 0)]
LAG_OWN = [1, 2, 3, 10, 100, 5000, 1, 2, 5000, 10, 3, 100]        # the own count of the first step taken here


@pytest.mark.parametrize("hname", ("half", "half_b99"))
def test_step_lag_branch(dev, hname):
    """tensors resumed from a torch.optim.AdamW state dict at their own step counts beside fresh ones: the launch's step
    is the largest count, every other tensor takes the step-lag branch.  The same 4 E as A."""
    worst = _Worst()
    h = R.HYPERS[hname]
    for gname in ("normal", "mixed"):
        run = _Run(dev, LAG_TABLE, hname)
        half = (len(run.params) + 1) // 2
        topt = torch.optim.AdamW([dict(params=run.params[:half], lr=h["lr"][0], weight_decay=h["wd"][0]),
                                  dict(params=run.params[half:], lr=h["lr"][1], weight_decay=h["wd"][1])],
                                 betas=h["betas"], eps=h["eps"])
        sc = R.grad_scales(LAG_TABLE, gname, SEED)
        g = torch.Generator().manual_seed(SEED)
        for i, (p, own) in enumerate(zip(run.params, LAG_OWN)):
            if own > 1:
                topt.state[p] = dict(step=torch.tensor(float(own - 1)),
                                     exp_avg=(0.3 * sc[i] * torch.randn(p.shape, generator=g)).to(dev),
                                     exp_avg_sq=(sc[i] ** 2 * (0.25 + torch.rand(p.shape, generator=g))).to(dev))
                run.count[i] = own - 1
        run.opt.load_state_dict(topt.state_dict())
        for k in range(2):
            run.set_grads(gname)
            run.step(f"D {hname} {gname} step {k + 1}", worst, h["gs"])
        assert run.count == [o + 1 for o in LAG_OWN]
        run.finish(f"D {hname} {gname}")
    print(f"\nADAMWPATH D lag {hname}: {worst.line()}", end="")


# ------------------------------------------------------------------------------------------------
# E. grad_scale
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gname", ("normal", "large", "tiny"))
def test_grad_scale_is_clip_grad_norm(dev, gname):
    """step(grad_scale=s), s = min(1, max_norm / (grad_norm() + 1e-6)) (clip_grad_norm_'s factor): the reference fed s g,
    and, for the first step from zero moments, clip_grad_norm_ + torch.optim.AdamW in float64 on the decimal
    hyperparameters within 4 E + 8 u lr (1 + |p|): the fp32 rounding of lr, weight_decay, betas, eps and s and the fp32
    error of the norm each move a step of at most lr by a few u of it."""
    worst = _Worst()
    hname, max_norm = "half", 1.0
    h = R.HYPERS[hname]
    run = _Run(dev, R.table_counts(), hname)
    for k in range(3):
        run.set_grads(gname)
        s = min(1.0, max_norm / (run.opt.grad_norm().item() + 1e-6))
        assert (s < 1.0) == (gname != "tiny")
        if k == 0:
            twins = [torch.nn.Parameter(p.detach().double().clone()) for p in run.params]
            for t, p in zip(twins, run.params):
                t.grad = p.grad.double().clone()
            half = (len(twins) + 1) // 2
            topt = torch.optim.AdamW([dict(params=twins[:half], lr=h["lr"][0], weight_decay=h["wd"][0]),
                                      dict(params=twins[half:], lr=h["lr"][1], weight_decay=h["wd"][1])],
                                     betas=h["betas"], eps=h["eps"])
            torch.nn.utils.clip_grad_norm_(twins, max_norm)
            topt.step()
        ref = run.step(f"E {gname} step {k + 1}", worst, s)
        if k == 0:
            P = _flat(run.params).double()
            lr = run._vec(run.lr, range(len(run.params)))
            figure = MARGIN * ref["E_p"] + 8 * R.U * lr * (1 + P.abs())
            gap = (P - _flat(twins)).abs()
            worst.add("torch64/figure", (gap / figure).max().item())
            assert (gap <= figure).all(), (gap / figure).max().item()
    run.finish(f"E {gname}")
    print(f"\nADAMWPATH E grad_scale {gname}: {worst.line()}", end="")


# ------------------------------------------------------------------------------------------------
# F. shadows
# ------------------------------------------------------------------------------------------------
def _check_shadows(tag, params, dt):
    from ptv3_hip.optim import weight_shadow
    n = 0
    for i, p in enumerate(params):
        if not R.shadowed(tuple(p.shape)):
            assert not hasattr(p, "_ptv3_shadow"), (tag, i)
            continue
        sh = weight_shadow(p, dt)
        assert sh is not None, f"{tag}: the shadow of tensor {i} {tuple(p.shape)} is stale"
        nat, tr = R.shadow_nat(p, dt), R.shadow_t(p, dt)
        assert sh["nat"].shape == nat.shape and sh["t"].shape == tr.shape
        assert torch.equal(_bits(sh["nat"]), _bits(nat)), f"{tag}: natural shadow of tensor {i} {tuple(p.shape)}"
        assert torch.equal(_bits(sh["t"]), _bits(tr)), f"{tag}: transposed shadow of tensor {i} {tuple(p.shape)}"
        n += 1
    return n


@pytest.mark.parametrize("dt", (F32, BF16), ids=("fp32", "bf16"))
@pytest.mark.parametrize("order", (0, 1, 2))
def test_shadows_bit_for_bit(dev, dt, order):
    from ptv3_hip.optim import weight_shadow
    worst = _Worst()
    shapes = R.shadow_orders()[order]
    g = torch.Generator().manual_seed(SEED + order)
    extra = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]
    run = _Run(dev, [], "fork", opt_kw=dict(shadow_dtype=dt), extra=extra)
    for k in range(3):
        run.set_grads("normal")
        run.step(f"F order {order} step {k + 1}", worst)
        assert _check_shadows(f"F order {order} step {k + 1}", extra, dt) == len(R.SHADOW_WEIGHTS)
    # a torch-side in-place change: the shadow is stale until the next step has rewritten it
    w = next(p for p in extra if p.dim() == 3 and R.shadowed(tuple(p.shape)))
    with torch.no_grad():
        w.mul_(1.5)
    assert weight_shadow(w, dt) is None
    run.set_grads("normal")
    run.step(f"F order {order} after mul_", worst)
    assert _check_shadows(f"F order {order} after mul_", extra, dt) == len(R.SHADOW_WEIGHTS)
    print(f"\nADAMWPATH F shadows order {order} {'fp32' if dt == F32 else 'bf16'}: {worst.line()}", end="")


@pytest.mark.parametrize("misaligned", (False, True), ids=("vector", "scalar"))
def test_bf16_shadow_rounding_decisions(dev, misaligned):
    """lr = 0, wd = 0: the step leaves p as it is, and the shadow must be p.to(bfloat16) for chosen values: ties with an
    even and an odd kept bit, their fp32 neighbours, subnormals, +-0, the largest finite values.  The vector path packs
    with pack4<__bf16>, the scalar path (a parameter one element off alignment) casts with (__bf16)."""
    from ptv3_hip.optim import FusedAdamW
    v = torch.from_numpy(R.bf16_edge_values()).to(dev)
    buf = torch.zeros(v.numel() + 8, device=dev)
    off = 1 if misaligned else 0
    buf[off:off + v.numel()] = v
    g = torch.Generator().manual_seed(SEED)
    for shape in ((64, 8), (8, 64), (8, 1, 1, 8, 8)):
        p = torch.nn.Parameter(buf[off:off + v.numel()].view(shape))
        assert (p.data_ptr() % 16 != 0) == misaligned
        opt = FusedAdamW([p], lr=0.0, weight_decay=0.0, shadow_dtype=BF16)
        before = p.detach().clone()
        for k in range(2):
            p.grad = torch.randn(shape, generator=g).to(dev)
            opt.step()
            nz = before != 0
            assert torch.equal(_bits(p.detach())[nz], _bits(before)[nz]), "lr = 0, wd = 0 must leave p bit for bit"
            assert (p.detach()[~nz] == 0).all()
            assert _check_shadows(f"F edge {shape} {'scalar' if misaligned else 'vector'}", [p], BF16) == 1
        want = before.to(BF16).reshape(p._ptv3_shadow["nat"].shape)
        assert torch.equal(_bits(p._ptv3_shadow["nat"])[nz.reshape(want.shape)], _bits(want)[nz.reshape(want.shape)])


# ------------------------------------------------------------------------------------------------
# G. grad_norm()
# ------------------------------------------------------------------------------------------------
def _norm_tables():
    t = {"counts": R.table_counts()}
    t.update({f"t{n}": R.table_large(n) for n in R.LARGE_TABLES})
    t.update({f"empty_{place}": R.table_with_empty(place) for place in R.EMPTY_PLACES})
    return t


def test_grad_norm_within_its_bound(dev):
    worst = 0.0
    for tname, table in _norm_tables().items():
        blocks = R.blocks_of([n for n, _, _ in table])
        run = _Run(dev, table, "fork")
        for gname in R.GRAD_FAMILIES:
            run.set_grads(gname)
            live = [p.grad for p in run.params]
            want = _flat(live).double().pow(2).sum().sqrt().item()
            got = run.opt.grad_norm()
            assert torch.equal(got, run.opt.grad_norm()) and torch.equal(got, run.opt.grad_norm()), "repeated calls"
            if gname == "zero":
                assert got.item() == 0.0 and want == 0.0
                continue
            E = R.grad_norm_bound(want, blocks)
            worst = max(worst, abs(got.item() - want) / E)
            assert abs(got.item() - want) <= E, (tname, gname, got.item(), want, E)
        if tname == "t600":
            assert blocks > 2 * 256          # the second stage adds more than one partial per thread
    print(f"\nADAMWPATH G grad_norm: largest err / E_norm {worst:.3f}", end="")


def test_grad_norm_without_gradients(dev):
    from ptv3_hip.optim import FusedAdamW
    ps = [torch.nn.Parameter(torch.randn(n, device=dev)) for n in (5, 4097)]
    opt = FusedAdamW(ps, lr=1e-3)
    assert opt.grad_norm().item() == 0.0
    before = [p.detach().clone() for p in ps]
    opt.step()
    assert all(torch.equal(a.detach(), b) for a, b in zip(ps, before))
    ps[1].grad = torch.full((4097,), 2.0, device=dev)
    assert opt.grad_norm().item() == pytest.approx(2.0 * math.sqrt(4097), rel=1e-6)
    ps[1].grad = None
    assert opt.grad_norm().item() == 0.0


# ------------------------------------------------------------------------------------------------
# H. table reuse
# ------------------------------------------------------------------------------------------------
def test_table_reuse_and_rebuild_triggers(dev, monkeypatch):
    from ptv3_hip.lib import lib
    from ptv3_hip.optim import weight_shadow
    worst = _Worst()
    fills = [0]
    real = lib.ptv3_adamw_fill_entry

    def counted(*a):
        fills[0] += 1
        return real(*a)

    monkeypatch.setattr(lib, "ptv3_adamw_fill_entry", counted, raising=False)
    table = [(1025, 0, 0), (4096, 0, 0), (64, 0, 0), (4100, 1, 0), (8, 0, 0)]
    g = torch.Generator().manual_seed(SEED)
    w = torch.nn.Parameter(torch.randn((72, 27, 40), generator=g).to(dev))
    run = _Run(dev, table, "half", opt_kw=dict(shadow_dtype=BF16), extra=[w])
    n = len(run.params)

    def go(tag, skip=(), fresh=True):
        if fresh:
            run.set_grads("normal", skip=skip)
        run.step(f"H {tag}", worst)
        assert _check_shadows(f"H {tag}", [w], BF16) == 1

    go("first")
    assert fills[0] == n
    go("unchanged")
    go("unchanged again")
    assert fills[0] == n, "new gradient addresses alone must take the fast path"
    go("a parameter lost its gradient", skip={1})
    assert fills[0] == 2 * n - 1
    go("and has it again")
    assert fills[0] == 3 * n - 1 and run.count[1] == run.count[0] - 1
    run.params[2].data = run.params[2].data.clone()               # p.data replaced: a new address, the moments stay
    go("p.data replaced")
    assert fills[0] == 4 * n - 1
    late = torch.nn.Parameter(torch.randn(4097, generator=g).to(dev))
    run.opt.add_param_group(dict(params=[late]))
    run.params.append(late); run.count.append(0); run.group.append(2)
    run.lr.append(R.f32(run.opt.param_groups[2]["lr"])); run.wd.append(R.f32(run.opt.param_groups[2]["weight_decay"]))
    go("add_param_group")
    assert fills[0] == 5 * n and run.count[-1] == 1
    run.opt.zero_grad(set_to_none=False)                          # the same gradient tensors, zeroed
    assert all(p.grad is not None and not p.grad.any() for p in run.params)
    go("zero_grad(set_to_none=False)", fresh=False)
    assert fills[0] == 5 * n
    with torch.no_grad():
        w.add_(0.25)
    assert weight_shadow(w, BF16) is None
    go("after a torch-side add_")
    run.finish("H")
    assert run.count == [9, 8, 9, 9, 9, 9, 3]
    print(f"\nADAMWPATH H table reuse: {worst.line()}", end="")
