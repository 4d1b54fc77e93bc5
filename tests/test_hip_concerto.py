"""GPU tests of Concerto's image branch: the kernels of csrc/concerto.hip against tests/concerto_ref.py in float64, and the
model "Concerto-v1m1" against the reference's fixture (tests/golden/concerto_tiny.npz).

Kernel tolerances follow the project's rule (DESIGN.md sections 13 - 15, the check() of test_hip_sonata.py): the kernel's
largest error against the float64 yardstick may be at most four times that of the reference's LITERAL formulation
(concerto_ref: sort and per-image segment sums; gather, dense scatter_mean, select; shift, CosineSimilarity, mean)
evaluated by torch in float32 on the device, with a floor of 8 float32 ulps of the tensor's largest entry.  With bf16
inputs both sides start from the same rounded input; a gradient, which the kernel writes in the input's dtype, is then
compared with the float32 run's gradient rounded to bf16 once as well.  Model tolerances are four times the fixture's
stored fp32-vs-float64 gap of the same tensor with the floor of one fp32 rounding at the tensor's scale; a gradient,
stored as float16 of grad / max|grad|, is also allowed the float16 step of its stored value.

Inputs never hold a pair with exactly one entry -1 at the level the plan reads: it passes the reference's "any" test, and
the reference then truncates -1 into its patch index, which points into a neighbouring patch or out of range.  The
pooling itself is tested with such children, since its count ("both") and its sum (elementwise) differ exactly there."""
import functools

import numpy as np
import pytest
import torch

import concerto_ref as R

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]


def check(name, got, ref64, ref32):
    ref64 = ref64.detach().cpu().double()
    err_k = (got.detach().cpu().double() - ref64).abs().max().item()
    err_t = (ref32.detach().cpu().double() - ref64).abs().max().item()
    top = ref64.abs().max().item()
    bound = max(4.0 * err_t, 8.0 * ULP * top)
    print(f"{name}: kernel {err_k:.3e} torch-fp32 {err_t:.3e} max|ref| {top:.3e} bound {bound:.3e}")
    assert err_k <= bound, (name, err_k, err_t, top)


# ---- correspondence pooling -------------------------------------------------------------------------------------------
def pooling(n_out, sizes, g):
    """(inverse (n_in), order (n_in), idx_ptr (n_out + 1)) of a pooling whose cluster c has sizes[c] children, scattered"""
    inverse = torch.repeat_interleave(torch.arange(n_out), sizes)
    inverse = inverse[torch.randperm(inverse.shape[0], generator=g)]
    order = torch.sort(inverse, stable=True)[1]
    return inverse, order, torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(sizes, 0)])


def level0(n, v, g, cells=37):
    """integer pixel cells, a third of the pairs (-1, -1), and children with exactly one entry -1"""
    corr = torch.randint(0, cells, (n, v, 2), generator=g).double()
    corr[torch.rand(n, v, generator=g) < 0.33] = -1
    half = torch.rand(n, v, generator=g) < 0.1
    corr[..., 1][half] = -1
    return corr


def run_pool(corr, order, idx_ptr):
    from ptv3_hip import ops
    return ops.concerto_pool_corr(corr.to(DEV), order.to(DEV), idx_ptr.int().to(DEV))


@pytest.mark.parametrize("v", [1, 3])
@pytest.mark.parametrize("n_out", [1, 65, 300])
def test_pool_corr(n_out, v):
    g = torch.Generator().manual_seed(100 * n_out + v)
    sizes = torch.randint(1, 9, (n_out,), generator=g)
    sizes[0] = 5
    inverse, order, idx_ptr = pooling(n_out, sizes, g)
    corr = level0(inverse.shape[0], v, g)
    corr[inverse == 0] = -1                                     # a cluster with every child invalid
    first = int((inverse == n_out - 1).nonzero()[0])            # and one whose only set entries stand beside a -1
    corr[inverse == n_out - 1] = -1
    if n_out > 1:
        corr[first, :, 0] = 7.0
    want = R.pool_level(corr, inverse, idx_ptr)
    fp32 = R.pool_level(corr.float().to(DEV), inverse.to(DEV), idx_ptr.to(DEV))
    got = run_pool(corr.float(), order, idx_ptr)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n_out, v, 2)
    check("pooled", got, want, fp32)
    assert torch.equal(got.cpu() == -1, want == -1)
    assert (got[0] == -1).all()
    if n_out > 1:      # count 0 (no child has both entries), so (-1, -1) although the sum of the first entries is 7
        assert (got[n_out - 1] == -1).all()
    assert torch.equal(run_pool(corr.float(), order, idx_ptr), got)
    assert torch.equal(run_pool(corr.long(), order, idx_ptr), got)          # an integer level-0 tensor is converted


def test_pool_corr_counts_both_sums_elementwise():
    """three children (4, -1), (2, 6), (-1, -1): count 1, sums (6, 6) -> (6, 6), not (3, 6)"""
    corr = torch.tensor([[[4.0, -1.0]], [[2.0, 6.0]], [[-1.0, -1.0]]])
    got = run_pool(corr, torch.arange(3), torch.tensor([0, 3]))
    assert got.cpu().tolist() == [[[6.0, 6.0]]]
    assert R.pool_level(corr.double(), torch.zeros(3, dtype=torch.long), torch.tensor([0, 3])).tolist() == [[[6.0, 6.0]]]


@pytest.mark.parametrize("exact", [False, True])
def test_pool_corr_two_levels(exact):
    """two chained levels as floats; with cluster sizes in {1, 2, 4} every mean of integers is exact in fp32 and the
    truncated patch coordinates are compared exactly"""
    g = torch.Generator().manual_seed(5 + exact)
    n2, v = 150, 3
    draw = (lambda n: torch.tensor([1, 2, 4])[torch.randint(0, 3, (n,), generator=g)]) if exact else \
        (lambda n: torch.randint(1, 9, (n,), generator=g))
    inv2, ord2, ptr2 = pooling(n2, draw(n2), g)
    n1 = inv2.shape[0]
    inv1, ord1, ptr1 = pooling(n1, draw(n1), g)
    corr = torch.randint(0, 37, (inv1.shape[0], v, 2), generator=g).double()
    if exact:      # whole level-2 clusters invisible, so that every count is a cluster size and every quotient a dyadic one
        corr[(torch.rand(n2, v, generator=g) < 0.33)[inv2[inv1]]] = -1
    else:
        corr[torch.rand(inv1.shape[0], v, generator=g) < 0.33] = -1
    want = R.pool_corr(corr, [(inv1, ptr1), (inv2, ptr2)])
    fp32 = R.pool_corr(corr.float().to(DEV), [(inv1.to(DEV), ptr1.to(DEV)), (inv2.to(DEV), ptr2.to(DEV))])
    mid = run_pool(corr.float(), ord1, ptr1)
    got = run_pool(mid, ord2, ptr2)
    check("two levels", got, want, fp32)
    assert torch.equal(got.cpu() == -1, want == -1)
    if exact:
        assert torch.equal(got.cpu().double(), want) and torch.equal(got.cpu().long(), want.long())


def test_pool_corr_without_views():
    from ptv3_hip import ops
    got = ops.concerto_pool_corr(torch.empty(10, 0, 2, device=DEV), torch.arange(10, device=DEV),
                                 torch.tensor([0, 4, 10], dtype=torch.int32, device=DEV))
    assert tuple(got.shape) == (2, 0, 2)


# ---- patch plan -------------------------------------------------------------------------------------------------------
PH, PW = 5, 7


@functools.lru_cache(maxsize=None)
def plan_inputs():
    """three scenes with 2, 0 and 3 images, V = 3; rows are two of every three feature rows; the first rows of scene 0 have
    0, 1 and V pairs; coordinates have fractions (pooled means), pairs are (-1, -1) or fully set"""
    g = torch.Generator().manual_seed(11)
    n, v = 900, 3
    img_num = torch.tensor([2, 0, 3])
    rows = torch.arange(n)[torch.arange(n) % 3 != 1]
    scene = torch.bucketize(rows, torch.tensor([300, 600, 900]), right=True)
    corr = torch.stack([torch.rand(n, v, generator=g) * PH, torch.rand(n, v, generator=g) * PW], dim=-1).double()
    corr[torch.rand(n, v, generator=g) < 0.4] = -1
    full = torch.bucketize(torch.arange(n), torch.tensor([300, 600, 900]), right=True)
    corr[full == 1] = -1                                        # a scene without an image has no correspondence
    corr[full == 0, 2] = -1                                     # scene 0 has two images only
    corr[0], corr[2, 1:], corr[2, 0] = -1, -1, torch.tensor([1.5, 2.25]).double()
    corr[3, :2] = torch.tensor([[4.0, 6.0], [0.0, 0.0]]).double()
    corr[701] = torch.tensor([[4.99, 6.99], [0.5, 0.5], [2.0, 3.0]]).double()
    return corr.float().double(), rows, scene, img_num


def test_plan_matches_unique():
    from ptv3_hip import ops
    corr, rows, scene, img_num = plan_inputs()
    n_patches = int(img_num.sum()) * PH * PW
    r, v, index = R.feature_index(corr, rows, scene, img_num, PH, PW)
    want_ids, want_slot, want_count = torch.unique(index, return_inverse=True, return_counts=True)
    img_base = (torch.cumsum(img_num, 0) - img_num).to(DEV)
    plan = ops.concerto_plan(corr.float().to(DEV), rows.to(DEV), scene.to(DEV), img_base, PH, PW, n_patches, check=True)
    assert plan.u == want_ids.shape[0] and torch.equal(plan.patch_ids.cpu(), want_ids)
    seg = plan.seg_start[:plan.u + 1].cpu().long()
    assert torch.equal(seg[1:] - seg[:-1], want_count) and int(seg[-1]) == index.shape[0]
    by_patch = torch.sort(index, stable=True)[1]                 # by patch, then by (row, view)
    assert torch.equal(plan.pair_row[:index.shape[0]].cpu(), rows[r][by_patch])
    slot = plan.slot[:rows.shape[0] * 3].cpu().view(-1, 3)
    assert torch.equal(slot[r, v], want_slot) and (slot[(corr[rows] == -1).all(-1)] >= plan.u).all()
    pairs_of = lambda row: int(((corr[row] != -1).any(-1)).sum())  # noqa: E731
    assert [pairs_of(0), pairs_of(2), pairs_of(701)] == [0, 1, 3]
    assert not (scene[r] == 1).any() and index.max() < n_patches
    again = ops.concerto_plan(corr.float().to(DEV), rows.to(DEV), scene.to(DEV), img_base, PH, PW, n_patches)
    assert torch.equal(again.patch_ids, plan.patch_ids) and torch.equal(again.pair_row, plan.pair_row)
    # a correspondence outside the images is a violated precondition: kept in one bucket, refused under check=True
    bad = corr.clone().float()
    bad[701, 2] = torch.tensor([float(PH), 0.0])                 # the row below the last patch row of the last image
    loose = ops.concerto_plan(bad.to(DEV), rows.to(DEV), scene.to(DEV), img_base, PH, PW, n_patches)
    assert int(loose.patch_ids[-1]) == n_patches
    with pytest.raises(RuntimeError, match="outside"):
        ops.concerto_plan(bad.to(DEV), rows.to(DEV), scene.to(DEV), img_base, PH, PW, n_patches, check=True)


def test_plan_without_a_pair():
    from ptv3_hip import ops
    corr, rows, scene, img_num = plan_inputs()
    img_base = (torch.cumsum(img_num, 0) - img_num).to(DEV)
    plan = ops.concerto_plan(-torch.ones(900, 3, 2, device=DEV), rows.to(DEV), scene.to(DEV), img_base, PH, PW, 175)
    assert plan.u == 0 and plan.patch_ids.numel() == 0
    with pytest.raises(RuntimeError, match="no occupied patch"):
        ops.concerto_patch_mean(torch.zeros(900, 8, device=DEV), plan)


# ---- patch mean -------------------------------------------------------------------------------------------------------
GRID = 30                                                        # 30 x 30 patches per image, two images


@functools.lru_cache(maxsize=None)
def mean_case(u):
    """rows (two of every three of n feature rows), one scene with two images, and correspondences that occupy exactly
    u patches; patch 0 of image 0 receives 300 pairs (more than a workgroup's threads), u >= 2 uses both images"""
    g = torch.Generator().manual_seed(31 + u)
    n = max(3 * u, 600)
    rows = torch.arange(n)[torch.arange(n) % 3 != 2]
    nr = rows.shape[0]
    chosen = torch.cat([torch.tensor([3]), 4 + torch.randperm(2 * GRID * GRID - 4, generator=g)[:u - 1]]).sort()[0]
    corr = -torch.ones(n, 2, 2, dtype=torch.float64)
    per_image = [chosen[chosen < GRID * GRID], chosen[chosen >= GRID * GRID] - GRID * GRID]
    for image, ids in enumerate(per_image):
        if ids.numel() == 0:
            continue
        pick = ids[torch.randint(0, ids.shape[0], (nr,), generator=g)]
        pick[:ids.shape[0]] = ids                                # every chosen patch at least once
        if image == 0:
            pick[-300:] = ids[0]
        keep = torch.rand(nr, generator=g) < 0.7
        keep[:ids.shape[0]] = True
        keep[-300:] = True
        cell = torch.stack([pick // GRID, pick % GRID], dim=1).double() + 0.25
        sel = rows[keep]
        corr[sel, image] = cell[keep]
    return n, rows, torch.zeros(nr, dtype=torch.long), corr


@functools.lru_cache(maxsize=None)
def mean_refs(c, u, dtype):
    n, rows, scene, corr = mean_case(u)
    g = torch.Generator().manual_seed(1000 * c + u)
    feat = torch.randn(n, c, generator=g, dtype=torch.float64).to(dtype).double()
    r, _, index = R.feature_index(corr, rows, scene, torch.tensor([2]), GRID, GRID)
    ids = torch.unique(index)
    assert ids.shape[0] == u
    dmean = torch.randn(u, c, generator=g, dtype=torch.float64).float().double()
    out = []
    for dt, dev in ((torch.float64, "cpu"), (torch.float32, DEV)):
        f = feat.to(dev, dt).clone().requires_grad_(True)
        mean = R.patch_mean_dense(f[rows.to(dev)][r.to(dev)], index.to(dev), 2 * GRID * GRID)[ids.to(dev)]
        mean.backward(dmean.to(dev, dt))
        out.append(dict(mean=mean.detach(), dfeat=f.grad))
    return feat, dmean, ids, out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("u", [1, 63, 65, 500])
@pytest.mark.parametrize("c", [3, 64, 80, 1664])
def test_patch_mean_forward_backward(c, u, dtype):
    from ptv3_hip import ops, autograd as A
    n, rows, scene, corr = mean_case(u)
    feat, dmean, ids, (r64, r32) = mean_refs(c, u, dtype)
    plan = ops.concerto_plan(corr.float().to(DEV), rows.to(DEV), scene.to(DEV), torch.zeros(1, dtype=torch.long, device=DEV),
                             GRID, GRID, 2 * GRID * GRID, check=True)
    assert plan.u == u and torch.equal(plan.patch_ids.cpu(), ids)
    seg = plan.seg_start[:u + 1].cpu()
    assert int((seg[1:] - seg[:-1]).max()) >= 300
    f = feat.to(DEV, dtype).requires_grad_(True)
    mean = A.concerto_patch_mean(f, plan)
    assert mean.dtype == torch.float32 and tuple(mean.shape) == (u, c)
    check("mean", mean, r64["mean"], r32["mean"])
    mean.backward(dmean.float().to(DEV))
    assert f.grad.dtype == dtype and tuple(f.grad.shape) == (n, c)
    check("dfeat", f.grad, r64["dfeat"], r32["dfeat"].to(dtype))
    paired = torch.zeros(n, dtype=torch.bool)
    paired[rows[(corr[rows] != -1).any(-1).any(-1)]] = True
    assert (~paired).sum() >= n // 3 and not f.grad[~paired.to(DEV)].any()          # exact zeros, every row written
    assert torch.equal(ops.concerto_patch_mean(f.detach(), plan), mean)
    assert torch.equal(ops.concerto_patch_mean_bwd(dmean.float().to(DEV), plan, dtype), f.grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("c,lead,vec", [(3, "row", False), (80, "row", True), (80, "two", False)],
                         ids=["c3-rows", "c80-rows", "c80-off-boundary"])
def test_patch_mean_of_a_slice_of_a_larger_matrix(c, lead, vec, dtype):
    """feat as a view into a larger matrix, its data pointer offset: rows 1 .. n of an (n + 2, C) matrix (C = 3 is
    then on no 16-byte boundary, C = 80 is), and a view that starts two elements into its storage, where C = 80 must
    fall back from 4 columns a load to one.  Same results as the whole tensor gives."""
    from ptv3_hip import ops, autograd as A
    u = 65
    n, rows, scene, corr = mean_case(u)
    feat, dmean, ids, (r64, r32) = mean_refs(c, u, dtype)
    plan = ops.concerto_plan(corr.float().to(DEV), rows.to(DEV), scene.to(DEV), torch.zeros(1, dtype=torch.long, device=DEV),
                             GRID, GRID, 2 * GRID * GRID, check=True)
    if lead == "row":
        big = torch.full((n + 2, c), 1e4, dtype=dtype, device=DEV)
        view = big[1:n + 1]
    else:
        big = torch.full((n * c + 4,), 1e4, dtype=dtype, device=DEV)
        view = big[2:2 + n * c].view(n, c)
    view.copy_(feat.to(DEV, dtype))
    assert view.is_contiguous() and view.data_ptr() != big.data_ptr()
    assert (view.data_ptr() % 16 == 0 and c % 4 == 0) == vec
    f = view.detach().requires_grad_(True)
    mean = A.concerto_patch_mean(f, plan)
    check("mean", mean, r64["mean"], r32["mean"])
    mean.backward(dmean.float().to(DEV))
    check("dfeat", f.grad, r64["dfeat"], r32["dfeat"].to(dtype))
    whole = ops.concerto_patch_mean(feat.to(DEV, dtype), plan)
    assert torch.equal(mean, whole)          # whichever load width: the same additions in the same order
    assert (big.flatten()[:1] == 1e4).all() and (big.flatten()[-1:] == 1e4).all()


# ---- centred cosine loss ----------------------------------------------------------------------------------------------
COS_CASES = [(u, d) for u in (1, 63, 65, 700) for d in (2, 64, 100, 384, 1536)] + [(2500, 100)]


def eps_row(u):
    """the row of `a` that is constant (zero without the shift), so that its centred norm is 0; u = 1 has none, its one
    row is an ordinary one"""
    return u // 2 if u > 1 else None


def check_da(name, da, r64, r32, u):
    """the gradient under the rule on the ordinary rows by themselves - the eps row's entries, b' / (1e-6 |b'|), are 1e5 to
    1e7 times larger and would set both terms of the bound for every other row - and on the eps row by itself"""
    e = eps_row(u)
    rest = torch.ones(u, dtype=torch.bool)
    if e is not None:
        rest[e] = False
        check(name + " eps row", da[e], r64[e], r32[e])
    assert r64[rest].abs().max() > 0
    check(name + " ordinary rows", da.cpu()[rest], r64[rest], r32.cpu()[rest])


@functools.lru_cache(maxsize=None)
def cos_refs(u, d, shift, dtype):
    g = torch.Generator().manual_seed(17 * u + d)
    nb = 2 * u + 5
    a = (torch.randn(u, d, generator=g, dtype=torch.float64) * 0.3 + 0.2).to(dtype).double()
    b = (torch.randn(nb, d, generator=g, dtype=torch.float64) + 0.5).to(dtype).double()

    def apart(t):
        """no accidental eps row: at D = 2 two bf16 entries of a row can coincide, which centres it to nothing"""
        c = t - t.mean(1, keepdim=True) if shift else t
        t[c.norm(dim=1) < 1e-5, 0] += 0.5
        return t.to(dtype).double()

    a, b = apart(a), apart(b)
    if eps_row(u) is not None:
        a[eps_row(u)] = 0.375 if shift else 0.0                  # centred norm 0: the eps branch
    ids = torch.randperm(nb, generator=g)[:u].sort()[0]
    out = []
    for dt, dev in ((torch.float64, "cpu"), (torch.float32, DEV)):
        av = a.to(dev, dt).clone().requires_grad_(True)
        rows = b.to(dev, dt)[ids.to(dev)]
        cos = R.cosines(av, rows, shift)
        loss = (1 - cos).mean() * 10
        (loss * 0.75).backward()
        out.append(dict(cos=cos.detach(), loss=loss.detach().reshape(1), da=av.grad))
    return a, b, ids, out


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shift", [True, False], ids=["shift", "plain"])
@pytest.mark.parametrize("u,d", COS_CASES)
def test_cos_loss_forward_backward(u, d, shift, dtype):
    from ptv3_hip import ops
    assert ops.concerto_cos_capable(d)
    a, b, ids, (r64, r32) = cos_refs(u, d, shift, dtype)
    assert u == 1 or (ids[1:] - ids[:-1]).max() > 1              # patch ids with gaps
    ad, bd, idd = a.to(DEV, dtype), b.to(DEV, dtype), ids.to(DEV)
    loss, cos, stats = ops.concerto_cos(ad, bd, idd, shift)
    check("cos", cos, r64["cos"], r32["cos"])
    check("loss", loss, r64["loss"], r32["loss"])
    e = eps_row(u)
    if e is not None:
        assert abs(r64["cos"][e].item()) < 1e-6 and abs(cos[e].item()) < 1e-6 and stats[e, 2].item() < 1e-6
    rest = stats.cpu()[torch.arange(u) != (-1 if e is None else e)]
    assert (rest[:, 2:] > 1e-6).all()                            # every other row off the eps branch
    da = ops.concerto_cos_bwd(torch.tensor([0.75], device=DEV), ad, bd, idd, shift)
    assert da.dtype == dtype and da.shape == ad.shape
    check_da("da", da, r64["da"], r32["da"].to(dtype), u)
    again = ops.concerto_cos(ad, bd, idd, shift)
    assert all(torch.equal(p, q) for p, q in zip(again, (loss, cos, stats)))
    assert torch.equal(ops.concerto_cos_bwd(torch.tensor([0.75], device=DEV), ad, bd, idd, shift), da)


def test_cos_autograd_mixed_dtypes_and_refusals():
    from ptv3_hip import ops, autograd as A
    u, d = 65, 100
    a, b, ids, (r64, r32) = cos_refs(u, d, True, torch.float32)
    av = a.float().to(DEV).requires_grad_(True)
    loss = A.concerto_cos_loss(av, b.float().to(DEV), ids.to(DEV), True)
    (loss * 0.75).backward()
    check("loss", loss.reshape(1), r64["loss"], r32["loss"])
    check_da("da", av.grad, r64["da"], r32["da"], u)
    # a bf16 encoder against fp32 projected rows: the rounded rows, upcast, give the same loss bit for bit
    bb = b.to(DEV, torch.bfloat16)
    one = ops.concerto_cos(av.detach(), bb, ids.to(DEV))
    two = ops.concerto_cos(av.detach(), bb.float(), ids.to(DEV))
    assert all(torch.equal(p, q) for p, q in zip(one, two))
    assert not ops.concerto_cos_capable(0) and not ops.concerto_cos_capable(2049) and ops.concerto_cos_capable(2048)
    with pytest.raises(RuntimeError, match="unsupported"):
        ops.concerto_cos(torch.zeros(4, 2100, device=DEV), torch.zeros(9, 2100, device=DEV), torch.arange(4, device=DEV))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.concerto_cos(a.float(), b.float().to(DEV), ids.to(DEV))
    with pytest.raises(RuntimeError, match="expected"):
        ops.concerto_cos(av.detach(), b.float().to(DEV)[:, :50].contiguous(), ids.to(DEV))


# ---- the model against the reference's fixture ----------------------------------------------------------------------
from make_golden_sonata import SEED, MOMENTUM  # noqa: E402
from make_golden_concerto import load_golden, concerto_state_dict, with_stub_encoder, TINY_KW, LOSSES  # noqa: E402

_G = {}


def golden(golden_dir):
    if not _G:
        _G.update(load_golden(golden_dir))
    return _G


def _close(name, got, want, gap, extra=0.0):
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    floor = ULP * np.abs(want).max()             # one fp32 rounding at the tensor's scale: a stored gap can be less
    print(f"{name}: err {err.max():.3e} gap {gap:.3e} floor {floor:.3e}")
    assert (err <= np.maximum(4 * gap, floor) + extra).all(), (name, err.max(), gap)


def _grad_bound(g, name):
    stored = g["grad_" + name].astype(np.float64) * float(g["gmax_" + name])
    return stored, 2.0 ** -11 * np.abs(stored) + 2.0 ** -24 * float(g["gmax_" + name])


def _model(g, fused, monkeypatch=None):
    """the tiny model on the device, replaying the fixture's patch permutation; fused: the image branch and every loss
    through the kernels, whatever `wired` lists (the wiring is a measurement, not a capability)"""
    import copy
    from pointcept.models.concerto import Concerto, concerto_v1m1_base as M
    from pointcept.models.sonata import sonata_v1m1_base as S
    model = with_stub_encoder(Concerto)(**copy.deepcopy(TINY_KW))
    concerto_state_dict(model)
    model = model.to(DEV).set_fused(fused).train()
    real, perm = model.generate_mask, torch.from_numpy(g["patch_index"]).to(DEV)
    model.generate_mask = lambda coord, offset: real(coord, offset, patch_index=perm)
    if monkeypatch is not None:
        monkeypatch.setattr(M, "wired", lambda kernel, width, rows: True)
        monkeypatch.setattr(S, "wired", lambda kernel, k, m: True)
    return model


def _data(g):
    return {k[3:]: torch.from_numpy(g[k]).to(DEV) for k in g if k.startswith("in_")}


_STEP = {}


def _train_step(g, fused, monkeypatch):
    if fused not in _STEP:
        from ptv3_hip import autograd as A, ops
        calls = []

        def counted(owner, name):
            real = getattr(owner, name)
            monkeypatch.setattr(owner, name, lambda *a, **k: (calls.append(name), real(*a, **k))[1])

        counted(A, "concerto_patch_mean"), counted(A, "concerto_cos_loss"), counted(ops, "concerto_pool_corr")
        model = _model(g, fused, monkeypatch)
        torch.manual_seed(SEED)
        out = model(_data(g))
        out["loss"].backward()
        torch.cuda.synchronize()
        assert sorted(calls) == (["concerto_cos_loss", "concerto_patch_mean", "concerto_pool_corr"] if fused else [])
        _STEP[fused] = ({k: out[k].item() for k in out},
                        {k: (None if p.grad is None else p.grad.detach().cpu().numpy()) for k, p in model.named_parameters()},
                        model)
    return _STEP[fused]


@pytest.mark.parametrize("fused", [True, False])
def test_model_training_step_matches_reference(golden_dir, fused, monkeypatch):
    g = golden(golden_dir)
    losses, grads, model = _train_step(g, fused, monkeypatch)
    assert sorted(losses) == sorted(LOSSES)
    for k in LOSSES:
        _close(k, losses[k], g[k], float(g["gap_" + k]))
    nograd = set(g["nograd"].tolist())
    assert {k for k, v in grads.items() if v is None} == nograd
    assert all(not p.requires_grad for p in model.teacher.parameters())
    assert len(grads) - len(nograd) == sum(1 for k in g if k.startswith("gmax_"))
    for name, got in grads.items():
        if got is not None:
            stored, step = _grad_bound(g, name)
            _close("grad " + name, got, stored, float(g["gap_grad_" + name]), step)


def test_model_fused_and_composed_agree(golden_dir, monkeypatch):
    g = golden(golden_dir)
    (l1, g1, _), (l0, g0, _) = _train_step(g, True, monkeypatch), _train_step(g, False, monkeypatch)
    for k in LOSSES:
        _close(k, l1[k], l0[k], float(g["gap_" + k]))
    for name in g1:
        if g1[name] is not None:
            _close("grad " + name, g1[name], g0[name], float(g["gap_grad_" + name]))


def test_model_image_branch_intermediates(golden_dir, monkeypatch):
    """pooled correspondences and patch ids exactly, patch means and projected rows within the fixture's gaps, through
    the kernels on the fixture's stored up-cast features"""
    from ptv3_hip import ops
    g = golden(golden_dir)
    model = _model(g, True, monkeypatch)
    order = torch.sort(torch.from_numpy(g["pool_inverse"]), stable=True)[1].to(DEV)
    pooled = ops.concerto_pool_corr(torch.from_numpy(g["in_global_correspondence"]).to(DEV), order,
                                    torch.from_numpy(g["pool_idx_ptr"]).int().to(DEV))
    assert np.array_equal(pooled.cpu().numpy(), g["pooled_corr"])
    rows, scene = model.principal_rows(torch.from_numpy(g["offset_enc2d"]).to(DEV))
    with torch.no_grad():
        f2d = model.ENC2D_forward(torch.from_numpy(g["in_images"]).to(DEV))
    f2d = f2d.reshape(-1, f2d.shape[-1]).contiguous()
    loss, mid = model.enc2d_loss(torch.from_numpy(g["enc2d_feat"]).to(DEV), pooled, rows, scene, f2d,
                                 torch.from_numpy(g["in_img_num"]).to(DEV), check=True)
    assert np.array_equal(mid["patch_ids"].cpu().numpy(), g["patch_ids"])
    _close("patch_mean", mid["patch_mean"].detach().cpu().numpy(), g["patch_mean"], float(g["gap_patch_mean"]))
    _close("projected", mid["projected"].detach().cpu().numpy(), g["projected"], float(g["gap_projected"]))
    _close("enc2d_loss", loss.item(), g["enc2d_loss"], float(g["gap_enc2d_loss"]))


def test_model_after_step_and_return_point(golden_dir, monkeypatch):
    g = golden(golden_dir)
    _, _, model = _train_step(g, True, monkeypatch)
    model.momentum = MOMENTUM
    model.after_step()
    torch.cuda.synchronize()
    for k, p in model.teacher.named_parameters():
        _close("ema " + k, p.detach().cpu().numpy(), g["ema_teacher." + k], float(g["gap_ema_teacher." + k]))
    for k, p in model.enc2d_head_teacher.named_parameters():
        _close("2d " + k, p.detach().cpu().numpy(), g["ema_enc2d_head_teacher." + k],
               float(g["gap_ema_enc2d_head_teacher." + k]))
    data = _data(g)
    with torch.no_grad():
        torch.manual_seed(SEED)
        out = model.eval()(dict(feat=data["global_feat"], coord=data["global_coord"], offset=data["global_offset"],
                                grid_size=data["grid_size"][0]), return_point=True)
    point = out["point"]
    # the teacher's point up-cast by up_cast_level = 1: level 2 of the hierarchy, 32 + 32 channels
    assert tuple(point.feat.shape) == (g["teacher_mask_head_in"].shape[0], 64) and torch.isfinite(point.feat).all()
    assert torch.equal(point.offset.cpu(), torch.from_numpy(g["offset_teacher"]))
