"""The evaluator kernels on the GPU (csrc/evaluator.hip) against the numpy restatements of
tests/insseg_ref.py, and the three hooks through those kernels against tests/golden/seg_evaluators.npz.  Everything the
kernels produce is an integer count: every comparison is equality."""
import numpy as np
import pytest
import torch

import insseg_ref as R
import test_seg_evaluators_cpu as C

pytestmark = pytest.mark.gpu

fixture = C.fixture


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture()
def kernels_everywhere(monkeypatch):
    """The hooks call a kernel only at the shapes where it measured ahead; here every shape takes it."""
    import pointcept.utils.misc as M
    import pointcept.engines.hooks.evaluator as E
    monkeypatch.setattr(M, "SEG_CONFUSION_MIN_ELEMENTS", 0)
    monkeypatch.setattr(E, "INSSEG_MIN_PROPOSALS", 0)
    monkeypatch.setattr(E, "INSSEG_MIN_POINTS", 0)


# ------------------------------------------------------------------------------------------------
# 1. seg_confusion
# ------------------------------------------------------------------------------------------------
def _seg_case(n, k, seed, m=None, ignore=-1):
    """logits in quarters from a narrow range (exact in bf16 and fp16, most rows tie), targets from [-1, k + 2] and the
    ignore index, so that values below 0 and at or above K occur"""
    g = np.random.default_rng(seed)
    logits = (g.integers(-6, 7, size=(n, k)) / 4.0).astype(np.float32)
    m = n if m is None else m
    target = g.integers(-1, k + 3, size=m)
    target[g.random(m) < 0.15] = ignore
    inverse = None if m == n else g.integers(0, n, size=m)
    return logits, target.astype(np.int64), inverse


def _expect(logits, target, inverse, k, ignore):
    pred = R.argmax_first(logits)
    return R.confusion(pred if inverse is None else pred[inverse], target, k, ignore)


@pytest.mark.parametrize("k", [1, 2, 13, 200])
def test_seg_confusion_sizes_dtypes_and_both_forms(dev, k):
    from ptv3_hip import ops
    for n in (1, 63, 64, 65, 5003):
        logits, target, _ = _seg_case(n, k, 100 * k + n)
        want = _expect(logits, target, None, k, -1)
        if k > 1 and n >= 63:
            top = np.sort(logits, axis=1)
            assert (top[:, -1] == top[:, -2]).any()   # rows with more than one maximum
        t64 = torch.from_numpy(target).to(dev)
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            got = ops.seg_confusion(torch.from_numpy(logits).to(dev).to(dtype), t64, k, -1)
            assert got.dtype == torch.int64 and tuple(got.shape) == (3, k)
            assert np.array_equal(got.cpu().numpy(), want), (n, k, dtype)
        pred = torch.from_numpy(R.argmax_first(logits)).to(dev)
        for pt, tt in ((torch.int64, torch.int64), (torch.int32, torch.int64), (torch.int64, torch.int32),
                       (torch.int32, torch.int32)):
            got = ops.seg_confusion(pred.to(pt), t64.to(tt), k, -1)
            assert np.array_equal(got.cpu().numpy(), want), (n, k, pt, tt)
        got = ops.seg_confusion(torch.from_numpy(logits).to(dev), t64.int(), k, -1)
        assert np.array_equal(got.cpu().numpy(), want)


def test_seg_confusion_at_the_cap_and_above_it(dev):
    """K at PTV3_SEG_CONFUSION_MAX_K takes the kernel, one more the torch composition; both count the same."""
    from ptv3_hip import ops
    for k in (ops.SEG_CONFUSION_MAX_K, ops.SEG_CONFUSION_MAX_K + 1):
        logits, target, inverse = _seg_case(5003, k, k, m=7001)
        want = _expect(logits, target, inverse, k, -1)
        got = ops.seg_confusion(torch.from_numpy(logits).to(dev), torch.from_numpy(target).to(dev), k, -1,
                                inverse=torch.from_numpy(inverse).to(dev))
        assert np.array_equal(got.cpu().numpy(), want), k
        pred = torch.from_numpy(R.argmax_first(logits)[inverse]).to(dev)
        got = ops.seg_confusion(pred, torch.from_numpy(target).to(dev), k, -1)
        assert np.array_equal(got.cpu().numpy(), want), k


@pytest.mark.parametrize("ignore", [-1, 255, 5])
def test_seg_confusion_inverse_ignore_accumulate_and_repeat(dev, ignore):
    """inverse of 7 001 over 5 003 rows in both forms; the ignore index outside and inside [0, K); two calls add into one
    table; two identical runs are bitwise equal; every target ignored counts nothing."""
    from ptv3_hip import ops
    k = 13
    logits, target, inverse = _seg_case(5003, k, 7 + ignore, m=7001, ignore=ignore)
    assert (target == ignore).any() and ((target >= k) & (target != ignore)).any()
    want = _expect(logits, target, inverse, k, ignore)
    lo, tg, inv = (torch.from_numpy(a).to(dev) for a in (logits, target, inverse))
    got = ops.seg_confusion(lo, tg, k, ignore, inverse=inv)
    assert np.array_equal(got.cpu().numpy(), want)
    for dtype in (torch.bfloat16, torch.float16):
        assert torch.equal(ops.seg_confusion(lo.to(dtype), tg, k, ignore, inverse=inv), got)
    pred = torch.from_numpy(R.argmax_first(logits)).to(dev)
    assert torch.equal(ops.seg_confusion(pred, tg, k, ignore, inverse=inv), got)
    assert torch.equal(ops.seg_confusion(pred.int(), tg.int(), k, ignore, inverse=inv), got)
    # accumulation: a second batch into the same table
    logits2, target2, _ = _seg_case(4097, k, 99, ignore=ignore)
    back = ops.seg_confusion(torch.from_numpy(logits2).to(dev), torch.from_numpy(target2).to(dev), k, ignore, counts=got)
    assert back is got
    assert np.array_equal(got.cpu().numpy(), want + _expect(logits2, target2, None, k, ignore))
    again = ops.seg_confusion(lo, tg, k, ignore, inverse=inv)
    ops.seg_confusion(torch.from_numpy(logits2).to(dev), torch.from_numpy(target2).to(dev), k, ignore, counts=again)
    assert torch.equal(again, got)
    # every target ignored
    all_ignored = torch.full_like(tg, ignore)
    got = ops.seg_confusion(lo, all_ignored, k, ignore, inverse=inv).cpu().numpy()
    assert np.array_equal(got, R.confusion(R.argmax_first(logits)[inverse], np.full(7001, ignore), k, ignore))
    if not 0 <= ignore < k:
        assert not got.any()
    # the composition, which the wrapper takes above the cap, on the same inputs
    assert np.array_equal(ops.seg_confusion_torch(lo, tg, k, ignore, inverse=inv).cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------
# 2. insseg_associate
# ------------------------------------------------------------------------------------------------
def _ins_case(p, nm, g, seed, n=None, density=0.04):
    """masks with a few percent of entries set, among them values 2 and -1; row 0 all zero, row 1 all set and row 2 of
    2 and -1 only, where there are that many rows; codes over [0, g] with a fifth of the points void"""
    r = np.random.default_rng(seed)
    masks = (r.random((p, nm)) < density).astype(np.int64)
    masks[r.random((p, nm)) < density / 4] = 2
    masks[r.random((p, nm)) < density / 4] = -1
    if p > 0:
        masks[0] = 0
    if p > 1:
        masks[1] = 1
    if p > 2:
        masks[2] = np.where(np.arange(nm) % 2 == 0, 2, -1)
    n_eval = nm if n is None else n
    idx = None if n is None else r.integers(0, nm, size=n)
    code = r.integers(0, g + 1, size=n_eval).astype(np.int64)
    if g > 0 and n_eval > g:
        code[: g + 1] = np.arange(g + 1)      # every column is hit
    code = np.where(r.random(n_eval) < 0.2, code + R.VOID, code).astype(np.int32)
    return masks, code, idx


MASK_DTYPES = (torch.int32, torch.uint8, torch.bool, torch.int64)


def _check_associate(dev, masks, code, g, idx=None, dtypes=MASK_DTYPES, idx_dtypes=(torch.int64,)):
    from ptv3_hip import ops
    want = R.associate(masks, code, g, idx)
    tc = torch.from_numpy(code).to(dev)
    first = None
    for dtype in dtypes:
        tm = torch.from_numpy(masks).to(dev)
        tm = tm.ne(0) if dtype == torch.bool else tm.to(dtype)   # -1 becomes 255 in uint8: still set
        for it in (idx_dtypes if idx is not None else (None,)):
            ti = None if idx is None else torch.from_numpy(idx).to(dev).to(it)
            got = ops.insseg_associate(tm, tc, g, ti)
            assert all(t.dtype == torch.int32 for t in got)
            assert tuple(got[0].shape) == (masks.shape[0], g + 1)
            for a, b, name in zip(got, want, ("inter", "vert_count", "void_inter")):
                assert np.array_equal(a.cpu().numpy(), b), (name, dtype, it)
            if first is None:
                first = got
                again = ops.insseg_associate(tm, tc, g, ti)
                assert all(torch.equal(a, b) for a, b in zip(first, again))
    return first


@pytest.mark.parametrize("p,n,g", [(1, 1, 1), (3, 257, 5), (37, 4099, 300)])
def test_insseg_associate_shapes_and_mask_dtypes(dev, p, n, g):
    masks, code, _ = _ins_case(p, n, g, 1000 + n)
    _check_associate(dev, masks, code, g)


def test_insseg_associate_at_the_cap_and_above_it(dev):
    from ptv3_hip import ops
    for g in (ops.INSSEG_MAX_GT, ops.INSSEG_MAX_GT + 1):
        masks, code, _ = _ins_case(5, 6000, g, g)      # 6000: rows that take the 16-byte loads in every dtype
        _check_associate(dev, masks, code, g)


def test_insseg_associate_without_proposals_or_points(dev):
    from ptv3_hip import ops
    code = torch.zeros(50, dtype=torch.int32, device=dev)
    inter, vert, void = ops.insseg_associate(torch.zeros((0, 50), dtype=torch.int32, device=dev), code, 4)
    assert tuple(inter.shape) == (0, 5) and tuple(vert.shape) == (0,) and tuple(void.shape) == (0,)
    inter, vert, void = ops.insseg_associate(torch.zeros((3, 0), dtype=torch.int32, device=dev), code[:0], 4)
    assert tuple(inter.shape) == (3, 5) and not inter.any() and not vert.any() and not void.any()
    inter, vert, void = ops.insseg_associate(torch.ones((2, 50), dtype=torch.int32, device=dev), code, 0)
    assert inter.cpu().tolist() == [[50], [50]] and vert.cpu().tolist() == [50, 50] and void.cpu().tolist() == [0, 0]


def test_insseg_associate_through_idx(dev):
    """idx of 9 001 entries over masks of 4 099 points, int32 and int64: some columns are read by several evaluated
    points and some by none; the gathered copy is never made"""
    masks, code, idx = _ins_case(7, 4099, 40, 5, n=9001)
    _check_associate(dev, masks, code, 40, idx, idx_dtypes=(torch.int64, torch.int32))


def test_insseg_associate_rows_split_over_workgroups(dev):
    """Three full chunks and a ragged fourth per row, with and without the 16-byte loads and through idx: the counts
    equal the unsplit restatement."""
    from ptv3_hip import ops
    chunk = ops.insseg_chunk()
    for n in (3 * chunk + 80, 3 * chunk + 77):     # a multiple of 16 and an odd length
        masks, code, _ = _ins_case(4, n, 9, n, density=0.02)
        _check_associate(dev, masks, code, 9)
    masks, code, idx = _ins_case(4, 3 * chunk + 77, 9, 3, n=40001, density=0.02)
    _check_associate(dev, masks, code, 9, idx, dtypes=(torch.int32,))


# ------------------------------------------------------------------------------------------------
# 3. the hooks on the GPU
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", C.SEM_RUNS + ["cls0"])
def test_semseg_and_cls_hooks_through_the_kernel(dev, fixture, kernels_everywhere, monkeypatch, tag):
    from ptv3_hip import ops
    calls = []
    kernel = ops.seg_confusion
    monkeypatch.setattr(ops, "seg_confusion", lambda *a, **k: calls.append(1) or kernel(*a, **k))
    C.run_seg_hook(fixture, tag, device=dev)     # the same integers and metrics as the CPU test asks
    assert len(calls) == int(fixture[tag + "_nbatch"])


@pytest.mark.parametrize("masks_on", ["cpu", "device"])
def test_insseg_hook_with_host_and_device_masks(dev, fixture, kernels_everywhere, monkeypatch, masks_on):
    from ptv3_hip import ops
    calls = []
    kernel = ops.insseg_associate
    monkeypatch.setattr(ops, "insseg_associate", lambda *a, **k: calls.append(1) or kernel(*a, **k))
    C.run_ins_hook(fixture, device=dev, out_device="cpu" if masks_on == "cpu" else dev, monkeypatch=monkeypatch)
    assert len(calls) == (0 if masks_on == "cpu" else int(fixture["ins0_nbatch"]))


def test_insseg_hook_on_pointgroup_device_results(dev, golden_dir, kernels_everywhere):
    """A tiny PG-v1m1 through InsSegEvaluator: the hook switches the model to device results for the evaluation and back,
    and its tables equal those the restatement makes from the same model's CPU results."""
    import types
    import test_hip_pointgroup as PG
    from pointcept.engines.hooks.builder import HOOKS
    import pointcept.engines.hooks  # noqa: F401
    g, model, data = PG._golden(golden_dir, dev, "v1m1")
    model.eval()
    n = data["coord"].shape[0]
    data["offset"] = torch.tensor([n], device=dev)      # one scene per batch, as the hook asks
    with torch.no_grad():
        host = model(dict(data))
    assert not host["pred_masks"].is_cuda and host["pred_masks"].shape[0] > 0
    seen = []
    handle = model.register_forward_hook(lambda m, i, out: seen.append(out))
    logs = []
    hook = HOOKS.build(dict(type="InsSegEvaluator", segment_ignore_index=PG.IGNORE, instance_ignore_index=-1))
    hook.trainer = types.SimpleNamespace(
        val_loader=[dict(data, name=["tiny"])], model=model, logger=types.SimpleNamespace(info=logs.append), writer=None,
        epoch=0, comm_info={}, best_metric_value=0.0,
        cfg=types.SimpleNamespace(evaluate=True, enable_wandb=False, data=types.SimpleNamespace(
            num_classes=20, ignore_index=-1, names=[f"c{i}" for i in range(20)])))
    hook.before_train()
    hook.after_epoch()
    handle.remove()
    assert len(seen) == 1 and all(seen[0][k].is_cuda for k in ("pred_masks", "pred_classes", "pred_scores"))
    assert model._device_results is False
    assert torch.equal(seen[0]["pred_masks"].cpu(), host["pred_masks"])
    scene = hook.scenes["tiny"]
    want = R.scene_tables(host["pred_masks"].numpy(), data["segment"].cpu().numpy(), data["instance"].cpu().numpy(),
                          PG.IGNORE, -1)
    for key, value in want.items():
        assert np.array_equal(scene[key], value), key
    assert np.array_equal(scene["pred_classes"], host["pred_classes"].numpy())
    assert np.array_equal(scene["pred_scores"], host["pred_scores"].numpy().astype(np.float64))
    assert hook.trainer.comm_info["current_metric_name"] == "AP50" and logs[-1].startswith("<<<<")
