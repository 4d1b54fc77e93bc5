"""cRSE window attention at windows above 64 tokens, forward (both kernels) and backward, vs oracle/swin3d.py and
torch autograd (float64) over test_hip_swin3d's restatement.  PARITY UNPINNED, as every Swin3D test (see test_hip_swin3d).

swin_attn_kernel and swin_attn_bwd_kernel serve a query with G = max(16, head_dim, pow2ceil(m)) <= 64 lanes.  Above 64
tokens a lane walks several keys, the backward's third sweep runs several group-uniform steps (shuffle-fed scatter into
the table gradients, LDS atomics into dK / dV) and the per-wave logit rows grow from 64 to max_tokens entries.  The
fork's models (quant_size 50: 700- and 400-row tables, refused by the matrix-core kernel) run exactly these two kernels,
with 7^3 windows on the coarse levels.  The windows here have chosen token counts on both sides of every change of G
(16/17, 32/33, 64/65), of the number of key steps (64/65, 128/129), the full windows (125, 343) and one voxel."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_hip_swin3d as base  # noqa: E402  (helpers: _case, _run, _rel, _crse_attention_torch)
from oracle import swin3d as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


CONFIGS = [(2, 16, 50, "XYZ_RGB"),            # the fork's setting: long tables, gather kernel only
           (2, 8, 4, "XYZ_RGB_NORM"), (2, 32, 4, "XYZ")]
SIZES = {5: [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 125], 7: [1, 64, 65, 128, 129, 343]}
# (window size, shift).  Shift 3 is the model's own half-window shift: it cuts the aligned 7^3 cubes 4 | 3 per axis, so
# no piece exceeds 4^3 = 64 tokens.  Shift 1 cuts them 6 | 1: pieces up to 6^3 = 216 tokens, the shifted partition
# with several key steps per lane.
GEOMS = [(5, 0), (7, 0), (7, 3), (7, 1)]
SEED = 1
BF16_OUT = 2.0 ** -7          # one bf16 rounding of an output (test_layernorm_backward_with_residual_gradient's figure)


def _sized_windows(ws, sizes, seed):
    """Window w holds sizes[w] randomly chosen cells of the ws^3 cube at origin (2 w ws, 0, 0); voxels shuffled."""
    rng = np.random.default_rng(seed)
    cells = np.stack(np.meshgrid(np.arange(ws), np.arange(ws), np.arange(ws), indexing="ij"), -1).reshape(-1, 3)
    c = np.concatenate([cells[rng.permutation(ws ** 3)[:m]] + np.array([2 * w * ws, 0, 0])
                        for w, m in enumerate(sizes)])
    c = c[rng.permutation(len(c))]
    return np.concatenate([np.zeros((len(c), 1), np.int64), c], 1).astype(np.int32)


def _frozen(a):
    a.setflags(write=False)
    return a


def _bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a)).bfloat16().float().numpy()


@functools.lru_cache(maxsize=None)
def _sized_case(cfg, ws, shift, sizes=None):
    heads, hd, quant, crse = cfg
    sizes = SIZES[ws] if sizes is None else list(sizes)
    coords = _sized_windows(ws, sizes, SEED)
    case = base._case(coords, heads, hd, ws, quant, crse, seed=hd + ws + shift, shift=shift)
    w_sizes = case[5]
    if shift == 0:                           # the inputs hold the token counts they were built for
        assert list(w_sizes) == sorted(sizes), list(w_sizes)
    return case


def _row_reads(case):
    """How often each table row of each signal axis is read: floor(diff + rows // 2), clamped, as the restatement."""
    q, _, _, _, offs, w_sizes, w2n, _, cr = case
    per = q.shape[1] * q.shape[2]
    reads = [np.zeros(int(o) // per, np.int64) for o in offs]
    for w in range(len(w_sizes)):
        c = cr[int(w2n[w]):int(w2n[w]) + int(w_sizes[w])]
        for a, r in enumerate(reads):
            idx = np.floor((c[:, None, a] - c[None, :, a]) + np.float32(len(r) // 2)).astype(np.int64)
            r += np.bincount(idx.clip(0, len(r) - 1).reshape(-1), minlength=len(r))
    return reads


def _check_inputs(case, ws, shift, quant):
    """CPU-side: the case still sits on the edges it was built for.  -> mask of the table elements no pair reads."""
    q, _, _, _, offs, w_sizes, _, _, _ = case
    per = q.shape[1] * q.shape[2]
    reads = _row_reads(case)
    if shift == 0:
        assert {65, 125} <= set(w_sizes) if ws == 5 else {65, 129, 343} <= set(w_sizes)
        # clamped end rows: reached on every axis at quant 4; at quant 50 only the signal axes' (the +-2 differences
        # of _case's pinned signals), a window is too small for the position tables' ends
        for a, r in enumerate(reads):
            if quant == 4 or a >= 3:
                assert r[0] >= 1 and r[-1] >= 1, (a, r[0], r[-1])
    elif shift == 1:
        assert w_sizes.max() > 128, w_sizes.max()
    else:
        assert w_sizes.max() == 64                 # 4 | 3 cut of the full 7^3 window
    if shift:
        assert all((r == 0).sum() > 0 for r in reads[:3])             # position rows out of a cut window's reach
    return np.concatenate([np.repeat(r == 0, per) for r in reads])


def _per_window_worst(err, case):
    """max-abs error over the rows of each window -> (worst error, that window's token count)."""
    w_sizes, w2n, n2n = case[5], case[6], case[7]
    per_row = err.reshape(len(err), -1).max(1)[np.asarray(n2n, np.int64)]
    per_win = np.maximum.reduceat(per_row, np.asarray(w2n, np.int64))
    worst = int(per_win.argmax())
    return float(per_win[worst]), int(w_sizes[worst])


@functools.lru_cache(maxsize=None)
def _forward_want(cfg, ws, shift, bf16, sizes=None):
    case = _sized_case(cfg, ws, shift, sizes)
    qkv = [_bf16_round(a) for a in case[:3]] if bf16 else case[:3]
    return _frozen(O.crse_attention(*qkv, *case[3], *case[4:]))


def _check_forward(got, want, case, dtype, what):
    rel = base._rel(got, want)
    worst, tokens = _per_window_worst(np.abs(got - want), case)
    scale = max(1.0, float(np.abs(want).max()))
    print(f"{what}: rel L2 {rel:.3e}, worst window ({tokens} tokens) max-abs {worst:.3e}")
    if dtype == torch.float32:
        assert rel <= 1e-4, (what, rel)
        assert worst <= 1e-4 * scale, f"{what}: max-abs {worst:.3e} in a window of {tokens} tokens"
    else:
        assert rel <= 1e-2, (what, rel)
        assert worst <= BF16_OUT * scale, f"{what}: max-abs {worst:.3e} in a window of {tokens} tokens"


def _run_gather(dev, case, ws, dtype):
    os.environ["PTV3_SWIN_ATTN_MFMA"] = "0"
    try:
        return base._run(dev, case, ws, dtype)
    finally:
        os.environ.pop("PTV3_SWIN_ATTN_MFMA", None)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ws", [5, 7])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"h{c[0]}d{c[1]}q{c[2]}{c[3]}")
def test_crse_attention_forward_at_chosen_window_sizes(dev, cfg, ws, dtype):
    """Forward at windows of 1 .. 125 / 343 tokens against the oracle (bf16: on bf16-rounded q, k, v), whole tensor and
    per window.  Quant 4 runs the default selection (matrix-core kernel) and the gather kernel; quant 50 has only the
    gather kernel."""
    quant = cfg[2]
    case = _sized_case(cfg, ws, 0)
    _check_inputs(case, ws, 0, quant)
    want = _forward_want(cfg, ws, 0, dtype == torch.bfloat16)
    got = base._run(dev, case, ws, dtype)
    _check_forward(got, want, case, dtype, "default selection")
    if quant == 4:
        gather = _run_gather(dev, case, ws, dtype)
        _check_forward(gather, want, case, dtype, "gather kernel")
        if dtype == torch.float32:
            assert not np.array_equal(got, gather)          # two kernels did run (different summation order)


# ---------------------------------------------------------------------------------------------------------------
# the backward's LDS limit
# ---------------------------------------------------------------------------------------------------------------
def _bwd_lds_bytes(max_tokens, hd, axes):
    """launch_bwd's plan (swin_attn_bwd.hip): K and V rows of head_dim + 4 floats, dK and dV rows, the signal vectors,
    two logit rows per wave (4 waves) of max(64, max_tokens) floats, the row indices."""
    lcap = max(max_tokens, 64)
    return (max_tokens * (2 * (hd + 4) + 2 * hd + axes) + 2 * 4 * lcap) * 4 + max_tokens * 4


LDS_CFG = (2, 32, 4, "XYZ")
LDS_LIMIT = max(m for m in range(1, 513) if _bwd_lds_bytes(m, 32, 3) <= 160 * 1024)
SMALL = tuple(SIZES[7][:-1])           # the 7^3 list without its full window


@functools.lru_cache(maxsize=None)
def _backward_want(cfg, ws, shift, bf16, sizes=None):
    """float64 torch autograd over the restated forward -> (dout, out, [dq, dk, dv, dq_table, dk_table, dv_table])."""
    case = _sized_case(cfg, ws, shift, sizes)
    q, k, v, tabs, offs, w_sizes, w2n, n2n, cr = case
    dout = np.random.default_rng(1).normal(size=q.shape).astype(np.float32)
    ins = [q, k, v, dout]
    if bf16:
        ins = [_bf16_round(a) for a in ins]
    ref_in = [torch.from_numpy(np.array(a)).double().requires_grad_(True) for a in (*ins[:3], *tabs)]
    ref = base._crse_attention_torch(*ref_in, offs, w_sizes, w2n, n2n, cr)
    ref.backward(torch.from_numpy(ins[3]).double())
    return _frozen(dout), _frozen(ref.detach().numpy()), [_frozen(t.grad.numpy()) for t in ref_in]


def _check_backward(dev, case, want, dtype, unread):
    """Runs the taped op on the GPU and holds its output and six gradients to `want`."""
    from ptv3_hip import autograd as A
    q, k, v, tabs, offs, w_sizes, w2n, n2n, cr = case
    dout, ref_out, ref_grads = want
    t = lambda a, d=None: torch.from_numpy(np.array(a)).to(dev).to(d or torch.float32)
    dev_in = [t(a, dtype).requires_grad_(True) for a in (q, k, v)] + [t(a).requires_grad_(True) for a in tabs]
    w_start = torch.from_numpy(np.concatenate([w2n, [len(q)]]).astype(np.int32)).to(dev)
    out = A.swin_attention(*dev_in, offs, torch.from_numpy(n2n.astype(np.int64)).to(dev), w_start,
                           torch.from_numpy(np.array(cr)).to(dev), int(w_sizes.max()))
    fp32 = dtype == torch.float32
    assert out.dtype == dtype
    assert base._rel(out.detach().float().cpu().numpy(), ref_out) <= (1e-4 if fp32 else 1e-2)
    out.backward(t(dout, dtype))
    torch.cuda.synchronize()
    grads = [a.grad for a in dev_in]
    assert all(g.dtype == dtype for g in grads[:3]) and all(g.dtype == torch.float32 for g in grads[3:])
    grads = [g.float().cpu().numpy().astype(np.float64) for g in grads]
    failures = []
    for name, got, ref in zip(("dq", "dk", "dv"), grads[:3], ref_grads[:3]):
        rel = base._rel(got, ref)
        worst, tokens = _per_window_worst(np.abs(got - ref), case)
        scale = max(1.0, float(np.abs(ref).max()))
        print(f"{name}: rel L2 {rel:.3e}, worst window ({tokens} tokens) max-abs {worst:.3e} (|ref|max {scale:.3e})")
        if fp32 and rel > 1e-4:
            failures.append(f"{name}: rel L2 {rel:.3e}")
        if worst > (1e-4 if fp32 else BF16_OUT) * scale:
            failures.append(f"{name}: max-abs {worst:.3e} in a window of {tokens} tokens")
    starts = np.concatenate([[0], np.cumsum(offs)]).astype(np.int64)
    for name, got, ref in zip(("dq_table", "dk_table", "dv_table"), grads[3:], ref_grads[3:]):
        rel = base._rel(got, ref)
        print(f"{name}: rel L2 {rel:.3e}")
        if rel > 1e-4:
            failures.append(f"{name}: rel L2 {rel:.3e}")
        for a in range(len(offs)):                        # each signal axis on its own scale
            sl = slice(int(starts[a]), int(starts[a + 1]))
            err, scale = float(np.abs(got[sl] - ref[sl]).max()), float(np.abs(ref[sl]).max())
            print(f"  axis {a}: max-abs {err:.3e} (|ref|max {scale:.3e})")
            if err > 1e-4 * scale:
                failures.append(f"{name} axis {a}: max-abs {err:.3e} vs |ref|max {scale:.3e}")
        assert not ref[unread].any()
        if got[unread].any():                             # memset only, no atomic: exactly 0.0
            failures.append(f"{name}: {int(np.count_nonzero(got[unread]))} elements of unread rows are not 0.0")
    assert not failures, failures


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ws,shift", GEOMS)
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"h{c[0]}d{c[1]}q{c[2]}{c[3]}")
def test_crse_attention_backward_at_chosen_window_sizes(dev, cfg, ws, shift, dtype):
    """ptv3_swin_attn_bwd at windows of 1 .. 125 / 343 tokens and on the shifted partition (pieces up to 64 tokens at
    the model's shift 3, up to 216 at shift 1), max_tokens = the largest window as the model passes it.  fp32: dq, dk,
    dv and the table gradients relative L2 <= 1e-4; dq, dk, dv max-abs per window <= 1e-4 max(1, |ref|max); every
    signal axis of every table gradient max-abs <= 1e-4 |ref slice|max; rows no pair reads exactly 0.0.  bf16 (q, k,
    v, dout; reference on the rounded inputs): dq, dk, dv within one output rounding, 2^-7 max(1, |ref|max); the table
    gradients are fp32 sums of exactly upcast inputs and keep the fp32 limits.  No bitwise repeatability is asserted:
    dk, dv and the table gradients are atomic sums.
    head_dim 32 with the full 7^3 window is past the backward's LDS plan (203 056 bytes against 160 KB; 276 tokens is
    its limit, test_crse_attention_backward_at_its_lds_limit runs the same windows with the largest cut to 276): what
    the caller of the taped op sees there is the host-side refusal, after a forward that matches."""
    case = _sized_case(cfg, ws, shift)
    unread = _check_inputs(case, ws, shift, cfg[2])
    want = _backward_want(cfg, ws, shift, dtype == torch.bfloat16)
    if _bwd_lds_bytes(int(case[5].max()), cfg[1], len(case[4])) > 160 * 1024:
        assert (cfg, ws, shift) == (LDS_CFG, 7, 0)              # the one combination past the limit
        with pytest.raises(RuntimeError, match="bytes of LDS"):
            _check_backward(dev, case, want, dtype, unread)
        return
    _check_backward(dev, case, want, dtype, unread)


def test_crse_attention_backward_at_its_lds_limit(dev):
    """head_dim 32, XYZ: the largest window launch_bwd accepts (160 KB of dynamic LDS, the largest footprint the
    kernel ever requests), forward and backward, fp32, tolerances of the test above."""
    assert LDS_LIMIT == 276 and _bwd_lds_bytes(LDS_LIMIT + 1, 32, 3) > 160 * 1024 >= _bwd_lds_bytes(LDS_LIMIT, 32, 3)
    sizes = SMALL + (LDS_LIMIT,)
    case = _sized_case(LDS_CFG, 7, 0, sizes)
    assert int(case[5].max()) == LDS_LIMIT < 343 and {65, 129} <= set(case[5])
    reads = _row_reads(case)
    unread = np.concatenate([np.repeat(r == 0, 2 * 32) for r in reads])
    want = _forward_want(LDS_CFG, 7, 0, False, sizes)
    _check_forward(_run_gather(dev, case, 7, torch.float32), want, case, torch.float32, "gather kernel")
    _check_backward(dev, case, _backward_want(LDS_CFG, 7, 0, False, sizes), torch.float32, unread)


def test_crse_attention_backward_refuses_past_its_lds_limit(dev):
    """One token past the limit, and at the full 7^3 window, the backward refuses on the host before any launch; the
    forward (both kernels) takes max_tokens = 343 at head_dim 32."""
    from ptv3_hip import ops
    case = _sized_case(LDS_CFG, 7, 0, SMALL)
    q, k, v, tabs, offs, w_sizes, w2n, n2n, cr = case
    assert list(w_sizes) == list(SMALL)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    w_start = t(np.concatenate([w2n, [len(q)]]).astype(np.int32))
    args = (t(q), t(k), t(v), t(np.ones_like(q)), *(t(a) for a in tabs), offs, t(n2n.astype(np.int64)), w_start, t(cr))
    for max_tokens in (LDS_LIMIT + 1, 343):
        with pytest.raises(RuntimeError, match="bytes of LDS"):
            ops.swin_attention_bwd(*args, max_tokens)
    grads = ops.swin_attention_bwd(*args, LDS_LIMIT)              # the same call at the limit goes through
    torch.cuda.synchronize()
    assert all(torch.isfinite(g).all() for g in grads)
    want = _forward_want(LDS_CFG, 7, 0, False, SMALL)
    for env in (None, "0"):
        if env is not None:
            os.environ["PTV3_SWIN_ATTN_MFMA"] = env
        try:
            out = ops.swin_attention(*args[:3], *args[4:], 343)
            torch.cuda.synchronize()
        finally:
            os.environ.pop("PTV3_SWIN_ATTN_MFMA", None)
        _check_forward(out.cpu().numpy(), want, case, torch.float32, f"max_tokens 343, PTV3_SWIN_ATTN_MFMA={env}")
