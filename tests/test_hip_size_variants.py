"""GPU parity of the row-count-selected kernel variants at their switch points (default thresholds, chosen by m):

- the fused block halves (ptv3_block_head / ptv3_block_tail): one 16-row tile per wave up to 32 767 rows, two from
  32 768 (row_tiles); workgroups that loop over row blocks once the grid cap is reached (head: 1024 workgroups of 64
  rows, resident-weight tail: 512 of 128 rows); the non-resident tail of C = 64 fp32; the cooperative C = 128 kernels
  up to coop_max_rows(128) = 16 384; the weight-streaming kernels from 24 576 rows up to the last row count whose
  output stays below 2^31 - 2^20 bytes (buffer stores with 32-bit byte offsets and num_records);
- ptv3_rows_linear at the same byte limit;
- the BatchNorm training reductions (col_reduce row chunks, bn_finalize, act_bwd, affine2) from 0 to 4M rows.

Every output row of the block and row kernels depends only on its own input row, so the multi-GB cases are checked on
sampled rows (both ends, the rows around the 2^30 and 2^31 - 2^20 byte offsets of every output, seeded random rows)
against float64 torch, and the profiler names the kernel that ran."""
import pytest
import torch

pytestmark = pytest.mark.gpu

F = torch.nn.functional
FP32_TOL = 1e-4
BF16_STEP = 2.0 ** -8
BYTE_LIMIT = (1 << 31) - (1 << 20)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _esize(dtype):
    return 4 if dtype == torch.float32 else 2


def _m_max(row_bytes):
    """largest m with m * row_bytes < 2^31 - 2^20"""
    return (BYTE_LIMIT - 1) // row_bytes


def _sample_rows(m, row_bytes, seed):
    """first and last 256 rows, the rows holding (and next to) the bytes 2^30 and 2^31 - 2^20 - 1 of every output whose
    row is `row_bytes` wide, 2048 seeded random rows"""
    rows = set(range(min(256, m))) | set(range(max(0, m - 256), m))
    for rb in row_bytes:
        for b in (1 << 30, BYTE_LIMIT - 1):
            r = b // rb
            rows |= {q for q in (r - 1, r, r + 1) if 0 <= q < m}
    g = torch.Generator().manual_seed(seed)
    rows |= set(torch.randint(0, m, (2048,), generator=g).tolist())
    return torch.tensor(sorted(rows), dtype=torch.int64)


def _kernels(fn):
    """run fn with the launch profiler on -> (fn's result, names of the kernels that ran)"""
    from ptv3_hip import ops
    ops.profile_enable(True)
    try:
        res = fn()
        torch.cuda.synchronize()
        names = set(ops.profile_collect_kernels())
        ops.profile_collect()          # resets the records
    finally:
        ops.profile_enable(False)
    return res, names


def _randn(m, c, dtype, gen, dev, scale=1.0, shift=0.0):
    t = torch.randn(m, c, generator=gen, device=dev)
    if scale != 1.0 or shift != 0.0:
        t.mul_(scale).add_(shift)
    return t.to(dtype) if dtype != torch.float32 else t


def _err(got, ref):
    return (got.double().cpu() - ref).abs().max().item()


def _bound(dtype, ref, steps=8):
    scale = max(1.0, ref.abs().max().item())
    return FP32_TOL * scale if dtype == torch.float32 else steps * BF16_STEP * scale


class _Block:
    """seeded weights of one PTv3 block (fp32 master copies) and the float64 reference of its two fused halves"""

    def __init__(self, c, seed):
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        self.c = c
        self.g0, self.b0, self.g1, self.b1, self.g2, self.b2 = (rnd(c) for _ in range(6))
        self.wqkv, self.bqkv = rnd(3 * c, c) / c ** 0.5, rnd(3 * c)
        self.wproj, self.bproj = rnd(c, c) / c ** 0.5, rnd(c)
        self.w1, self.bias1 = rnd(4 * c, c) / c ** 0.5, rnd(4 * c)
        self.w2, self.bias2 = rnd(c, 4 * c) / (4 * c) ** 0.5, rnd(c)

    def w(self, name, dtype):
        """weight as the kernels see it, in float64 (bf16-rounded in bf16 mode)"""
        return getattr(self, name).to(dtype).double()

    def head_ref(self, x, shortcut, dtype):
        c, v = self.c, lambda t: t.double()  # noqa: E731
        f1 = F.layer_norm(x, (c,), v(self.g0), v(self.b0), 1e-5) + shortcut
        qkv = F.linear(F.layer_norm(f1, (c,), v(self.g1), v(self.b1), 1e-5), self.w("wqkv", dtype), v(self.bqkv))
        return f1, qkv

    def tail_ref(self, attn, f1, dtype):
        c, v = self.c, lambda t: t.double()  # noqa: E731
        f2 = F.linear(attn, self.w("wproj", dtype), v(self.bproj)) + f1
        h = F.gelu(F.linear(F.layer_norm(f2, (c,), v(self.g2), v(self.b2), 1e-5), self.w("w1", dtype), v(self.bias1)))
        return f2 + F.linear(h, self.w("w2", dtype), v(self.bias2))

    def dev_args(self, dev, dtype, permute):
        from ptv3_hip import ops
        d = lambda t: t.to(dev).contiguous()  # noqa: E731
        cv = lambda t: d(t).to(dtype).contiguous()  # noqa: E731
        pm = (lambda t: ops.chain_permute(cv(t), dtype)) if permute else cv  # noqa: E731
        head = (d(self.g0), d(self.b0), d(self.g1), d(self.b1), pm(self.wqkv), d(self.bqkv), 1e-5)
        tail = (cv(self.wproj), d(self.bproj), d(self.g2), d(self.b2), pm(self.w1), d(self.bias1), pm(self.w2),
                d(self.bias2), 1e-5)
        return head, tail

    def unfused_head(self, x, shortcut, dev, dtype):
        """LayerNorm + tiled GEMM launches the fused head replaces, on the same (sampled) device rows"""
        from ptv3_hip import ops
        d = lambda t: t.to(dev).contiguous()  # noqa: E731
        f1, t3 = ops.layernorm(x, d(self.g0), d(self.b0), 1e-5, res=shortcut, gamma2=d(self.g1), beta2=d(self.b1))
        return f1, ops.gemm(t3, d(self.wqkv).to(dtype), bias=d(self.bqkv))

    def unfused_tail(self, attn, f1, dev, dtype):
        from ptv3_hip import ops
        d = lambda t: t.to(dev).contiguous()  # noqa: E731
        f2 = ops.gemm(attn, d(self.wproj).to(dtype), bias=d(self.bproj), res=f1)
        t6 = ops.gemm(ops.layernorm(f2, d(self.g2), d(self.b2), 1e-5), d(self.w1).to(dtype), bias=d(self.bias1),
                      act=ops.ACT_GELU)
        return ops.gemm(t6, d(self.w2).to(dtype), bias=d(self.bias2), res=f2)


def _check_halves(blk, dev, dtype, m, x, shortcut, attn, f1_in, head_kernel, tail_kernel, permute, seed, report):
    """run both fused halves on m rows (x / shortcut / attn / f1_in hold at least m rows), check the kernel names
    and the sampled rows against float64 and (bf16) against the unfused launches"""
    from ptv3_hip import ops
    c, es = blk.c, _esize(dtype)
    head_args, tail_args = blk.dev_args(dev, dtype, permute)
    (f1, qkv), names = _kernels(lambda: ops.block_head(x[:m], None, 0, None, shortcut[:m], *head_args))
    assert names == {head_kernel}, (m, dtype, names)
    idx = _sample_rows(m, (c * es, 3 * c * es), seed)
    di = idx.to(dev)
    xs, ss = x.index_select(0, di), shortcut.index_select(0, di)
    f1_ref, qkv_ref = blk.head_ref(xs.double().cpu(), ss.double().cpu(), dtype)
    f1s, qkvs = f1.index_select(0, di), qkv.index_select(0, di)
    del f1, qkv
    errs = {}
    for nm, got, ref in (("f1", f1s, f1_ref), ("qkv", qkvs, qkv_ref)):
        errs[nm] = e = _err(got, ref)
        assert e < _bound(dtype, ref), (nm, m, dtype, e, _bound(dtype, ref))
    if dtype == torch.bfloat16:
        for nm, got, ref in zip(("f1", "qkv"), (f1s, qkvs), blk.unfused_head(xs, ss, dev, dtype)):
            e = (got.float() - ref.float()).abs().max().item()
            assert e <= _bound(dtype, ref.float(), steps=4), (nm, "vs unfused", m, e)
    if attn is None:
        report(errs)
        return
    out, names = _kernels(lambda: ops.block_tail(attn[:m], f1_in[:m], *tail_args))
    assert names == {tail_kernel}, (m, dtype, names)
    idx = _sample_rows(m, (c * es,), seed + 1)
    di = idx.to(dev)
    asmp, fsmp = attn.index_select(0, di), f1_in.index_select(0, di)
    out_ref = blk.tail_ref(asmp.double().cpu(), fsmp.double().cpu(), dtype)
    outs = out.index_select(0, di)
    del out
    errs["out"] = e = _err(outs, out_ref)
    assert e < _bound(dtype, out_ref), ("out", m, dtype, e, _bound(dtype, out_ref))
    if dtype == torch.bfloat16:
        ref = blk.unfused_tail(asmp, fsmp, dev, dtype).float()
        e = (outs.float() - ref).abs().max().item()
        assert e <= _bound(dtype, ref, steps=4), ("out vs unfused", m, e)
    report(errs)


def _reporter(tag):
    def report(errs):
        print(f"{tag}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    return report


# ------------------------------------------------------------------------------------------------
# fused block halves: wave-local register chain (C = 32, 64)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_chain_block_halves_at_row_switches(dev, c, dtype):
    """m = 32 767 (last one-tile case), 32 768 (first RT = 2 case), 65 536 (head: last grid without looping; tail: 512
    workgroups x 128 rows exactly), 65 537 and 100 003 (both halves loop, ragged last tile).  C = 64 fp32 takes the
    tail without resident weights (its weights exceed 96 KB of LDS)."""
    from ptv3_hip import ops
    assert ops.block_fusable(c, 4 * c, dtype) == 1
    blk = _Block(c, seed=c)
    gen = torch.Generator(device=dev).manual_seed(1000 + c)
    M = 100003
    x, shortcut = _randn(M, c, dtype, gen, dev, 1.5, 0.3), _randn(M, c, dtype, gen, dev)
    attn, f1_in = _randn(M, c, dtype, gen, dev), _randn(M, c, dtype, gen, dev)
    for m in (32767, 32768, 65536, 65537, M):
        _check_halves(blk, dev, dtype, m, x, shortcut, attn, f1_in, "block_head_kernel", "block_tail_kernel",
                      dtype == torch.bfloat16, seed=m, report=_reporter(f"chain c={c} {dtype} m={m}"))


# ------------------------------------------------------------------------------------------------
# fused block halves: cooperative (C = 128 up to 16 384 rows) and weight-streaming (C = 128, 256 from 24 576 rows)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_coop_block_halves_at_their_row_limit(dev, dtype):
    from ptv3_hip import ops
    c, m = 128, 16384
    assert ops.block_fusable(c, 4 * c, dtype, m) == 2
    assert ops.block_fusable(c, 4 * c, dtype, m + 1) == 0        # 16 385 .. 24 575: unfused / rows_linear path
    assert ops.block_fusable(c, 4 * c, dtype, 24575) == 0
    assert ops.block_fusable(c, 4 * c, dtype, 24576) == 3
    blk = _Block(c, seed=7)
    gen = torch.Generator(device=dev).manual_seed(77)
    x, shortcut = _randn(m, c, dtype, gen, dev, 1.5, 0.3), _randn(m, c, dtype, gen, dev)
    attn, f1_in = _randn(m, c, dtype, gen, dev), _randn(m, c, dtype, gen, dev)
    _check_halves(blk, dev, dtype, m, x, shortcut, attn, f1_in, "block_head_coop_kernel", "block_tail_coop_kernel",
                  False, seed=m, report=_reporter(f"coop c={c} {dtype} m={m}"))


@pytest.mark.parametrize("c", [128, 256])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_wide_block_halves_at_their_byte_limit(dev, c, dtype):
    """m = 24 576 (first streaming case) and m_max, the last row count whose qkv stays below 2^31 - 2^20 bytes; at
    m_max + 1 the streaming kernels are not served and the head falls back to the cooperative kernel."""
    from ptv3_hip import ops
    es = _esize(dtype)
    m_max = _m_max(3 * c * es)
    assert m_max == {1536: 1397418, 3072: 698709, 768: 2794837}[3 * c * es]
    assert ops.block_fusable(c, 4 * c, dtype, 24576) == 3
    assert ops.block_fusable(c, 4 * c, dtype, 24575) != 3
    assert ops.block_fusable(c, 4 * c, dtype, m_max) == 3
    assert ops.block_fusable(c, 4 * c, dtype, m_max + 1) != 3
    blk = _Block(c, seed=c + 1)
    gen = torch.Generator(device=dev).manual_seed(2000 + c)
    M = m_max + 1
    try:
        x, shortcut = _randn(M, c, dtype, gen, dev, 1.5, 0.3), _randn(M, c, dtype, gen, dev)
        attn, f1_in = _randn(M, c, dtype, gen, dev), _randn(M, c, dtype, gen, dev)
        for m in (24576, m_max):
            _check_halves(blk, dev, dtype, m, x, shortcut, attn, f1_in, "block_head_wide_kernel",
                          "block_tail_wide_kernel", False, seed=m, report=_reporter(f"wide c={c} {dtype} m={m}"))
        del attn, f1_in
        _check_halves(blk, dev, dtype, M, x, shortcut, None, None, "block_head_coop_kernel", None, False, seed=M,
                      report=_reporter(f"wide->coop c={c} {dtype} m={M}"))
    finally:
        x = shortcut = attn = f1_in = None
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# rows_linear at its byte limit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,cout,dtype", [(512, 2048, torch.bfloat16), (256, 1024, torch.float32)],
                         ids=["c512-bf16", "c256-fp32"])
def test_rows_linear_at_its_byte_limit(dev, c, cout, dtype):
    """all three prologues at m_max = 524 031, the last row count whose (m, cout) output stays below 2^31 - 2^20 bytes"""
    from ptv3_hip import ops
    es = _esize(dtype)
    m = _m_max(cout * es)
    assert m == 524031
    assert ops.rows_linear_capable(c, cout, dtype, m)
    assert not ops.rows_linear_capable(c, cout, dtype, m + 1)
    g = torch.Generator().manual_seed(c + cout)
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    g0, b0, g1, b1 = rnd(c), rnd(c), rnd(c), rnd(c)
    w, bias = rnd(cout, c) / c ** 0.5, rnd(cout)
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    wd = d(w).to(dtype)
    w64, v = w.to(dtype).double(), lambda t: t.double()  # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(3000 + c)
    idx = _sample_rows(m, (c * es, cout * es), seed=c)
    di = idx.to(dev)
    report = _reporter(f"rows c={c} cout={cout} {dtype} m={m}")
    errs = {}
    try:
        x, shortcut = _randn(m, c, dtype, gen, dev, 1.5, 0.3), _randn(m, c, dtype, gen, dev)
        xs, ss = x.index_select(0, di), shortcut.index_select(0, di)
        x64, s64 = xs.double().cpu(), ss.double().cpu()
        # prologue 0: proj + residual
        res = _randn(m, cout, dtype, gen, dev)
        rs = res.index_select(0, di)
        out, names = _kernels(lambda: ops.rows_linear(x, wd, d(bias), res=res))
        del res
        assert names == {"rows_linear_kernel"}, names
        cases = [("proj", out.index_select(0, di), F.linear(x64, w64, v(bias)) + rs.double().cpu(),
                  ops.gemm(xs, wd, bias=d(bias), res=rs))]
        del out
        # prologue 1: LayerNorm -> fc1 -> GELU
        out, names = _kernels(lambda: ops.rows_linear(x, wd, d(bias), act=ops.ACT_GELU, ln=(d(g1), d(b1))))
        assert names == {"rows_linear_kernel"}, names
        cases.append(("fc1", out.index_select(0, di),
                      F.gelu(F.linear(F.layer_norm(x64, (c,), v(g1), v(b1), 1e-5), w64, v(bias))),
                      ops.gemm(ops.layernorm(xs, d(g1), d(b1), 1e-5), wd, bias=d(bias), act=ops.ACT_GELU)))
        del out
        # prologue 2: LayerNorm + shortcut -> stored f1 -> LayerNorm -> linear
        (f1, out), names = _kernels(lambda: ops.rows_linear(x, wd, d(bias), ln=(d(g1), d(b1)), ln0=(d(g0), d(b0)),
                                                            shortcut=shortcut))
        assert names == {"rows_linear_kernel"}, names
        f1_ref = F.layer_norm(x64, (c,), v(g0), v(b0), 1e-5) + s64
        f1u, t3 = ops.layernorm(xs, d(g0), d(b0), 1e-5, res=ss, gamma2=d(g1), beta2=d(b1))
        cases.append(("f1", f1.index_select(0, di), f1_ref, f1u))
        cases.append(("ln-linear", out.index_select(0, di),
                      F.linear(F.layer_norm(f1_ref, (c,), v(g1), v(b1), 1e-5), w64, v(bias)),
                      ops.gemm(t3, wd, bias=d(bias))))
        del f1, out, x, shortcut
        for nm, got, ref, unfused in cases:
            errs[nm] = e = _err(got, ref)
            assert e < _bound(dtype, ref), (nm, e, _bound(dtype, ref))
            if dtype == torch.bfloat16:
                e = (got.float() - unfused.float()).abs().max().item()
                assert e <= _bound(dtype, unfused.float(), steps=4), (nm, "vs unfused", e)
        report(errs)
    finally:
        x = shortcut = res = out = f1 = None
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# BatchNorm training reductions
# ------------------------------------------------------------------------------------------------
_ACTS = {"none": (lambda t: t), "gelu": F.gelu, "relu": F.relu}


def _bn_case(dev, m, c, dtype, training, act, seed):
    """A.batch_norm_act (fp32 parameters, x / dy in `dtype`) against torch.nn.BatchNorm1d in float64 on the same
    (rounded) x and dy: y, dx, dgamma, dbeta and both running statistics"""
    import copy
    from ptv3_hip import autograd as A, ops
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(m, c, generator=g) * 1.7 + 3.0).to(dtype)
    dy = torch.randn(m, c, generator=g).to(dtype)
    bn = torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)
    with torch.no_grad():
        bn.weight.copy_(torch.randn(c, generator=g)); bn.bias.copy_(torch.randn(c, generator=g))
        bn.running_mean.copy_(torch.randn(c, generator=g)); bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    bn.train(training)
    bnd = copy.deepcopy(bn).to(dev)
    bn64 = copy.deepcopy(bn).double()
    xd = x.to(dev).requires_grad_(True)
    yd = A.batch_norm_act(xd, bnd, {"none": ops.ACT_NONE, "gelu": ops.ACT_GELU, "relu": ops.ACT_RELU}[act])
    yd.backward(dy.to(dev))
    xr = x.double().requires_grad_(True)
    zr = bn64(xr)
    if act == "relu":
        # a pre-activation within fp32 rounding of 0 may land on either side of the step: take the kernel's side there
        z = zr.detach()
        keep = torch.where(z.abs() < 1e-5, (yd.detach().float().cpu() > 0).double(), (z > 0).double())
        yr = zr * keep
    else:
        yr = _ACTS[act](zr)
    yr.backward(dy.double())
    out = {}
    # bf16: y, dx and the activation gradient in front of the dgamma / dbeta sums are stored in bf16 -> a few bf16
    # steps of their scale; the running statistics are fp32 sums of the bf16 x
    tol = 1e-4 if dtype == torch.float32 else 4 * BF16_STEP
    for nm, got, ref, tol in (("y", yd, yr.detach(), tol), ("dx", xd.grad, xr.grad, tol),
                              ("dgamma", bnd.weight.grad, bn64.weight.grad, tol),
                              ("dbeta", bnd.bias.grad, bn64.bias.grad, tol),
                              ("running_mean", bnd.running_mean, bn64.running_mean, 1e-4),
                              ("running_var", bnd.running_var, bn64.running_var, 1e-4)):
        out[nm] = e = _err(got, ref)
        assert e <= tol * max(1.0, ref.abs().max().item()), (nm, m, c, dtype, training, act, e)
    return out


@pytest.mark.parametrize("m,c", [(m, c) for c in (32, 64, 512) for m in (2, 63, 65, 100003)] + [(1000003, 32)])
def test_batchnorm_act_across_row_chunkings(dev, m, c):
    """row counts below one 16-row chunk, around 64, and past 256 chunks (chunk size grows with m); m = 2 checks the
    unbiased factor m / (m - 1) of the running variance"""
    worst = {}
    for training in (True, False):
        for act in _ACTS:
            for k, e in _bn_case(dev, m, c, torch.float32, training, act, seed=m + c).items():
                worst[k] = max(worst.get(k, 0.0), e)
    print(f"batch_norm_act m={m} c={c} fp32: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("m,c", [(65, 64), (100003, 64), (4099, 512)])
def test_batchnorm_act_bf16(dev, m, c):
    for training in (True, False):
        for act in _ACTS:
            _bn_case(dev, m, c, torch.bfloat16, training, act, seed=m * 3 + c)


_CR_SHAPES = [(m, c) for m in (0, 1, 15, 16, 1025, 100003) for c in (1, 19, 63, 64, 65, 512)] + \
    [(4194307, c) for c in (1, 19, 63, 64, 65)]


@pytest.mark.parametrize("m,c", _CR_SHAPES)
def test_col_reduce_modes(dev, m, c):
    """ops.col_reduce, modes 0-3 with mu given as column sums and mu_scale = 1 / m (as BatchNorm calls it), against
    float64 sums: within 1e-6 of each column's sum of |terms|.  Odd class counts (19) reach it through
    LinearFn.backward."""
    from ptv3_hip import ops
    gen = torch.Generator(device=dev).manual_seed(m * 131 + c)
    dtypes = (torch.float32, torch.bfloat16) if m <= 100003 else (torch.float32,)
    for dtype in dtypes:
        a = _randn(m, c, dtype, gen, dev, 1.7, 3.0)
        b = _randn(m, c, dtype, gen, dev, 0.5, -1.0)
        mu = (a.double().sum(0) + 0.25).float().contiguous()
        rs = (torch.rand(c, generator=gen, device=dev) + 0.5).contiguous()
        mu_scale = 1.0 / (m + 3)        # != 1 at every m, m = 0 and 1 included
        mc = (mu * torch.tensor(mu_scale, dtype=torch.float32, device=dev)).double()   # the kernel scales in fp32
        a64, b64 = a.double(), b.double()
        t = [a64, a64 * a64, a64 * ((b64 - mc) * rs.double()), (a64 - mc) ** 2]
        for mode in range(4):
            got = ops.col_reduce(a, b if mode == 2 else None, mu if mode >= 2 else None, rs if mode == 2 else None,
                                 mode=mode, mu_scale=mu_scale)
            got = got.reshape(1 if mode == 0 else 2, c).double()
            terms = [t[0]] + ([t[mode]] if mode else [])
            for q, tq in enumerate(terms):
                ref, mag = tq.sum(0), tq.abs().sum(0)
                err = (got[q] - ref).abs()
                assert bool((err <= 1e-6 * mag).all()), (dtype, mode, q, (err / mag.clamp_min(1e-300)).max().item())
        del a, b, t, a64, b64
    torch.cuda.empty_cache()


@pytest.mark.parametrize("m,c", [(100003, 64), (4194307, 32), (100003, 512)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_act_bwd_and_affine2_at_large_m(dev, m, c, dtype):
    """dy * act'(x * scale + shift) (with and without scale / shift) and ca * dy + cb * x + cc against float64"""
    from ptv3_hip import ops
    gen = torch.Generator(device=dev).manual_seed(m + c)
    x, dy = _randn(m, c, dtype, gen, dev, 1.5, 0.2), _randn(m, c, dtype, gen, dev)
    vec = lambda: torch.randn(c, generator=gen, device=dev).contiguous()  # noqa: E731
    scale, shift = vec(), vec()
    x64, dy64 = x.double(), dy.double()
    tol = FP32_TOL if dtype == torch.float32 else 2 * BF16_STEP
    for act, fn in ((ops.ACT_GELU, F.gelu), (ops.ACT_RELU, F.relu)):
        for s in (None, (scale, shift)):
            z = (x64 * s[0].double() + s[1].double()) if s else x64
            z = z.detach().requires_grad_(True)
            fn(z).backward(dy64)
            ref = z.grad
            got = ops.act_bwd(dy, x, act, *(s or (None, None)))
            if act == ops.ACT_RELU:      # a z within fp32 rounding of 0 may take the other side of the step
                near = z.detach().abs() < 1e-6 * (1 + (x64 * s[0].double()).abs() + s[1].double().abs() if s else 1)
                got, ref = got.double().masked_fill(near, 0), ref.masked_fill(near, 0)
            e = (got.double() - ref).abs().max().item()
            assert e <= tol * max(1.0, ref.abs().max().item()), (act, s is None, e)
            del z, ref, got
    ca, cb, cc = vec(), vec(), vec()
    ref = ca.double() * dy64 + cb.double() * x64 + cc.double()
    got = ops.affine2(dy, x, ca, cb, cc)
    e = (got.double() - ref).abs().max().item()
    assert e <= tol * max(1.0, ref.abs().max().item()), e
    del x, dy, x64, dy64, ref, got
    torch.cuda.empty_cache()
