"""The kernels whose serial load chains were broken into batches: slab sums (layernorm_kernel, block_head_kernel,
block_head_coop_kernel), weight staging (stage_matrix of block_head / block_tail / mlp2) and the pooling gather
(pool_feat_kernel).  A batch changes when a load is issued, never what is added or in which order, so every check
that has an unbatched counterpart is bitwise.

Slab sums.  The reference is the same op fed x = T(bias + slab_0 + slab_1 + ...), summed in fp32 in slab order on the
host (norm_ref.slab_input).  `splits` sits on both sides of every batch size the kernels use (slabs per batch: 16, 12
and 6 in the LayerNorm at c = 256, 48 and 512; 4, 2, 1 in the wave-local head; 8 and 4 in the cooperative head) and
includes 44, the level-4 count of the headline forward.  The slab buffer is longer than `splits` slabs and its tail is
NaN: a partial batch loads from a clamped slab index and must drop that sum.  "cancel" (1e8, 1, -1e8, ... down the
slabs) gives another sum as soon as a batch is summed on its own before it joins the bias; "negzero" holds -0.0 in every slab and in the bias, the sum a `+ 0.0f`
for a skipped slab would turn into +0.0 (a LayerNorm output cannot show the sign of a zero input: that case guards the
select against anything worse, the order case is the sharp one).

Staging.  C = 32 (the first batch of chunks is only partly filled: 32 * 32 / 8 = 128 bf16 chunks for 256 threads) and
C = 64, against the float64 block of test_hip_size_variants with its bounds, and bitwise between two calls.

Pooling.  Segments of 1, 8, 9 and 17 members (and 3, 4, 5, 16: fp32 rows go in batches of 4) in one call against a
segment maximum in torch."""
import numpy as np
import pytest
import torch

import norm_ref as R
from test_hip_size_variants import _Block, _bound, _err, _randn

pytestmark = pytest.mark.gpu

FP32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [FP32, BF16], ids=["fp32", "bf16"])
LN_SPLITS = (5, 6, 7, 8, 9, 11, 12, 13, 15, 16, 17, 32, 33, 44)
LN_ROWS = (1, 5, 245)
LN_WIDTHS = (48, 256, 512)          # 48: a partial channel group (12 chunks on 16 lanes); 512: two chunks per lane
HEAD_SPLITS = (1, 2, 3, 4, 5, 7, 8, 9)
NAN_TAIL = 3                        # slabs of NaN behind the ones in use


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _slabs(kind, splits, m, c, seed):
    """(slabs (splits, m, c) fp32, bias (c,) fp32) as numpy arrays"""
    rng = np.random.default_rng(seed)
    if kind == "randn":
        return rng.standard_normal((splits, m, c), dtype=np.float32), rng.standard_normal(c, dtype=np.float32)
    if kind == "cancel":
        col = np.array([1e8, 1.0, -1e8], dtype=np.float32)[np.arange(splits) % 3]
        slabs = np.broadcast_to(col[:, None, None], (splits, m, c)).copy()
        slabs[:, :, ::2] *= rng.uniform(0.5, 2.0, (1, m, (c + 1) // 2)).astype(np.float32)   # rows are not constant
        return slabs, rng.standard_normal(c, dtype=np.float32)
    assert kind == "negzero"
    return np.full((splits, m, c), -0.0, dtype=np.float32), np.full(c, -0.0, dtype=np.float32)


def _slab_buffer(slabs, dev):
    """the slabs on the device, followed by NAN_TAIL slabs of NaN"""
    tail = np.full((NAN_TAIL,) + slabs.shape[1:], np.nan, dtype=np.float32)
    return torch.from_numpy(np.concatenate([slabs, tail])).to(dev).contiguous()


def _summed(slabs, bias, dtype, dev):
    x = torch.from_numpy(R.slab_input(slabs, bias, dtype == BF16)).to(dev)
    return x.to(dtype).contiguous()


def _same(a, b):
    """bitwise equality (NaN == NaN, -0.0 != +0.0)"""
    ia = a.contiguous().view(torch.int32 if a.dtype == FP32 else torch.int16)
    ib = b.contiguous().view(torch.int32 if b.dtype == FP32 else torch.int16)
    return torch.equal(ia, ib)


# ------------------------------------------------------------------------------------------------
# ops.layernorm_slabs
# ------------------------------------------------------------------------------------------------
def _ln_pair(kind, splits, m, c, dtype, dev, chained):
    from ptv3_hip import ops
    slabs, bias = _slabs(kind, splits, m, c, seed=splits * 1000 + m + c)
    g = torch.Generator().manual_seed(c + splits)
    gamma, beta, gamma2, beta2 = (torch.randn(c, generator=g).to(dev) for _ in range(4))
    res = torch.randn(m, c, generator=g).to(dev).to(dtype) if chained else None
    kw = dict(res=res, gamma2=gamma2, beta2=beta2) if chained else {}
    want = ops.layernorm(_summed(slabs, bias, dtype, dev), gamma, beta, R.EPS, **kw)
    got = ops.layernorm_slabs(_slab_buffer(slabs, dev), splits, m, c, torch.from_numpy(bias).to(dev), dtype, gamma,
                              beta, R.EPS, **kw)
    return (want, got) if chained else ((want,), (got,))


@DTYPES
@pytest.mark.parametrize("c", LN_WIDTHS)
def test_layernorm_slabs_at_batch_boundaries(dev, c, dtype):
    for splits in LN_SPLITS:
        for m in LN_ROWS:
            want, got = _ln_pair("randn", splits, m, c, dtype, dev, chained=(splits + m) % 2 == 0)
            for w, g_ in zip(want, got):
                assert torch.isfinite(g_.float()).all(), ("NaN tail reached the sum", splits, m, c)
                assert _same(w, g_), (splits, m, c, (w.float() - g_.float()).abs().max().item())


@DTYPES
@pytest.mark.parametrize("kind", ["cancel", "negzero"])
def test_layernorm_slabs_order_and_signed_zero(dev, kind, dtype):
    for c in LN_WIDTHS:
        for splits in (7, 9, 17, 44):
            want, got = _ln_pair(kind, splits, 5, c, dtype, dev, chained=True)
            for w, g_ in zip(want, got):
                assert torch.isfinite(g_.float()).all() and _same(w, g_), (kind, splits, c)


def test_slab_input_keeps_order_and_signed_zero():
    """the host reference itself: "cancel" tells the slab-order sum from one that first sums a batch of slabs on its own
    and then adds it (bias + 1e8 loses the bias, bias + (1e8 + 1 - 1e8) keeps it); "negzero" sums to -0.0"""
    slabs, bias = _slabs("cancel", 9, 2, 8, seed=0)
    batched = bias[None, :].astype(np.float32)
    for z0 in range(0, 9, 3):
        part = slabs[z0]
        for z in range(z0 + 1, z0 + 3):
            part = part + slabs[z]
        batched = batched + part
    assert not np.array_equal(R.slab_input(slabs, bias, False), batched)
    slabs, bias = _slabs("negzero", 9, 2, 8, seed=0)
    assert np.signbit(R.slab_input(slabs, bias, False)).all()


# ------------------------------------------------------------------------------------------------
# ops.block_head with slabs
# ------------------------------------------------------------------------------------------------
def _head_pair(blk, kind, splits, m, dtype, dev, permute):
    from ptv3_hip import ops
    c = blk.c
    slabs, bias = _slabs(kind, splits, m, c, seed=splits * 100 + m + c)
    g = torch.Generator().manual_seed(m + splits)
    shortcut = torch.randn(m, c, generator=g).to(dev).to(dtype)
    head_args, _ = blk.dev_args(dev, dtype, permute)
    want = ops.block_head(_summed(slabs, bias, dtype, dev), None, 0, None, shortcut, *head_args)
    got = ops.block_head(None, _slab_buffer(slabs, dev), splits, torch.from_numpy(bias).to(dev), shortcut, *head_args)
    return want, got


# C = 512 has no fp32 fused halves (its cooperative tail does not fit LDS, so ptv3_block_fusable answers 0 and
# ptv3_block_head rejects the call): that width is a bf16 case only
HEAD_CASES = [(c, dt) for c in (32, 64, 128, 256, 512) for dt in (FP32, BF16) if (c, dt) != (512, FP32)]


def test_block_head_has_no_fp32_c512(dev):
    from ptv3_hip import ops
    assert ops.block_fusable(512, 2048, FP32) == 0 and ops.block_fusable(512, 2048, BF16) == 2


@pytest.mark.parametrize("c,dtype", HEAD_CASES, ids=[f"c{c}-{'fp32' if dt == FP32 else 'bf16'}" for c, dt in HEAD_CASES])
def test_block_head_slabs_at_batch_boundaries(dev, c, dtype):
    from ptv3_hip import ops
    chain = c <= 64
    assert ops.block_fusable(c, 4 * c, dtype) == (1 if chain else 2)
    blk = _Block(c, seed=c)
    for m in ((1, 63, 65) if chain else (1, 17)):
        for splits in HEAD_SPLITS:
            for kind in (("randn", "cancel", "negzero") if splits == 9 else ("randn",)):
                want, got = _head_pair(blk, kind, splits, m, dtype, dev, chain and dtype == BF16)
                for nm, w, g_ in zip(("f1", "qkv"), want, got):
                    assert torch.isfinite(g_.float()).all(), ("NaN tail reached the sum", nm, kind, splits, m, c)
                    assert _same(w, g_), (nm, kind, splits, m, c)


# ------------------------------------------------------------------------------------------------
# weight staging: block_head, block_tail, mlp2
# ------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("c", [32, 64])
def test_staged_block_halves(dev, c, dtype):
    from ptv3_hip import ops
    blk = _Block(c, seed=3 * c)
    head_args, tail_args = blk.dev_args(dev, dtype, dtype == BF16)
    gen = torch.Generator(device=dev).manual_seed(c)
    for m in (1, 64, 200):
        x, shortcut = _randn(m, c, dtype, gen, dev, 1.5, 0.3), _randn(m, c, dtype, gen, dev)
        attn, f1_in = _randn(m, c, dtype, gen, dev), _randn(m, c, dtype, gen, dev)
        f1, qkv = ops.block_head(x, None, 0, None, shortcut, *head_args)
        out = ops.block_tail(attn, f1_in, *tail_args)
        f1_ref, qkv_ref = blk.head_ref(x.double().cpu(), shortcut.double().cpu(), dtype)
        out_ref = blk.tail_ref(attn.double().cpu(), f1_in.double().cpu(), dtype)
        for nm, got, ref in (("f1", f1, f1_ref), ("qkv", qkv, qkv_ref), ("out", out, out_ref)):
            e, b = _err(got, ref), _bound(dtype, ref)
            print(f"staged c={c} {dtype} m={m} {nm}: {e:.3e} (bound {b:.3e})")
            assert e < b, (nm, m, c, dtype, e, b)
        again = ops.block_head(x, None, 0, None, shortcut, *head_args) + (ops.block_tail(attn, f1_in, *tail_args),)
        for nm, a, b in zip(("f1", "qkv", "out"), (f1, qkv, out), again):
            assert _same(a, b), ("two calls differ", nm, m, c, dtype)


@DTYPES
@pytest.mark.parametrize("cin", [32, 64])
def test_staged_mlp2(dev, cin, dtype):
    from ptv3_hip import ops
    F = torch.nn.functional
    hidden, cout = 4 * cin, 12
    assert ops.mlp2_fusable(cin, hidden, cout, dtype)
    g = torch.Generator().manual_seed(cin)
    w1, b1 = torch.randn(hidden, cin, generator=g) / cin ** 0.5, torch.randn(hidden, generator=g)
    s1, t1 = torch.rand(hidden, generator=g) + 0.5, torch.randn(hidden, generator=g)
    w2, b2 = torch.randn(cout, hidden, generator=g) / hidden ** 0.5, torch.randn(cout, generator=g)
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    w2p = ops.mlp2_weight2(d(w2), dtype)
    for m in (1, 64, 200):
        x = torch.randn(m, cin, generator=g).to(dtype)
        args = (d(x), d(w1).to(dtype), d(b1), d(s1), d(t1), ops.ACT_GELU, w2p, d(b2), cout)
        out = ops.mlp2(*args)
        v = lambda t: t.to(dtype).double()  # noqa: E731
        ref = F.linear(F.gelu((F.linear(x.double(), v(w1), b1.double())) * s1.double() + t1.double()), v(w2), b2.double())
        e, b = _err(out, ref), _bound(dtype, ref)
        print(f"staged mlp2 cin={cin} {dtype} m={m}: {e:.3e} (bound {b:.3e})")
        assert out.dtype == FP32 and e < b, (m, cin, dtype, e, b)
        assert _same(out, ops.mlp2(*args)), ("two calls differ", m, cin, dtype)


# ------------------------------------------------------------------------------------------------
# ops.pool_max
# ------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("c", [16, 64, 512])
def test_pool_max_across_member_batches(dev, c, dtype):
    from ptv3_hip import ops
    lengths = [1, 8, 9, 17, 3, 4, 5, 16, 1, 8] * 7          # 70 segments: more than one workgroup at c = 512
    n = sum(lengths)
    g = torch.Generator().manual_seed(c)
    feat = torch.randn(n, c, generator=g).to(dtype)
    order0 = torch.randperm(n, generator=g)
    seg = torch.tensor([0] + lengths).cumsum(0)
    ref = torch.stack([feat[order0[a:b]].float().max(0).values for a, b in zip(seg[:-1].tolist(), seg[1:].tolist())])
    got = ops.pool_max(feat.to(dev), order0.to(dev), seg.int().to(dev), len(lengths))
    assert got.dtype == dtype and _same(got.cpu(), ref.to(dtype)), (c, dtype)
