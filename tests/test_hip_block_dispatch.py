"""Which kernels one eval PTv3 block launches, branch by branch of Block._eval_after_cpe, for Block and BlockPlus.

Every case is one block built directly, in eval(), on a seeded cloud of two scenes with unique voxels (patch 48, orders
"z" / "z-trans").  A case first asserts the capability answers that put it on its branch (ptv3_block_fusable,
ptv3_rows_linear_capable, ptv3_gemm_splits, use_fused_cpe), so a moved threshold fails here instead of silently testing
another branch; then the whole {kernel: launches} dict of the launch profiler against EXPECTED, and the output against
the same block's _forward_generic on the same input.

EXPECTED was recorded with the commit before Block and BlockPlus shared their dispatch (two copies of it then), by
run_case() below, and is not to be re-recorded from the code under test: a changed dict means a configuration changed
branches.  What the shapes reach (fp32 | bf16 where they differ):

  Block c=32 n=777         register-chain halves; the fp32 conv splits over K, so its head sums the slabs
  Block c=128 n=333        cooperative halves fed by slabs
  Block c=128 n=16385      no fused halves in that row range, conv does not split -> ptv3_rows_linear chain
  Block c=128 n=24653      weight-streaming halves
  Block c=512 n=245        not fusable; conv splits -> ptv3_layernorm_slabs + qkv GEMM; the tail is GEMMs in fp32 (not
                           rows-capable) and ptv3_rows_linear in bf16: slabs win over the rows path at the head only
  BlockPlus k=5 c=64       fused front, composed 125-tap conv, chain halves
  BlockPlus k=5 c=128      rows chain with ln0 = cpe[8]
  BlockPlus k=5 c=512      (512, 128) is in FUSED_FRONT_OFF: composed front; ptv3_layernorm + GEMMs
  Block qkv_bias=False     the fused head reads bqkv unconditionally: such a block takes the unfused kernels

The profiler brackets the GEMM, convolution, attention, rows-linear and fused-block kernels; LayerNorm, activation and
the geometry kernels (neighbour table, pad plan, window maps) do not appear in its dicts.  In the recording run max |fused - generic| / max(1, |generic|max) was
2.2e-7 to 1.0e-6 in fp32 (bound 1e-4) and 7.2e-3 to 1.3e-2 in bf16 (bound 8 * 2^-8 = 3.1e-2), so no case needs a bound
of its own."""
import pytest
import torch

from test_hip_size_variants import _bound

pytestmark = pytest.mark.gpu

FP32, BF16 = torch.float32, torch.bfloat16
SLAB_SHAPES = [(512, 245), (512, 37), (256, 100)]     # the first whose 27-tap conv splits over K is the slab case


class Case:
    def __init__(self, kind, c, n, dtype, fusable=None, slabs=None, rows=None, front=None, qkv_bias=True):
        self.kind, self.c, self.n, self.dtype, self.qkv_bias = kind, c, n, dtype, qkv_bias
        self.fusable, self.slabs, self.rows, self.front = fusable, slabs, rows, front
        self.id = "-".join([kind, f"c{c}", f"n{n}", "fp32" if dtype == FP32 else "bf16"]
                           + ([] if qkv_bias else ["nobias"]))


def _slab_case(dtype):
    """Block at the first of SLAB_SHAPES whose conv splits; fusable / rows are whatever that shape answers"""
    from ptv3_hip import ops
    from ptv3_hip.lib import lib
    found = [(c, n) for c, n in SLAB_SHAPES if lib.ptv3_gemm_splits(n, c, c, 27, ops._DT[dtype]) > 1]
    assert found, "no shape of SLAB_SHAPES splits its 27-tap conv over K any more"
    c, n = found[0]
    case = Case("block", c, n, dtype, slabs=True)
    case.id = "block-slab-" + ("fp32" if dtype == FP32 else "bf16")
    return case


CASES = [
    Case("block", 32, 777, FP32, fusable=1, slabs=True),
    Case("block", 32, 777, BF16, fusable=1, slabs=False),
    Case("block", 128, 333, FP32, fusable=2, slabs=True),
    Case("block", 128, 333, BF16, fusable=2, slabs=True),
    Case("block", 128, 16385, FP32, fusable=0, slabs=False, rows=True),
    Case("block", 128, 16385, BF16, fusable=0, slabs=False, rows=True),
    Case("block", 128, 24576 + 77, BF16, fusable=3, slabs=False),
    Case("block", 512, 245, FP32, fusable=0, slabs=True, rows=False),
    Case("plus", 64, 777, FP32, fusable=1, front=True),
    Case("plus", 64, 777, BF16, fusable=1, front=True),
    Case("plus", 128, 16385, FP32, fusable=0, rows=True, front=True),
    Case("plus", 512, 245, FP32, fusable=0, rows=False, front=False),
    Case("block", 32, 777, FP32, slabs=True, rows=False, qkv_bias=False),
]
IDS = [c.id for c in CASES] + ["block-slab-fp32", "block-slab-bf16"]

# {kernel name: launches} per case, recorded before the refactor (see the module docstring)
EXPECTED = {
    "block-c32-n777-fp32": {
        "gemm_kernel<32ch> gather (sparse conv)": 1, "block_head_kernel": 1, "block_tail_kernel": 1,
        "window_attn_full_kernel": 1},
    "block-c32-n777-bf16": {
        "gemm_kernel<32ch> gather (sparse conv)": 1, "block_head_kernel": 1, "block_tail_kernel": 1,
        "window_attn_full_kernel": 1},
    "block-c128-n333-fp32": {
        "gemm_kernel<64ch> gather (sparse conv)": 1, "block_head_coop_kernel": 1, "block_tail_coop_kernel": 1,
        "window_attn_full_kernel": 1},
    "block-c128-n333-bf16": {
        "block_head_coop_kernel": 1, "block_tail_coop_kernel": 1, "window_attn_full_kernel": 1,
        "conv_tile_kernel (sparse conv)": 1},
    "block-c128-n16385-fp32": {
        "gemm_kernel<64ch> dense": 1, "gemm_kernel<64ch> gather (sparse conv)": 1, "window_attn_full_kernel": 1,
        "rows_linear_kernel": 3},
    "block-c128-n16385-bf16": {
        "gemm_kernel<64ch> dense": 1, "gemm_kernel<64ch> gather (sparse conv)": 1, "window_attn_full_kernel": 1,
        "rows_linear_kernel": 3},
    "block-c128-n24653-bf16": {
        "gemm_kernel<64ch> gather (sparse conv)": 1, "window_attn_full_kernel": 1, "block_head_wide_kernel": 1,
        "block_tail_wide_kernel": 1},
    "block-c512-n245-fp32": {
        "gemm_kernel<64ch> dense": 4, "gemm_kernel<64ch> gather (sparse conv)": 1, "window_attn_full_kernel": 1},
    "plus-c64-n777-fp32": {
        "gemm_kernel<64ch> dense": 1, "gemm_kernel<32ch> gather (sparse conv)": 1, "block_head_kernel": 1,
        "block_tail_kernel": 1, "window_attn_full_kernel": 1},
    "plus-c64-n777-bf16": {
        "gemm_kernel<64ch> dense": 1, "gemm_kernel<32ch> gather (sparse conv)": 1, "block_head_kernel": 1,
        "block_tail_kernel": 1, "window_attn_full_kernel": 1},
    "plus-c128-n16385-fp32": {
        "gemm_kernel<64ch> dense": 2, "gemm_kernel<32ch> gather (sparse conv)": 1, "window_attn_full_kernel": 1,
        "rows_linear_kernel": 3},
    "plus-c512-n245-fp32": {
        "gemm_kernel<64ch> dense": 6, "gemm_kernel<64ch> gather (sparse conv)": 1, "window_attn_full_kernel": 1},
    "block-slab-fp32": {
        "gemm_kernel<64ch> dense": 4, "gemm_kernel<64ch> gather (sparse conv)": 1, "window_attn_full_kernel": 1},
    "block-slab-bf16": {
        "gemm_kernel<64ch> dense": 2, "window_attn_full_kernel": 1, "conv_tile_kernel (sparse conv)": 1,
        "rows_linear_kernel": 2},
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


def _cloud(n, seed):
    """two scenes (2/5 and 3/5 of n rows), each of distinct voxels at about a third of the cells of its cube"""
    g = torch.Generator().manual_seed(seed)
    sizes = [n * 2 // 5, n - n * 2 // 5]
    coords = []
    for m in sizes:
        e = max(4, int(round((3 * m) ** (1 / 3))) + 1)
        cell = torch.randperm(e ** 3, generator=g)[:m]
        coords.append(torch.stack([cell // (e * e), cell // e % e, cell % e], 1))
    return torch.cat(coords).int(), torch.tensor(sizes).cumsum(0)


def _block(case, dev):
    from pointcept.models.point_transformer_v3.point_transformer_v3m1_base import Block
    from pointcept.models.keypoint_ptv3_plus import BlockPlus
    torch.manual_seed(case.c + case.n)
    kw = dict(channels=case.c, num_heads=case.c // 16, patch_size=48, qkv_bias=case.qkv_bias, order_index=0,
              cpe_indice_key="stage0", enable_flash=True, upcast_attention=False, upcast_softmax=False)
    block = BlockPlus(cpe_kernel_size=5, **kw) if case.kind == "plus" else Block(**kw)
    with torch.no_grad():
        for p in block.parameters():      # LayerNorm affines and biases away from their 1 / 0 defaults
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape))
    return block.to(dev).eval()


def _point(grid_coord, offset, feat):
    from pointcept.models.utils.structure import Point
    point = Point(feat=feat.clone(), grid_coord=grid_coord, offset=offset)
    point.serialization(order=("z", "z-trans"))
    point.sparsify()
    return point


def _check_branch(case, block):
    """the capability answers that select the case's branch"""
    from ptv3_hip import ops
    from ptv3_hip.lib import lib
    from pointcept.models import keypoint_ptv3_plus as plus
    c, n, dt = case.c, case.n, case.dtype
    hidden = block.mlp[0].fc1.out_features
    if case.fusable is not None:
        assert ops.block_fusable(c, hidden, dt, n) == case.fusable
    if case.rows is not None:
        assert all(ops.rows_linear_capable(c, co, dt, n) for co in (3 * c, c, hidden)) == case.rows
        assert n >= ops.rows_linear_rows()
    if case.slabs is not None:
        assert (lib.ptv3_gemm_splits(n, c, c, 27, ops._DT[dt]) > 1) == case.slabs
    if case.front is not None:
        mid = block.cpe[3].in_channels
        assert plus.use_fused_cpe(c, mid, 125, dt) == (case.front, False)
        assert ((c, mid) in plus.FUSED_FRONT_OFF) == (not case.front)


def run_case(case, dev, generic=True):
    """({kernel: launches} of the block's eval forward, its output, the output of its _forward_generic or None)"""
    from ptv3_hip import ops
    block = _block(case, dev)
    _check_branch(case, block)
    grid_coord, offset = (t.to(dev) for t in _cloud(case.n, seed=case.n))
    g = torch.Generator().manual_seed(case.c * 7 + case.n)
    feat = ops.cast(torch.randn(case.n, case.c, generator=g).to(dev), case.dtype)
    point = _point(grid_coord, offset, feat)
    if case.slabs is not None and case.kind == "block":
        spt = point.sparse_conv_feat
        slabs = ops.conv_slabs(spt.features, block.folded_cpe(case.dtype)[0], spt.neighbors(3, "stage0"), 27, spt.row_order)
        assert (slabs is not None) == case.slabs
        point = _point(grid_coord, offset, feat)      # a fresh Point: the table is built inside the profiled forward
    with torch.no_grad():
        ops.profile_enable(True)
        try:
            out = block(point).feat
            torch.cuda.synchronize()
            kernels = {k: v["launches"] for k, v in ops.profile_collect_kernels().items()}
            ops.profile_collect()          # resets the records
        finally:
            ops.profile_enable(False)
        ref = block._forward_generic(_point(grid_coord, offset, feat)).feat if generic else None
    return kernels, out, ref


def _gap(out, ref):
    """(max |out - ref|, its bound: FP32_TOL or 8 bf16 steps of max(1, |ref|max))"""
    ref = ref.float()
    return (out.float() - ref).abs().max().item(), _bound(out.dtype, ref)


@pytest.mark.parametrize("case_id", IDS)
def test_block_dispatch(dev, case_id):
    case = next((c for c in CASES if c.id == case_id), None) or _slab_case(FP32 if case_id.endswith("fp32") else BF16)
    kernels, out, ref = run_case(case, dev)
    err, bound = _gap(out, ref)
    print(f"{case.id}: {kernels}  max|fused - generic| = {err:.3e} (bound {bound:.3e})")
    assert tuple(out.shape) == (case.n, case.c) and out.dtype == case.dtype and bool(torch.isfinite(out).all())
    if case.qkv_bias:
        assert kernels == EXPECTED[case.id]
    else:
        assert kernels and not any(k.startswith("block_head") for k in kernels), kernels
    assert err <= bound, (case.id, err, bound)
