"""GPU: the hidden-sliced block tail for few rows (block_tail_sliced_kernel + tail_sliced_finish_kernel in
csrc/block_wide.hip), called through ops.block_tail_sliced, bf16 at C = 256 and C = 128.

With one group the kernel is block_tail_wide_kernel's arithmetic to the last rounding: bitwise its result.  With G > 1
groups the only new rounding is an fp32 reassociation of the fc2 sum (G partials summed in group order before the one
bf16 rounding), so every case is held to the bounds tests/test_hip_size_variants.py holds block_tail_wide_kernel to:
8 bf16 steps of max(1, |ref|) against the float64 tail_ref, 4 against the unfused launches.  `out` is pre-filled
with NaN in every case, so a skipped store shows."""
import json
import os
import subprocess
import sys

import pytest
import torch

from test_hip_size_variants import _Block, _bound, _err, _kernels, _randn

pytestmark = pytest.mark.gpu

C = 256
WIDTHS = (256, 128)
DT = torch.bfloat16
GROUPS = {256: (1, 2, 4, 8, 16), 128: (1, 2, 4, 8)}      # the divisors of hidden / 64
KERNEL = "block_tail_sliced_kernel"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def blocks():
    return {c: _Block(c, seed=31 + c) for c in WIDTHS}


@pytest.fixture(scope="module")
def tails(blocks, dev):
    return {c: b.dev_args(dev, DT, False)[1] for c, b in blocks.items()}


@pytest.fixture(scope="module")
def blk(blocks):
    return blocks[C]


@pytest.fixture(scope="module")
def tail(tails):
    return tails[C]


def _inputs(m, dev, seed=None, c=C):
    gen = torch.Generator(device=dev).manual_seed(4000 + c + (m if seed is None else seed))
    return _randn(m, c, DT, gen, dev), _randn(m, c, DT, gen, dev)


def _sliced(attn, f1, tail, groups, workspace=None):
    from ptv3_hip import ops
    out = torch.full_like(attn, float("nan"))
    return ops.block_tail_sliced(attn, f1, *tail, groups=groups, out=out, workspace=workspace)


def _check(tag, got, ref64, unfused):
    """both bounds of the module docstring; returns the two maxima"""
    assert torch.isfinite(got.float()).all(), (tag, "a row was not stored")
    e = _err(got, ref64)
    assert e < _bound(DT, ref64), (tag, "vs float64", e, _bound(DT, ref64))
    u = (got.float() - unfused).abs().max().item()
    assert u <= _bound(DT, unfused, steps=4), (tag, "vs unfused", u, _bound(DT, unfused, steps=4))
    return e, u


@pytest.mark.parametrize("c", WIDTHS)
def test_one_group_is_bitwise_the_wide_kernel(dev, tails, c):
    """m = 24 576 + 77: ops.block_tail runs block_tail_wide_kernel there (two 16-row tiles per wave, a partial last
    workgroup); the sliced kernel with one group (one tile per wave: a row's arithmetic does not depend on its tile)
    writes the same bytes."""
    from ptv3_hip import ops
    m = 24576 + 77
    tail = tails[c]
    attn, f1 = _inputs(m, dev, c=c)
    want, names = _kernels(lambda: ops.block_tail(attn, f1, *tail))
    assert names == {"block_tail_wide_kernel"}, names
    got, names = _kernels(lambda: _sliced(attn, f1, tail, 1))
    assert names == {KERNEL}, names
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, want)


@pytest.mark.parametrize("c", WIDTHS)
@pytest.mark.parametrize("m", [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 245, 1388, 5590])
def test_row_counts_and_groups(dev, blocks, tails, m, c):
    """a single row, partial 16-row tiles, a wave with no valid row, a partial last workgroup (64 rows per workgroup),
    and row counts of the deep levels of the 100k-point scene; every group count"""
    blk, tail = blocks[c], tails[c]
    attn, f1 = _inputs(m, dev, c=c)
    ref = blk.tail_ref(attn.double().cpu(), f1.double().cpu(), DT)
    unfused = blk.unfused_tail(attn, f1, dev, DT).float()
    for groups in GROUPS[c]:
        got, names = _kernels(lambda: _sliced(attn, f1, tail, groups))
        assert names == {KERNEL}, names
        e, u = _check((c, m, groups), got, ref, unfused)
        print(f"sliced c={c} m={m} G={groups}: vs float64 {e:.3e} (bound {_bound(DT, ref):.3e}), vs unfused {u:.3e} "
              f"(bound {_bound(DT, unfused, steps=4):.3e})")


@pytest.mark.parametrize("c,big", [(256, 0), (256, 5), (256, 15), (128, 0), (128, 3), (128, 7)])
def test_one_large_hidden_slice(dev, c, big):
    """|bias1| about 8 on one 64-wide slice of the hidden layer and about 0 elsewhere: a group that multiplies the
    wrong w2 columns, or adds another slice's bias1, misses the bounds by far"""
    blk = _Block(c, seed=32)
    gen = torch.Generator().manual_seed(big)
    blk.bias1 = 0.01 * torch.randn(4 * c, generator=gen)
    blk.bias1[64 * big:64 * big + 64] = 8.0 * (1.0 + 0.1 * torch.randn(64, generator=gen))
    tail = blk.dev_args(dev, DT, False)[1]
    m = 129
    attn, f1 = _inputs(m, dev, seed=big, c=c)
    ref = blk.tail_ref(attn.double().cpu(), f1.double().cpu(), DT)
    unfused = blk.unfused_tail(attn, f1, dev, DT).float()
    for groups in GROUPS[c]:
        e, u = _check((c, big, groups), _sliced(attn, f1, tail, groups), ref, unfused)
        print(f"sliced c={c} large slice {big} G={groups}: vs float64 {e:.3e}, vs unfused {u:.3e}, |ref| {ref.abs().max():.2f}")


def test_repeated_calls_are_bitwise_equal(dev, tail):
    """the partials are summed in group order by a second launch: no dependence on the order the groups finish in"""
    m = 1388
    attn, f1 = _inputs(m, dev)
    first = _sliced(attn, f1, tail, 8)
    for _ in range(2):
        assert torch.equal(_sliced(attn, f1, tail, 8), first)


def test_refusals_launch_nothing(dev, blk, tail):
    from ptv3_hip import ops
    m = 65
    attn, f1 = _inputs(m, dev)
    nan = lambda t: torch.full_like(t, float("nan"))  # noqa: E731

    def refused(what, fn, out):
        with pytest.raises(RuntimeError, match=what):
            fn()
        torch.cuda.synchronize()
        assert torch.isnan(out.float()).all(), what

    need = ops.lib.ptv3_block_tail_sliced_workspace_bytes(m, C, 8)
    assert need == 8 * m * C * 4
    out = nan(attn)
    small = torch.empty(need - 1, dtype=torch.uint8, device=dev)
    refused("workspace", lambda: ops.block_tail_sliced(attn, f1, *tail, groups=8, out=out, workspace=small), out)
    for groups in (3, 5, 32):
        refused("must divide", lambda: ops.block_tail_sliced(attn, f1, *tail, groups=groups, out=out), out)
    # fp32
    tail32 = blk.dev_args(dev, torch.float32, False)[1]
    a32, f32 = attn.float(), f1.float()
    out32 = nan(a32)
    refused("bf16 only", lambda: ops.block_tail_sliced(a32, f32, *tail32, groups=4, out=out32), out32)
    # a width outside the served set
    b64 = _Block(64, seed=33)
    tail64 = b64.dev_args(dev, DT, False)[1]
    a64 = attn[:, :64].contiguous()
    out64 = nan(a64)
    refused("not served", lambda: ops.block_tail_sliced(a64, a64, *tail64, groups=4, out=out64), out64)
    # no rows: fine, and nothing to write
    empty = attn[:0]
    assert ops.block_tail_sliced(empty, empty, *tail, groups=8).shape == (0, C)


# ---- the executor ------------------------------------------------------------------------------------------------
_CHILD = r"""
import json, sys
root, pkg, points, pred_path = sys.argv[1], sys.argv[2], int(sys.argv[3]), sys.argv[4]
sys.path[:0] = [root, pkg]
import torch
from pointcept.models import build_model
from ptv3_hip import ops
from ptv3_hip.configs import FORK_CFG
import ptv3_scenes as S
torch.manual_seed(0)
model = build_model(dict(type="OffsetKeypointPTv3", num_keypoints=6, backbone_conf=dict(type="PT-v3m1", **FORK_CFG))).eval()
data = S.make_batch([points], in_channels=4, extent=None, seed=21, with_target=6)
model = model.to("cuda:0")
model.backbone.compute_dtype = torch.bfloat16
datad = {k: v.to("cuda:0") for k, v in data.items()}
ops.profile_enable(True)
with torch.no_grad():
    torch.manual_seed(3)
    levels = model.backbone(datad, _head=model.head)["_stage_points"]
    torch.cuda.synchronize()
    ops.profile_collect_kernels(); ops.profile_collect()
    torch.manual_seed(3)
    pred = model(datad)["pred"].float().cpu()
torch.cuda.synchronize()
kernels = ops.profile_collect_kernels()
ops.profile_enable(False)
torch.save(pred, pred_path)
print("RESULT " + json.dumps(dict(levels=list(levels), launches={k: v["launches"] for k, v in kernels.items()})))
"""

POINTS = 30000


def _child(mode, pred_path):
    env = dict(os.environ)
    env.pop("PTV3_TAIL_SLICED_GROUPS", None)
    if mode is None:
        env.pop("PTV3_TAIL_SLICED", None)
    else:
        env["PTV3_TAIL_SLICED"] = mode
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd"),
                        str(POINTS), pred_path], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):]), torch.load(pred_path)


def test_forward_through_the_executor(tmp_path):
    """The fork config in bf16 at 30 000 points (the 6 000 of test_forward_through_the_executor_levels_0_and_1 scaled
    until the C = 256 level lies inside the policy's row range): PTV3_TAIL_SLICED=0 against the default and against
    PTV3_TAIL_SLICED=2, each in a process of its own.  Every prediction is held to the bf16 bound of
    test_fork_config_at_bench_scene_vs_oracle against the oracle; by default the C = 256 blocks run the sliced tail
    and no rows_linear_kernel, forced the C = 128 blocks (1 359 rows here, the cooperative tail's by policy) run it too."""
    from oracle import ptv3 as O
    from pointcept.models import build_model
    from ptv3_hip import ops
    from ptv3_hip.configs import FORK_CFG
    import ptv3_scenes as S
    torch.manual_seed(0)
    model = build_model(dict(type="OffsetKeypointPTv3", num_keypoints=6,
                             backbone_conf=dict(type="PT-v3m1", **FORK_CFG))).eval()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    data = S.make_batch([POINTS], in_channels=4, extent=None, seed=21, with_target=6)
    torch.manual_seed(3)
    with torch.no_grad():
        ref = O.OffsetKeypointOracle(FORK_CFG, sd).forward(data)
    off, pred_off = _child("0", str(tmp_path / "off.pt"))
    on, pred_on = _child(None, str(tmp_path / "on.pt"))
    forced, pred_forced = _child("2", str(tmp_path / "forced.pt"))
    levels = on["levels"]
    assert levels == off["levels"] == forced["levels"]
    blocks, blocks128 = 0, 0
    for st, n in enumerate(levels):
        for c, count in ((FORK_CFG["enc_channels"][st], FORK_CFG["enc_depths"][st]),
                         (FORK_CFG["dec_channels"][st], FORK_CFG["dec_depths"][st]) if st < len(FORK_CFG["dec_channels"]) else (0, 0)):
            if c == C and ops.block_tail_sliced_policy(c, 4 * c, DT, n):
                blocks += count
            if c == 128:
                assert not ops.block_tail_sliced_policy(c, 4 * c, DT, n), (n, "the scene grew into the C = 128 policy")
                blocks128 += count
    assert blocks == 8, (blocks, levels)                      # encoder 3 six blocks, decoder 3 two
    assert blocks128 == 4, (blocks128, levels)                # encoder 2 two blocks, decoder 2 two
    assert off["launches"].get(KERNEL, 0) == 0, off["launches"]
    assert on["launches"].get(KERNEL, 0) == blocks, on["launches"]
    assert forced["launches"].get(KERNEL, 0) == blocks + blocks128, forced["launches"]
    assert off["launches"].get("block_tail_coop_kernel", 0) - forced["launches"].get("block_tail_coop_kernel", 0) == blocks128
    # the two rows_linear launches of each of those tails (proj, fc1) are gone; the profiler has one name for every
    # width, and the C = 512 level keeps its own
    rows_off, rows_on = off["launches"].get("rows_linear_kernel", 0), on["launches"].get("rows_linear_kernel", 0)
    assert rows_off - rows_on == 2 * blocks, (rows_off, rows_on)
    scale = max(1.0, ref["logits"].abs().max().item())
    for tag, pred in (("PTV3_TAIL_SLICED=0", pred_off), ("default", pred_on), ("PTV3_TAIL_SLICED=2", pred_forced)):
        assert torch.isfinite(pred).all()
        err = (pred - ref["pred"]).abs()
        print(f"{tag}: max err {err.max().item():.3e}, mean {err.mean().item():.3e} (scale {scale:.3f}), levels {levels}")
        assert err.max().item() < 64 * 2.0 ** -8 * scale, (tag, err.max().item(), scale)
        assert err.mean().item() < 8 * 2.0 ** -8 * scale, (tag, err.mean().item(), scale)
