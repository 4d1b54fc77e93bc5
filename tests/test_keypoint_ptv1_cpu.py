"""CPU-side checks of KeypointPTv1: registered under the reference's names and module paths, the fork config's exact
state_dict, argument refusals of the two new C entries without a GPU, the golden fixture's farthest-point selections
re-derived in float64 with their margin, and the refusal of scenes too small for five stages."""
import ctypes
import os

import numpy as np
import pytest
import torch

MARGIN = 2e-6


def _fps64(xyz, count):
    """Farthest point sampling of one scene in float64 (first point, then the first maximum of the running minimum
    squared distance); returns the rows and the smallest relative gap between a winner and its runner-up."""
    x = np.asarray(xyz, dtype=np.float64)
    d = np.full(len(x), 1e10)
    rows, gap, old = [0], np.inf, 0
    for _ in range(1, count):
        d = np.minimum(d, ((x - x[old]) ** 2).sum(1))
        old = int(np.argmax(d))
        top2 = np.partition(d, -2)[-2:]
        gap = min(gap, (top2[1] - top2[0]) / top2[1])
        rows.append(old)
    return np.asarray(rows[:count]), gap


def test_keypoint_ptv1_names_registered_and_build():
    from pointcept.models import MODELS, build_model
    blocks = {"KeypointPTv1": [1, 2, 3, 5, 2], "KeypointPTv1-26": [1, 1, 1, 1, 1], "KeypointPTv1-38": [1, 2, 2, 2, 2],
              "KeypointPTv1-50": [1, 2, 3, 5, 2]}
    for name, depth in blocks.items():
        assert MODELS.get(name) is not None, name
        model = build_model(dict(type=name, in_channels=7, num_keypoints=6, hidden_dim=32))
        assert [len(getattr(model, f"enc{i + 1}")) for i in range(5)] == depth
    model = build_model(dict(type="KeypointPTv1", blocks=[2, 2, 2, 1, 1], in_channels=7, num_keypoints=6, hidden_dim=64))
    assert sum(p.numel() for p in model.parameters()) == 331528


def test_fork_config_builds_with_reference_state_dict(golden_dir):
    """configs/my_dataset/keypoint_ptv1.py through the registry: keys, shapes, dtypes and order of the reference class
    built from the same config (tests/golden/make_golden_keypoint_ptv1.py)."""
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_PTV1_CFG
    model = build_model(KEYPOINT_PTV1_CFG)
    got = [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]
    ref = open(os.path.join(golden_dir, "state_dict_keypoint_ptv1_fork.txt")).read().strip().split("\n")
    assert len(ref) == 409 and got == ref
    assert sum(p.numel() for p in model.parameters()) == 3295010


def test_reference_module_paths_import():
    from pointcept.models.point_transformer.point_transformer_seg import TransitionDown, Bottleneck, PointTransformerLayer
    from pointcept.models.point_transformer.utils import LayerNorm1d
    block = Bottleneck(32, 32, 8, nsample=8)
    assert isinstance(block.transformer, PointTransformerLayer) and Bottleneck.expansion == 1
    assert isinstance(block.transformer.linear_w[0], LayerNorm1d) and isinstance(LayerNorm1d(3), torch.nn.BatchNorm1d)
    assert TransitionDown(32, 64, 4, 16).linear.in_features == 35 and TransitionDown(7, 32, 1, 8).linear.in_features == 7


def test_farthest_point_sampling_refuses_cpu_tensors():
    import pointops
    with pytest.raises(RuntimeError, match="GPU tensor"):
        pointops.farthest_point_sampling(torch.zeros(8, 3), torch.tensor([8]), torch.tensor([2]))
    from pointops import _C
    with pytest.raises(RuntimeError, match="GPU tensor"):
        _C.farthest_point_sampling_cuda(1, 8, torch.zeros(8, 3), torch.tensor([8], dtype=torch.int32),
                                        torch.tensor([2], dtype=torch.int32), torch.zeros(8),
                                        torch.zeros(2, dtype=torch.int32))


def test_new_entries_refuse_bad_arguments_without_a_gpu():
    """Argument checks come before any pointer is touched or kernel launched: error code 1 and a message."""
    from ptv3_hip.lib import lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    va = lambda n, c, ns: lib.ptv3_vector_attn_fwd(p, p, p, p, p, n, c, ns, *([p] * 12), p, None)   # noqa: E731
    assert va(4, 12, 8) == 1 and b"c=12 unsupported" in lib.ptv3_last_error()
    assert va(4, 520, 8) == 1 and b"c=520 unsupported" in lib.ptv3_last_error()
    assert va(4, 64, 33) == 1 and b"ns=33 unsupported" in lib.ptv3_last_error()
    assert va(4, 64, 0) == 1 and b"ns=0 unsupported" in lib.ptv3_last_error()
    for b in (0, -3):
        assert lib.ptv3_farthest_point_sampling(b, 8, p, p, p, p, p, None) == 1
        assert f"b={b} scenes".encode() in lib.ptv3_last_error()
    assert lib.ptv3_farthest_point_sampling(1, 8, None, p, p, p, p, None) == 1
    assert b"NULL" in lib.ptv3_last_error()
    with pytest.raises(RuntimeError, match="c=12 unsupported"):
        lib.check(va(4, 12, 8), "ptv3_vector_attn_fwd")


def test_golden_selections_hold_the_margin_in_float64(golden_dir):
    """Every farthest-point selection stored in keypoint_ptv1_tiny.npz, recomputed in float64 from the stored
    coordinates stage by stage: the same rows, and every runner-up at least 2e-6 (relative) below its winner - eight
    times the worst fp32 rounding of a squared distance (3 products and 2 sums, each 2^-24: about 2.4e-7), so an fp32
    kernel cannot legitimately pick another row."""
    g = np.load(os.path.join(golden_dir, "keypoint_ptv1_tiny.npz"))
    coord, ends = g["in_coord"], g["in_offset"].tolist()
    gap, selections = np.inf, 0
    for stage in range(2, 6):
        rows, new_ends, got = g[f"tap_idx{stage}"], g[f"tap_o{stage}"].tolist(), []
        assert new_ends == list(np.cumsum([(e - s) // 4 for s, e in zip([0] + ends[:-1], ends)]))
        for s, e, ms, me in zip([0] + ends[:-1], ends, [0] + new_ends[:-1], new_ends):
            r, gp = _fps64(coord[s:e], me - ms)
            got.append(r + s)
            gap = min(gap, gp)
            selections += me - ms - 1
        assert np.array_equal(np.concatenate(got), rows), stage
        coord, ends = coord[rows], new_ends
    assert selections == 1576 and gap >= MARGIN, (selections, gap)
    sizes4 = np.diff(np.concatenate([[0], g["tap_o4"]]))
    assert sizes4.min() < 16      # stage 5's TransitionDown sees -1 neighbours


def test_scene_too_small_for_five_stages_raises():
    """A scene under 256 points has no stage-5 point (the reference divides by zero there): refused by name, before any
    device work."""
    import ptv3_scenes as S
    from pointcept.models import build_model
    model = build_model(dict(type="KeypointPTv1-26", in_channels=7, num_keypoints=6, hidden_dim=32))
    data = S.make_batch([300, 255], in_channels=4, extent=32, seed=0)
    for mode in (True, False):
        with pytest.raises(ValueError, match="scene 1 has 255 points"):
            model.train(mode)(dict(data))
    ok = S.make_batch([300, 256], in_channels=4, extent=32, seed=0)
    with pytest.raises(RuntimeError, match="GPU tensor|No HIP GPUs"):
        model.eval()(dict(ok))
