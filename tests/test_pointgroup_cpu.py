"""PointGroup without a GPU: the numpy restatements of tests/pointgroup_ref.py against the reference's fixture
(tests/golden/pointgroup_tiny.npz; its clustering is that restatement, pointgroup_ops parity UNPINNED), the registry and
state_dict listings, InstanceParser against the reference's output, and the host breadth-first search through the C ABI
(it touches no GPU) against the restatement, plus a stand-alone sanitizer build of it."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import pointgroup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pointcept-keypointdetection_amd")
IGNORE = (-1, 0, 1)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "pointgroup_tiny.npz"))


def _sd(g):
    return {k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd_")}


def test_ref_reproduces_fixture_proposals(fixture):
    """The heads in float64 torch on the fixture's weights, then the restated tail: clusters and proposals exact (the
    fixture's seed keeps every pair 1e-4 away from the threshold and every top-two logit gap above 1e-3), scores to
    float64 rounding of the reference's fp32 means (2 m 2^-24, m the largest proposal)."""
    g = fixture
    sd = {k: v.double() for k, v in _sd(g).items()}
    feat = torch.from_numpy(g["in_feat"]).double() @ sd["backbone.lin.weight"].T + sd["backbone.lin.bias"]
    h = feat @ sd["bias_head.0.weight"].T + sd["bias_head.0.bias"]
    h = (h - sd["bias_head.1.running_mean"]) / torch.sqrt(sd["bias_head.1.running_var"] + 1e-3)
    h = torch.relu(h * sd["bias_head.1.weight"] + sd["bias_head.1.bias"])
    bias = h @ sd["bias_head.3.weight"].T + sd["bias_head.3.bias"]
    logit = feat @ sd["seg_head.weight"].T + sd["seg_head.bias"]
    center = ((torch.from_numpy(g["in_coord"]).double() + bias) / 0.02).float().numpy()
    prob = torch.softmax(logit, 1).numpy()
    seg = prob.argmax(1)
    keep = ~np.isin(seg, IGNORE)
    rows = np.nonzero(keep)[0]
    ends = np.searchsorted(rows, g["in_offset"])
    offsets = np.concatenate([[0], ends]).astype(np.int32)
    idxs, offs = R.cluster(center[rows], seg[rows].astype(np.int32), offsets, 1.5, 50)
    idxs = R.sort_members(idxs, offs)
    idxs[:, 1] = rows[idxs[:, 1]]
    assert np.array_equal(offs, g["proposals_offset"]) and np.array_equal(idxs, g["proposals_idx"])
    classes, scores, members = R.proposals(idxs, offs, prob, seg, 100)
    assert np.array_equal(classes, g["pred_classes"])
    assert np.array_equal(np.concatenate(members), g["pred_mask_rows"])
    assert np.array_equal(np.concatenate([[0], np.cumsum([len(m) for m in members])]), g["pred_mask_offset"])
    m = max(len(x) for x in members)
    assert np.abs(scores - g["pred_scores"].astype(np.float64)).max() <= 2 * m * 2.0 ** -24


def test_registry_and_state_dict_listings(golden_dir):
    from pointcept.models import MODELS, build_model
    from ptv3_hip.configs import PG_PTV3_SCANNET_CFG, PG_SPUNET_SCANNET_CFG
    assert MODELS.get("PG-v1m1") is not None and MODELS.get("PG-v1m2") is not None
    for cfg, fname in ((PG_PTV3_SCANNET_CFG, "state_dict_pointgroup_v1m2_ptv3_scannet.txt"),
                       (PG_SPUNET_SCANNET_CFG, "state_dict_pointgroup_v1m1_spunet_scannet.txt")):
        model = build_model(cfg)
        ref = open(os.path.join(golden_dir, fname)).read().strip().split("\n")
        assert [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()] == ref
    frozen = build_model(dict(PG_PTV3_SCANNET_CFG, freeze_backbone=True))
    assert not any(p.requires_grad for p in frozen.backbone.parameters())
    assert all(p.requires_grad for p in frozen.bias_head.parameters())


def test_instance_parser_equals_reference(fixture):
    from pointcept.datasets import InstanceParser, TRANSFORMS
    g = fixture
    assert TRANSFORMS.get("InstanceParser") is InstanceParser
    out = InstanceParser(segment_ignore_index=IGNORE, instance_ignore_index=-1)(
        dict(coord=g["ip_coord"].copy(), segment=g["ip_segment"].copy(), instance=g["ip_instance"].copy()))
    assert np.array_equal(out["instance"], g["ip_out_instance"])
    for got, want in ((out["instance_centroid"], g["ip_out_centroid"]), (out["bbox"], g["ip_out_bbox"])):
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def _directed_case():
    """0 -> 1 -> 2 and 3 -> 2: undirected, {0, 1, 2, 3} is one component; directed, 3 is found after 2 was taken"""
    label = np.array([7, 7, 7, 7, 9], dtype=np.int32)
    lists = [[0, 1], [1, 2], [2], [3, 2], [4, 0]]
    return label, lists


def _random_graph(n=3000, seed=3):
    g = np.random.default_rng(seed)
    label = g.integers(0, 3, size=n).astype(np.int32)
    return label, [[i] + g.integers(0, n, size=g.integers(0, 4)).tolist() for i in range(n)]


@pytest.mark.parametrize("case", ["directed", "random"])
@pytest.mark.parametrize("threshold", [1, 3])
def test_host_bfs_equals_ref_discovery_order(case, threshold):
    from ptv3_hip import ops
    label, lists = _directed_case() if case == "directed" else _random_graph()
    idx = np.concatenate([np.asarray(l, dtype=np.int32) for l in lists])
    lens = np.array([len(l) for l in lists], dtype=np.int32)
    start_len = np.stack([np.cumsum(lens) - lens, lens], 1).astype(np.int32)
    want_idxs, want_offs = R.bfs_cluster(label, idx, start_len, threshold)
    if case == "directed" and threshold == 1:
        assert want_offs.tolist() == [0, 3, 4, 5] and want_idxs[:, 1].tolist() == [0, 1, 2, 3, 4]
    got_idxs, got_offs = ops.pg_bfs_cluster_host(torch.from_numpy(label), torch.from_numpy(idx),
                                                 torch.from_numpy(start_len), threshold)
    assert np.array_equal(got_offs.numpy(), want_offs) and np.array_equal(got_idxs.numpy(), want_idxs)
    import pointgroup_ops
    s_idxs, s_offs = pointgroup_ops.bfs_cluster(torch.from_numpy(label), torch.from_numpy(idx),
                                                torch.from_numpy(start_len), threshold)
    assert np.array_equal(s_offs.numpy(), want_offs) and np.array_equal(s_idxs.numpy(), R.sort_members(want_idxs, want_offs))


def test_host_bfs_refuses_entries_outside_the_arrays():
    from ptv3_hip import ops
    with pytest.raises(RuntimeError):
        ops.pg_bfs_cluster_host(torch.zeros(1, dtype=torch.int32), torch.tensor([5], dtype=torch.int32),
                                torch.tensor([[0, 1]], dtype=torch.int32), 1)


def test_host_bfs_standalone_under_sanitizers(tmp_path):
    """tests/pg_bfs_host_main.cpp + csrc/pg_bfs_host.cpp alone, -fsanitize=address,undefined, run as a plain child."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pg_bfs_host_main")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "pg_bfs_host_main.cpp"),
                            os.path.join(PKG, "csrc", "pg_bfs_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "pg_bfs_host ok" in run.stdout, run.stdout + run.stderr
