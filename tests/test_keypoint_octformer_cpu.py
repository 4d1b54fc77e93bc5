"""OctFormer-v1m1 / KeypointOctFormer / OffsetKeypointOctFormer without a GPU: the state_dict listings of the fork
configs, the registry, tests/octree_ref.py against a brute-force numpy octree, the torch composition of the attention
(and of the whole model, over an octree_ref octree) against the reference's outputs in
tests/golden/keypoint_octformer_tiny.npz, and the domain check."""
import os

import numpy as np
import pytest
import torch

import octree_ref
from make_golden_keypoint_octformer import seeded_state_dict, load_golden, TINY_KW, TAPS, TAP_STRIDE, ATTN_BLOCK

FP32_TOL = 2e-5     # fp32 sums in another order against fp32 sums: the taps are O(1), their float64 gaps about 5e-7


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_golden(golden_dir)


@pytest.mark.parametrize("cfg_name, listing", [
    ("KEYPOINT_OCTFORMER_CFG", "state_dict_keypoint_octformer_fork.txt"),
    ("OFFSET_KEYPOINT_OCTFORMER_CFG", "state_dict_offset_keypoint_octformer_fork.txt")])
def test_fork_state_dict_listing(golden_dir, cfg_name, listing):
    from pointcept.models import build_model
    from ptv3_hip import configs
    model = build_model(dict(getattr(configs, cfg_name)))
    want = [line.rstrip("\n") for line in open(os.path.join(golden_dir, listing))]
    have = [f"{k} {tuple(v.shape)} {v.dtype}" for k, v in model.state_dict().items()]
    assert have == want


def test_build_model_resolves_the_three_names():
    from pointcept.models import build_model
    kw = {k: v for k, v in TINY_KW.items() if k not in ("num_keypoints", "hidden_dim")}
    assert type(build_model(dict(type="OctFormer-v1m1", num_classes=5, **kw))).__name__ == "OctFormer"
    assert type(build_model(dict(type="KeypointOctFormer", **TINY_KW))).__name__ == "KeypointOctFormer"
    assert type(build_model(dict(type="OffsetKeypointOctFormer", **TINY_KW))).__name__ == "OffsetKeypointOctFormer"


def _brute(points, batch, depth):
    """dict-based octree: per depth the sorted (b, morton) list, parents, 27 neighbours and deconvolution pairs"""
    def morton(c, d):
        k = 0
        for i in range(d):
            k |= ((c[0] >> i) & 1) << (3 * i + 2) | ((c[1] >> i) & 1) << (3 * i + 1) | ((c[2] >> i) & 1) << (3 * i)
        return k
    cell = np.floor((points.astype(np.float32) + np.float32(1)) * np.float32(2 ** (depth - 1))).astype(np.int64)
    out = {}
    for d in range(1, depth + 1):
        nodes = sorted({(int(b), morton(tuple(c >> (depth - d)), d), tuple(int(v) for v in c >> (depth - d)))
                        for b, c in zip(batch, cell)})
        row = {(b, c): i for i, (b, _, c) in enumerate(nodes)}
        out[d] = dict(keys=[(b << 48) | m for b, m, _ in nodes], row=row, cells=[(b, c) for b, _, c in nodes])
    for d in range(1, depth + 1):
        cells_d, row = out[d]["cells"], out[d]["row"]
        out[d]["nbr"] = [[row.get((b, (c[0] + dx, c[1] + dy, c[2] + dz)), -1) for dx in (-1, 0, 1) for dy in (-1, 0, 1)
                          for dz in (-1, 0, 1)] for b, c in cells_d]
        if d > 1:
            out[d]["parent"] = [out[d - 1]["row"][(b, (c[0] >> 1, c[1] >> 1, c[2] >> 1))] for b, c in cells_d]
        if d < depth:
            fine = out[d + 1]["row"]
            pairs = set()
            for p, (b, c) in enumerate(cells_d):
                for t, o in enumerate((a, e, f) for a in (-1, 0, 1) for e in (-1, 0, 1) for f in (-1, 0, 1)):
                    f_row = fine.get((b, (2 * c[0] + o[0], 2 * c[1] + o[1], 2 * c[2] + o[2])), -1)
                    if f_row >= 0:
                        pairs.add((p, t, f_row))
            out[d]["pairs"] = pairs
    return out


def test_octree_ref_against_brute_force():
    rs = np.random.RandomState(3)
    pts = np.clip(rs.randn(200, 3) * 0.3, -0.999, 0.999).astype(np.float32)
    batch = np.sort(rs.randint(0, 2, 200))
    depth = 5
    oct = octree_ref.Octree(depth, 2, batch_size=2)
    oct.build_octree(octree_ref.Points(torch.from_numpy(pts), features=torch.zeros(200, 1),
                                       batch_id=torch.from_numpy(batch).view(-1, 1), batch_size=2))
    oct.construct_all_neigh()
    ref = _brute(pts, batch, depth)
    for d in range(1, depth + 1):
        assert oct.keys[d].tolist() == ref[d]["keys"], d
        assert oct.neighs[d].tolist() == ref[d]["nbr"], d
        if d > 1:
            assert oct.parent[d].tolist() == ref[d]["parent"], d
        if d < depth:
            assert {tuple(r) for r in oct.deconv_pairs(d).tolist()} == ref[d]["pairs"], d
            # the package's gather table lists the same pairs from the fine side
            lv = octree_ref.Levels(oct, 1)
            tab = lv.deconv_table(d)
            rows, taps = torch.nonzero(tab >= 0, as_tuple=True)
            assert {(int(tab[r, t]), int(t), int(r)) for r, t in zip(rows, taps)} == ref[d]["pairs"], d
            assert int((tab >= 0).sum(1).max()) <= 8


def _tiny_on_cpu(golden, kind="KeypointOctFormer"):
    from pointcept.models import build_model
    model = build_model(dict(type=kind, **TINY_KW))
    model.load_state_dict(seeded_state_dict(model.state_dict()), strict=True)
    coord, feat, offset = (torch.from_numpy(golden["in_" + k]) for k in ("coord", "feat", "offset"))
    batch = torch.searchsorted(offset, torch.arange(len(coord)), right=True)
    oct = octree_ref.Octree(TINY_KW["octree_depth"], 2, batch_size=len(offset))
    oct.build_octree(octree_ref.Points(coord / TINY_KW["octree_scale_factor"], features=feat,
                                       batch_id=batch.view(-1, 1), batch_size=len(offset)))
    oct.construct_all_neigh()
    levels = octree_ref.Levels(oct, TINY_KW["octree_depth"] - TINY_KW["stem_down"] - 3)
    data = {"coord": coord, "feat": feat, "offset": offset, "octree": levels}
    return model.eval(), data, levels


def test_composed_attention_equals_the_reference(golden):
    """OctreeAttention (dilation 4, finest stage) of the package, composed in torch, on the stored input"""
    model, data, levels = _tiny_on_cpu(golden)
    depth = int(golden["attn_depth"])
    assert golden["keys%d" % depth].tolist() == levels.keys[depth].tolist()
    attn = dict(model.named_modules())[ATTN_BLOCK]
    assert attn.dilation == 4
    from pointcept.models.octformer.octformer_v1m1_base import OctreeT
    tree = OctreeT(levels, TINY_KW["patch_size"], TINY_KW["dilation"], True, max_depth=depth, start_depth=depth - 3)
    with torch.no_grad():
        out = attn(torch.from_numpy(golden["attn_in"]), tree, depth)
    err = (out - torch.from_numpy(golden["attn_out"])).abs().max().item()
    print("composed attention against the reference", err)
    assert err < FP32_TOL * max(1.0, float(np.abs(golden["attn_out"]).max()))


def test_composed_model_equals_the_reference(golden):
    """the whole torch composition over an octree_ref octree: taps and pred of KeypointOctFormer, pred and loss of
    OffsetKeypointOctFormer"""
    model, data, _ = _tiny_on_cpu(golden)
    taps = {}
    with torch.no_grad():
        feats = model.backbone(data, taps)
    for name in TAPS:
        ref = golden["tap_" + name]
        err = np.abs(taps[name].numpy()[::TAP_STRIDE[name]] - ref).max() / max(1.0, np.abs(ref).max())
        print(name, err)
        assert err < FP32_TOL, name
    head = model.reg_head      # its eval path is one GPU kernel: restated here
    g = torch.zeros(3, feats.shape[1]).index_add_(0, torch.searchsorted(data["offset"], torch.arange(len(feats)),
                                                                         right=True), feats)
    g = g / torch.tensor([1500.0, 40.0, 2600.0]).view(-1, 1)
    bn = head[1]
    h = torch.relu((g @ head[0].weight.t() + head[0].bias - bn.running_mean) / torch.sqrt(bn.running_var + bn.eps)
                   * bn.weight + bn.bias)
    h = torch.relu(h @ head[4].weight.t() + head[4].bias)
    pred = (h @ head[6].weight.t() + head[6].bias).view(-1, 6, 3)
    assert (pred.detach() - torch.from_numpy(golden["eval_pred"])).abs().max().item() < FP32_TOL

    model, data, _ = _tiny_on_cpu(golden, "OffsetKeypointOctFormer")
    data["target"] = torch.from_numpy(golden["offset_target"])
    with torch.no_grad():
        out = model(data)
    assert np.abs(out["pred"].numpy()[::16] - golden["offset_pred"]).max() < FP32_TOL
    assert abs(out["loss"].item() - float(golden["offset_loss"])) < FP32_TOL


def test_point_outside_the_domain_raises():
    from pointcept.models.octformer.octformer_v1m1_base import octree_cells
    good = torch.tensor([[0.0, -10.24, 10.2399]])
    assert octree_cells(good, 10.24, 11).tolist() == [[1024, 0, 2047]]
    for bad in (10.24, -10.2401, 11.0, float("nan")):
        with pytest.raises(ValueError):
            octree_cells(torch.tensor([[0.0, bad, 0.0]]), 10.24, 11)
        with pytest.raises(ValueError):
            octree_ref.cells(torch.tensor([[0.0, bad / 10.24, 0.0]]), 11)
