"""Build-container-only: run the reference's PG-v1m1 and PG-v1m2 (pointcept/models/point_group/, imported in place through
ref_loader's stubs) on a seeded three-scene batch of Gaussian blobs and store, in pointgroup_tiny.npz, the inputs, the
state_dict, the clusters and proposals of an eval forward, one training step of each class (the four losses, every
parameter gradient, the updated BatchNorm statistics), and the reference InstanceParser's output on a 300-point sample.

The backbone is a stand-in registered in the reference's registry - nn.Linear(6, 64) on data_dict["feat"] - so the file
pins the wrapper, not a backbone.  `pointgroup_ops` is the CUDA library of libs/pointgroup_ops, which cannot be built
here: it is stubbed by the brute-force restatement of tests/pointgroup_ref.py, so PARITY WITH pointgroup_ops IS UNPINNED;
what the file pins is everything the reference's Python does around it.

The seed is the first one for which (a) no same-scene pair of kept `center_pred` rows lies within a relative 1e-4 of
cluster_thresh in float64, so the neighbour sets are the same under any fp32 evaluation order or FMA contraction, (b) no
connected component has min_points - 1, min_points, propose_points or propose_points + 1 members, (c) every point's
top-two logit gap exceeds 1e-3, (d) every scene yields at least two proposals.  Gradients are stored as
make_golden_keypoint_regression.py stores them (float16 of grad / max|grad| plus that fp32 maximum).  PG-v1m2 runs with
criteria = CrossEntropyLoss(loss_weight=0.7) alone: the library's LovaszLoss deliberately departs from the reference's
fp32 differences at a few thousand rows (include/ptv3_hip.h) and is pinned by its own fixture.

Not stored: the branch with no point kept.  The reference indexes a 1-d tensor with two indices there
(point_group_v1m1_base.py:120, :149) and raises.

Also lists the state_dict of both classes built from configs/scannet/insseg-pointgroup-v1m2-0-ptv3-base.py and
configs/scannet/insseg-pointgroup-v1m1-0-spunet-base.py.
usage: python tests/golden/make_golden_pointgroup.py"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "pointcept-keypointdetection_amd"))
import ref_loader  # noqa: E402
import pointgroup_ref as R  # noqa: E402
from make_golden_swin3d import _cfg  # noqa: E402
from make_golden_keypoint_regression import perturb_bn, write_listing  # noqa: E402

BLOBS = [[400, 300, 250, 150, 120, 80, 70, 60, 40, 30], [250, 180, 120, 80, 40, 30],
         [500, 400, 300, 250, 200, 130, 90, 70, 40, 20]]
THRESH, MIN_POINTS, PROPOSE, VOXEL, MARGIN = 1.5, 50, 100, 0.02, 1e-4
IGNORE = (-1, 0, 1)
CAPTURED = {}


def _install_pointgroup_ops_stub():
    m = types.ModuleType("pointgroup_ops")

    def ballquery_batch_p(coords, batch_idxs, batch_offsets, radius, mean_active):
        idx, start_len = R.ball_query(coords.detach().numpy(), batch_idxs.numpy(), batch_offsets.numpy(), radius)
        CAPTURED["max_count"] = int(R.neighbour_counts(coords.detach().numpy(), batch_idxs.numpy(), batch_offsets.numpy(),
                                                       radius).max())
        return torch.from_numpy(idx), torch.from_numpy(start_len)

    def bfs_cluster(semantic_label, ball_query_idxs, start_len, threshold):
        label, idx, sl = semantic_label.numpy(), ball_query_idxs.numpy(), start_len.numpy()
        CAPTURED["all_sizes"] = np.diff(R.bfs_cluster(label, idx, sl, 1)[1])
        idxs, offs = R.bfs_cluster(label, idx, sl, threshold)
        CAPTURED["clusters"] = (idxs.copy(), offs.copy())
        return torch.from_numpy(idxs.copy()), torch.from_numpy(offs.copy())

    m.ballquery_batch_p, m.bfs_cluster = ballquery_batch_p, bfs_cluster
    sys.modules["pointgroup_ops"] = m


def make_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    coord, feat, segment, instance, centroid, sizes = [], [], [], [], [], []
    for blobs in BLOBS:
        while True:                            # blob centres at least 5 radii apart, blobs well inside one radius
            centres = torch.rand(len(blobs), 3, generator=g) * 0.8 + 0.1
            if (torch.cdist(centres, centres) + torch.eye(len(blobs))).min().item() > 0.15:
                break
        pts, codes, seg, ins = [], [], [], []
        for k, m in enumerate(blobs):
            pts.append(centres[k] + 0.003 * torch.randn(m, 3, generator=g))
            code = torch.randn(6, generator=g) * 3.0
            codes.append(code + 0.03 * torch.randn(m, 6, generator=g))
            cls = int(torch.randint(0, 20, (1,), generator=g)) if k % 5 != 4 else -1
            seg.append(torch.full((m,), cls, dtype=torch.int64))
            ins.append(torch.full((m,), k if cls not in IGNORE else -1, dtype=torch.int64))
        perm = torch.randperm(sum(blobs), generator=g)
        pts, ins = torch.cat(pts)[perm], torch.cat(ins)[perm]
        cen = torch.full((pts.shape[0], 3), -1.0)
        for k in range(len(blobs)):
            if (ins == k).any():
                cen[ins == k] = pts[ins == k].mean(0)
        coord.append(pts), feat.append(torch.cat(codes)[perm]), segment.append(torch.cat(seg)[perm])
        instance.append(ins), centroid.append(cen), sizes.append(pts.shape[0])
    return dict(coord=torch.cat(coord), feat=torch.cat(feat), segment=torch.cat(segment), instance=torch.cat(instance),
                instance_centroid=torch.cat(centroid), offset=torch.tensor(np.cumsum(sizes), dtype=torch.int64))


def build(cls, seed, **extra):
    torch.manual_seed(1234 + seed)
    model = cls(backbone=dict(type="PGStandInBackbone"), backbone_out_channels=64, semantic_num_classes=20,
                semantic_ignore_index=-1, segment_ignore_index=IGNORE, instance_ignore_index=-1, cluster_thresh=THRESH,
                cluster_closed_points=300, cluster_propose_points=PROPOSE, cluster_min_points=MIN_POINTS,
                voxel_size=VOXEL, **extra)
    with torch.no_grad():                      # predicted shifts well below the blob width
        model.bias_head[3].weight.mul_(2e-3)
        model.bias_head[3].bias.mul_(2e-3)
    perturb_bn(model)
    return model


def clean(model, data):
    """conditions (a) and (c) on the model's own fp32 predictions; returns None or the kept-row mask"""
    with torch.no_grad():
        feat = model.backbone(data)
        center = (data["coord"] + model.bias_head(feat)) / VOXEL
        logit = model.seg_head(feat)
    top = logit.topk(2, dim=1).values
    if (top[:, 0] - top[:, 1]).min().item() <= 1e-3:
        return None
    pred = logit.argmax(1)
    keep = ~torch.isin(pred, torch.tensor(IGNORE))
    start = 0
    for end in data["offset"].tolist():
        c = center[start:end][keep[start:end]].double()
        if c.shape[0] > 1:
            dist = torch.cdist(c, c)
            if ((dist - THRESH).abs() < MARGIN * THRESH).any():
                return None
        start = end
    return keep


def train_step(model, data, tag, res):
    model.train()
    model.zero_grad()
    out = model(dict(data))
    assert sorted(out.keys()) == ["bias_cosine_loss", "bias_l1_loss", "loss", "seg_loss"]
    out["loss"].backward()
    for k in out:
        res[f"{tag}_{k}"] = out[k].detach().numpy()
    for k, p in model.named_parameters():
        top = p.grad.abs().max().clamp(min=1e-30)
        res[f"{tag}_grad_{k}"] = (p.grad / top).to(torch.float16).numpy()
        res[f"{tag}_gmax_{k}"] = top.numpy()
    res.update({f"{tag}_buf_{k}": b.detach().numpy().copy() for k, b in model.named_buffers() if "running" in k})
    print(tag, {k: float(out[k]) for k in out})


def instance_parser_sample(res):
    try:
        import torchvision  # noqa: F401
    except ImportError:
        tv = types.ModuleType("torchvision")
        tv.transforms = types.ModuleType("torchvision.transforms")
        sys.modules.update({"torchvision": tv, "torchvision.transforms": tv.transforms})
    ref_loader._bare_pkg("pointcept.datasets", os.path.join(ref_loader.REF, "pointcept", "datasets"))
    tr = importlib.import_module("pointcept.datasets.transform")
    g = np.random.default_rng(5)
    coord = g.random((300, 3)).astype(np.float32)
    instance = g.integers(-1, 9, size=300).astype(np.int64) * 3
    segment = np.where(instance >= 0, (instance // 3) % 7 - 1, -1).astype(np.int64)   # classes -1 .. 5, one per instance
    res["ip_coord"], res["ip_segment"], res["ip_instance"] = coord.copy(), segment.copy(), instance.copy()
    out = tr.InstanceParser(segment_ignore_index=IGNORE, instance_ignore_index=-1)(
        dict(coord=coord, segment=segment, instance=instance))
    res["ip_out_instance"], res["ip_out_centroid"], res["ip_out_bbox"] = (out["instance"], out["instance_centroid"],
                                                                           out["bbox"])
    print("InstanceParser sample:", out["bbox"].shape[0], "instances")


def main():
    assert ref_loader.available()
    ref_loader.load()
    _install_pointgroup_ops_stub()
    from pointcept.models.builder import MODELS

    @MODELS.register_module("PGStandInBackbone")
    class PGStandInBackbone(nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = nn.Linear(6, 64)

        def forward(self, data_dict):
            return self.lin(data_dict["feat"])

    ref_loader._bare_pkg("pointcept.models.point_group", os.path.join(ref_loader.REF, "pointcept", "models", "point_group"))
    m1 = importlib.import_module("pointcept.models.point_group.point_group_v1m1_base").PointGroup
    m2 = importlib.import_module("pointcept.models.point_group.point_group_v1m2_custom_criteria").PointGroup
    criteria = [dict(type="CrossEntropyLoss", loss_weight=0.7, ignore_index=-1)]

    seed = 0
    while True:
        data = make_inputs(seed)
        model = build(m1, seed).eval()
        keep = clean(model, data)
        if keep is not None:
            with torch.no_grad():
                out = model(dict(data))
            sizes = CAPTURED["all_sizes"]
            masks = out["pred_masks"].numpy()
            scene = np.searchsorted(data["offset"].numpy(), masks.argmax(1), side="right") if masks.shape[0] else []
            per_scene = np.bincount(scene, minlength=len(BLOBS)) if masks.shape[0] else np.zeros(len(BLOBS))
            if not np.isin(sizes, [MIN_POINTS - 1, MIN_POINTS, PROPOSE, PROPOSE + 1]).any() and per_scene.min() >= 2:
                break
        seed += 1
        assert seed < 40, "no clean seed"
        print("seed", seed - 1, "rejected", flush=True)
    print("seed", seed, "; kept rows", int(keep.sum()), "of", keep.shape[0], "; component sizes", sorted(sizes.tolist()),
          "; proposals per scene", per_scene.tolist(), "; largest neighbour count", CAPTURED["max_count"])
    assert CAPTURED["max_count"] <= 1000
    assert sorted(out.keys()) == ["bias_cosine_loss", "bias_l1_loss", "loss", "pred_classes", "pred_masks", "pred_scores",
                                  "seg_loss"]
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    res = {"in_" + k: v.numpy() for k, v in data.items()}
    res.update({"sd_" + k: v.numpy() for k, v in sd0.items()})
    rows = keep.nonzero().view(-1).numpy()
    idxs, offs = CAPTURED["clusters"]
    idxs = R.sort_members(idxs, offs)
    idxs[:, 1] = rows[idxs[:, 1]]
    res["proposals_idx"], res["proposals_offset"] = idxs.astype(np.int32), offs.astype(np.int32)
    res["pred_classes"], res["pred_scores"] = out["pred_classes"].numpy(), out["pred_scores"].numpy()
    mask_rows = [np.nonzero(m)[0].astype(np.int32) for m in masks]
    res["pred_mask_rows"] = np.concatenate(mask_rows)
    res["pred_mask_offset"] = np.concatenate([[0], np.cumsum([len(r) for r in mask_rows])]).astype(np.int32)
    for k in ("loss", "seg_loss", "bias_l1_loss", "bias_cosine_loss"):
        res["eval_" + k] = out[k].numpy()

    # PG-v1m2 with the same weights: the same eval results
    model2 = build(m2, seed, criteria=criteria).eval()
    model2.load_state_dict(sd0, strict=True)
    with torch.no_grad():
        out2 = model2(dict(data))
    assert torch.equal(out2["pred_masks"], out["pred_masks"]) and torch.equal(out2["pred_scores"], out["pred_scores"])
    assert torch.equal(out2["pred_classes"], out["pred_classes"])
    res["eval_v1m2_seg_loss"] = out2["seg_loss"].numpy()

    train_step(model, data, "v1m1", res)
    train_step(model2, data, "v1m2", res)
    res["seed"] = np.array(seed)
    instance_parser_sample(res)
    path = os.path.join(HERE, "pointgroup_tiny.npz")
    np.savez_compressed(path, **res)
    print("pointgroup_tiny.npz", os.path.getsize(path) // 1024, "KiB;", len(res["pred_classes"]), "proposals, classes",
          res["pred_classes"].tolist())

    # state_dict listings of the two scannet configs
    write_listing(MODELS.build(_cfg("configs/scannet/insseg-pointgroup-v1m2-0-ptv3-base.py")),
                  "state_dict_pointgroup_v1m2_ptv3_scannet.txt")
    from make_golden_keypoint_spunet import _load_reference
    _load_reference()
    write_listing(MODELS.build(_cfg("configs/scannet/insseg-pointgroup-v1m1-0-spunet-base.py")),
                  "state_dict_pointgroup_v1m1_spunet_scannet.txt")


if __name__ == "__main__":
    main()
