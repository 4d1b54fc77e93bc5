"""Build-container-only: run the reference's KeypointOctFormer and OffsetKeypointOctFormer (pointcept/models/
keypoint_octformer.py and offset_keypoint_octformer.py over octformer/octformer_v1m1_base.py, all three imported in place)
on a seeded three-scene batch and store, in keypoint_octformer_tiny.npz (+ _grad<i>.npz), the inputs, the node counts and
keys of every depth, strided feature taps (patch embed, every stage, the decoder output, the interpolated rows), the
input and output of one dilated OctreeAttention, eval `pred` and loss of both models and one training step of
KeypointOctFormer (loss, curves, every parameter gradient as float16 of grad / max|grad|, the updated BatchNorm
statistics).  Also lists the state_dicts of the models built from configs/my_dataset/keypoint_octformer.py and
offset_keypoint_octformer.py.

Stand-ins for what the reference imports and this machine lacks (parity with the packages is unpinned):
  ocnn (octree.Octree / Points / key2xyz, nn.OctreeConv / OctreeDeconv / OctreeUpsample / OctreeInterp / OctreeDropPath,
  modules.OctreeConvBnRelu / OctreeDeconvBnRelu), dwconv.OctreeDWConv, torch_scatter.scatter_mean
                                         tests/octree_ref.py (plain torch on the CPU, restated from the published sources)
The float64 model keeps the fp32 COORDINATES: the octree is part of the input's definition and must be the same in both
runs; only the feature arithmetic is float64.

The tiny model takes patch_size, dilation, stem_down, head_up, four stages and head dimension 16 from the fork config and
shrinks octree_depth to 7 and the widths; drop_path = 0 and the head's Dropout at p = 0 (the RNG streams cannot be
shared between CPU and device).  Weights are drawn from the key names (seeded_state_dict) and not stored; RPE tables
~ 0.5 N so that they stay in play.

The script asserts what the tests rest on:
  * every cell expression, evaluated in float64, lies at least 1e-4 from an integer and equals its fp32 value;
  * some patch straddles two scenes and some group is part padding;
  * the deepest stage of the 40-point scene has fewer than 26 nodes;
  * several leaves hold more than one point;
  * some coordinate difference inside a patch exceeds pos_bnd at dilation 1, so the clamp is exercised.
fp32 against float64 gaps are printed and stored as gap_*.  If an assertion fails, change the seed, not the tolerance.
usage: python tests/golden/make_golden_keypoint_octformer.py [find-seed]"""
import importlib
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from make_golden_keypoint_ptv1 import seeded_state_dict as _seeded  # noqa: E402
from make_golden_keypoint_oacnns import check_step  # noqa: E402,F401

TINY_KW = dict(in_channels=4, num_keypoints=6, hidden_dim=64, fpn_channels=24, channels=(16, 32, 64, 64),
               num_blocks=(2, 2, 2, 2), num_heads=(1, 2, 4, 4), patch_size=26, stem_down=2, head_up=2, dilation=4,
               drop_path=0.0, nempty=True, octree_scale_factor=10.24, octree_depth=7, octree_full_depth=2)
SIZES = [1500, 40, 2600]
EDGES = [17.0, 3.0, 19.0]
DATA_SEED = 114                 # first seed whose margins hold (searched by find_seed())
TAPS = ("patch_embed", "stage0", "stage1", "stage2", "stage3", "decoder", "interp")
TAP_STRIDE = {"patch_embed": 4, "stage0": 4, "stage1": 1, "stage2": 1, "stage3": 1, "decoder": 16, "interp": 16}
ATTN_BLOCK = "layers.0.blocks.1.attention"      # dilation 4, at the finest stage
CELL_MARGIN = 1e-4
GRAD_PART_BYTES = 900 * 1024
NAME = "keypoint_octformer_tiny"


def seeded_state_dict(shapes, seed=1234):
    """make_golden_keypoint_ptv1.seeded_state_dict, with the tensors it has no rule for: octree conv weights
    (kdim, cin, cout) ~ N(0, 1 / (kdim cin)), depthwise weights (27, 1, C) ~ N(0, 1 / 27), RPE tables ~ 0.5 N."""
    out = _seeded(shapes, seed)
    for key, v in shapes.items():
        shape = tuple(v.shape) if hasattr(v, "shape") else tuple(v)
        rs = np.random.RandomState((zlib.crc32(key.encode()) ^ seed ^ 0x0C7) & 0x7FFFFFFF)
        if key.endswith("rpe_table"):
            a = 0.5 * rs.standard_normal(shape)
        elif key.endswith(".weights"):
            a = rs.standard_normal(shape) / np.sqrt(shape[0] * shape[1])
        else:
            continue
        out[key] = torch.from_numpy(np.asarray(a, dtype=np.float32))
    return out


def load_golden(golden_dir):
    """{name: array} of keypoint_octformer_tiny.npz and exactly the `grad_parts` gradient files it names"""
    out = {}
    with np.load(os.path.join(golden_dir, NAME + ".npz")) as g:
        out.update({k: g[k] for k in g.files})
    want = [f"{NAME}_grad{i}.npz" for i in range(int(out.pop("grad_parts")))]
    have = sorted(f for f in os.listdir(golden_dir) if f.startswith(NAME + "_grad"))
    assert have == want, (have, want)
    for fname in want:
        with np.load(os.path.join(golden_dir, fname)) as g:
            assert not set(g.files) & set(out), fname
            out.update({k: g[k] for k in g.files})
    return out


def make_scenes(seed):
    """Three sheets z = 1.5 sin(0.4 x) + 0.1 N over a square of the scene's edge, centred on the origin; the last forty
    rows of the first scene sit in a blob of radius 0.1 (leaves with several points).  coord (n, 3) fp32, feat (n, 4)
    fp32, offset (3) int64."""
    rs = np.random.RandomState(seed)
    coord = []
    for k, (n, e) in enumerate(zip(SIZES, EDGES)):
        xy = (rs.rand(n, 2) - 0.5) * e
        z = 1.5 * np.sin(0.4 * xy[:, 0]) + 0.1 * rs.randn(n)
        c = np.concatenate([xy, z[:, None]], 1)
        if k == 0:
            d = rs.randn(40, 3)
            c[-40:] = c[700] + 0.1 * d / np.linalg.norm(d, axis=1, keepdims=True) * rs.rand(40, 1) ** (1 / 3)
        coord.append(c + 0.3 * rs.randn(3))
    coord = np.concatenate(coord).astype(np.float32)
    feat = rs.randn(len(coord), 4).astype(np.float32)
    return coord, feat, np.cumsum(SIZES).astype(np.int64)


def cell_margin(coord):
    """smallest distance of a cell expression from an integer in float64, and whether the fp32 cells equal the float64
    ones"""
    c32 = torch.as_tensor(coord, dtype=torch.float32)
    half = float(2 ** (TINY_KW["octree_depth"] - 1))
    e32 = (c32 / TINY_KW["octree_scale_factor"] + 1.0) * half
    e64 = (c32.double() / TINY_KW["octree_scale_factor"] + 1.0) * half
    return float((e64 - torch.round(e64)).abs().min()), bool((torch.floor(e32).long() == torch.floor(e64).long()).all())


def find_seed(limit=4000):
    for seed in range(limit):
        margin, same = cell_margin(make_scenes(seed)[0])
        if margin >= 2 * CELL_MARGIN and same:
            return seed
    raise RuntimeError("no seed holds the margins")


def _load_reference():
    import ref_loader
    import octree_ref
    assert ref_loader.available()
    ref_loader.load()
    octree_ref.install_standins()
    ref_loader._bare_pkg("pointcept.models.octformer", os.path.join(ref_loader.REF, "pointcept", "models", "octformer"))
    importlib.import_module("pointcept.models.octformer.octformer_v1m1_base")
    return (importlib.import_module("pointcept.models.keypoint_octformer"),
            importlib.import_module("pointcept.models.offset_keypoint_octformer"), ref_loader)


def _tapped(model, data, train=False):
    taps, hooks = {}, []

    def tap(name, pick=lambda o: o):
        return lambda m, i, o: taps.__setitem__(name, pick(o).detach().clone())
    hooks.append(model.patch_embed.register_forward_hook(tap("patch_embed")))
    for i, layer in enumerate(model.layers):
        hooks.append(layer.register_forward_hook(tap(f"stage{i}")))
    hooks.append(model.decoder.register_forward_hook(tap("decoder")))
    hooks.append(model.interp.register_forward_hook(tap("interp")))
    attn = dict(model.named_modules())[ATTN_BLOCK]
    hooks.append(attn.register_forward_hook(
        lambda m, i, o: taps.update({"attn_in": i[0].detach().clone(), "attn_out": o.detach().clone(),
                                     "octree": i[1], "attn_depth": i[2]})))
    if train:
        model.train()
        model.reg_head[3].p = 0.0
        model.zero_grad()
        out = model(dict(data))
        out["loss"].backward()
    else:
        with torch.no_grad():
            out = model.eval()(dict(data))
    for h in hooks:
        h.remove()
    return out, taps


def _assert_layout(octree, res):
    """the layout properties the tests rest on, from the octree the reference built"""
    k, dil = TINY_KW["patch_size"], TINY_KW["dilation"]
    top = TINY_KW["octree_depth"] - TINY_KW["stem_down"]
    straddle = part_pad = clamp = False
    for d in range(top, top - 4, -1):
        key = octree.keys[d]
        n = len(key)
        res[f"keys{d}"] = key.numpy()
        pad = -n % (k * dil)
        scene = torch.cat([key >> 48, torch.full((pad,), len(SIZES))]).view(-1, k)
        straddle |= bool(((scene.min(1).values != scene.max(1).values) & (scene.max(1).values < len(SIZES))).any())
        part_pad |= 0 < pad < k * dil and n > 0
        xyz = torch.stack(octree.xyzb(d)[:3], 1)
        xyz = torch.cat([xyz, xyz.new_zeros((pad, 3))]).view(-1, k, 3)
        same = scene.unsqueeze(2) == scene.unsqueeze(1)
        rel = (xyz.unsqueeze(2) - xyz.unsqueeze(1)).abs().max(-1).values
        clamp |= bool((rel[same] > int(0.8 * k)).any())
        print(f"depth {d}: {n} nodes, per scene {torch.bincount(key >> 48, minlength=3).tolist()}")
    for d in range(1, TINY_KW["octree_depth"] + 1):
        res[f"nnum{d}"] = np.int32(len(octree.keys[d]))
    res[f"keys{TINY_KW['octree_depth']}"] = octree.keys[TINY_KW["octree_depth"]].numpy()
    deepest = octree.keys[top - 3]
    assert straddle and part_pad and clamp, (straddle, part_pad, clamp)
    assert int(((deepest >> 48) == 1).sum()) < k
    multi = int((torch.bincount(octree.leaf) > 1).sum())
    print("leaves with more than one point:", multi)
    assert multi >= 5


def main():
    sys.path.insert(0, ROOT)
    kp, okp, ref_loader = _load_reference()
    coord, feat, ends = make_scenes(DATA_SEED)
    margin, same = cell_margin(coord)
    print(f"cell margin {margin:.3e}, fp32 cells equal float64 cells: {same}")
    assert margin >= CELL_MARGIN and same
    data = {"coord": torch.from_numpy(coord), "feat": torch.from_numpy(feat), "offset": torch.from_numpy(ends)}
    g = torch.Generator().manual_seed(5)
    data["target"] = torch.randn(len(SIZES) * 6, 3, generator=g) * 0.5
    data["scale"] = torch.rand(len(SIZES), generator=g) + 0.5
    res = {"in_" + k: v.numpy() for k, v in data.items()}

    model = kp.KeypointOctFormer(**TINY_KW)
    print("tiny parameters", sum(p.numel() for p in model.parameters()), "entries", len(model.state_dict()))
    sd0 = seeded_state_dict(model.state_dict())
    model.load_state_dict(sd0, strict=True)
    model64 = kp.KeypointOctFormer(**TINY_KW).double()
    model64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd0.items()}, strict=True)
    data64 = {k: (v.double() if v.is_floating_point() and k != "coord" else v) for k, v in data.items()}

    out, taps = _tapped(model, data)
    out64, taps64 = _tapped(model64, data64)
    _assert_layout(taps["octree"], res)
    res["eval_pred"] = out["pred"].numpy()       # the reference's eval forward returns no loss
    gaps = {}
    for name in TAPS:
        x, x64 = taps[name].numpy(), taps64[name].numpy()
        res["tap_" + name] = x[::TAP_STRIDE[name]].copy()
        gaps[name] = float(np.abs(x - x64).max() / max(1.0, np.abs(x64).max()))
    res["attn_in"], res["attn_out"] = taps["attn_in"].numpy(), taps["attn_out"].numpy()
    res["attn_depth"] = np.int32(taps["attn_depth"])
    gaps["attn_out"] = float(np.abs(res["attn_out"] - taps64["attn_out"].numpy()).max()
                             / max(1.0, np.abs(taps64["attn_out"].numpy()).max()))
    gaps["pred"] = float(np.abs(res["eval_pred"] - out64["pred"].numpy()).max())

    # the per-point model: its own head, the same backbone keys
    n = len(coord)
    offset_model = okp.OffsetKeypointOctFormer(**TINY_KW)
    sd_off = seeded_state_dict(offset_model.state_dict())
    offset_model.load_state_dict(sd_off, strict=True)
    offset64 = okp.OffsetKeypointOctFormer(**TINY_KW).double()
    offset64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd_off.items()}, strict=True)
    target = torch.randn(n, 6, 4, generator=g) * 0.5
    target[..., 3] = (torch.rand(n, 6, generator=g) > 0.5).float()
    res["offset_target"] = target.numpy()
    with torch.no_grad():
        o32 = offset_model.eval()({**data, "target": target})
        o64 = offset64.eval()({**data64, "target": target.double()})
    res["offset_pred"], res["offset_loss"] = o32["pred"].numpy()[::16].copy(), o32["loss"].numpy()
    gaps["offset_pred"] = float(np.abs(o32["pred"].numpy() - o64["pred"].numpy()).max())
    gaps["offset_loss"] = abs(float(o32["loss"]) - float(o64["loss"]))

    out, _ = _tapped(model, data, train=True)
    out64, _ = _tapped(model64, data64, train=True)
    res["loss"] = out["loss"].detach().numpy()
    res["mean_dist"] = out["train/mean_dist"].numpy()
    res["kp_dist"] = np.array([out[f"train/kp{i}_dist"].item() for i in range(6)], dtype=np.float32)
    grads = {k: p.grad.detach().clone().numpy() for k, p in model.named_parameters()}
    bufs = {k: b.detach().clone().numpy() for k, b in model.named_buffers() if "running" in k}
    for k, gr in grads.items():
        top = max(float(np.abs(gr).max()), 1e-30)
        res["grad_" + k] = (gr / top).astype(np.float16)
        res["gmax_" + k] = np.float32(top)
    res.update({"buf_" + k: b for k, b in bufs.items()})
    grads64 = {k: p.grad.numpy() for k, p in model64.named_parameters()}
    bufs64 = {k: b.detach().numpy() for k, b in model64.named_buffers() if "running" in k}
    gmax = max(float(np.abs(v).max()) for v in grads64.values())
    check_step(float(res["loss"]), grads, bufs, float(out64["loss"].detach()), grads64, bufs64, gmax)
    stored = {k: res["grad_" + k].astype(np.float32) * res["gmax_" + k] for k in grads}
    check_step(float(res["loss"]), stored, bufs, float(out64["loss"].detach()), grads64, bufs64, gmax)
    gaps["loss"] = abs(float(res["loss"]) - float(out64["loss"]))
    for k, v in gaps.items():
        print(f"fp32 vs float64 gap {k}: {v:.3e}")
        res["gap_" + k] = np.float64(v)

    for f in os.listdir(HERE):
        if f.startswith(NAME):
            os.remove(os.path.join(HERE, f))
    parts, room = [{}], GRAD_PART_BYTES
    for k in grads:
        if res["grad_" + k].nbytes > room and parts[-1]:
            parts.append({})
            room = GRAD_PART_BYTES
        parts[-1]["grad_" + k] = res.pop("grad_" + k)
        room -= parts[-1]["grad_" + k].nbytes
    res["grad_parts"] = np.int32(len(parts))
    for fname, content in [(NAME + ".npz", res)] + [(f"{NAME}_grad{i}.npz", q) for i, q in enumerate(parts)]:
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **content)
        assert os.path.getsize(path) < (1 << 20), (fname, os.path.getsize(path))
        print(fname, os.path.getsize(path) // 1024, "KiB")

    from make_golden_keypoint_regression import write_listing
    from pointcept.models.builder import MODELS
    for cfg, fname in (("keypoint_octformer.py", "state_dict_keypoint_octformer_fork.txt"),
                       ("offset_keypoint_octformer.py", "state_dict_offset_keypoint_octformer_fork.txt")):
        scope = {}
        cfg_path = os.path.join(ref_loader.REF, "configs", "my_dataset", cfg)
        exec(compile(open(cfg_path).read(), cfg_path, "exec"), scope)
        fork = MODELS.build(scope["model"])
        print("fork parameters", sum(p.numel() for p in fork.parameters()))
        write_listing(fork, fname)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "find-seed":
        print("seed", find_seed())
    else:
        main()
