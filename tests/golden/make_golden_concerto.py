"""Build-container-only: run the reference's Concerto (pointcept/models/concerto/concerto_v1m1_base.py, imported in place
through ref_loader's stubs) with sonata_model_type="online" over a tiny four-stage "PT-v3m2" (enc_channels 16, 16, 32, 32,
three stride-2 poolings, otherwise the flags of make_golden_sonata.TINY_BACKBONE) with up_cast_level=1 and
enc2d_upcast_level=2: head_in_channels = 64 at level 2, backbone_out_channels = 80 at level 1, so the extra up-cast is
exercised and pool_corr goes through exactly one level.  Image branch: 6 x 6 patches, 24 channels, enc2d_cos_shift=True,
load_enc2d overridden to StubEncoder (a patchifying convolution behind one class token, read by the reference's DINO
convention: the last patch_h * patch_w tokens), whose weights come from concerto_state_dict like all others.
Stubs installed on top of ref_loader's and make_golden_sonata's, in this script only: torch_scatter.scatter_mean with the
documented semantics (segment_coo, segment_csr(sum), pointops.knn_query and timm.layers.trunc_normal_ are those of
make_golden_sonata._install_stubs / ref_loader), and Tensor.cuda as identity.

Data: make_golden_sonata.make_data (lattice scenes, two global and two local views each) plus 2 and 1 images of 12 x 12
pixels for the two scenes.  global_correspondence (N, 2, 2) float32 holds integer patch coordinates from an exact lattice
projection of the UNMOVED voxel index: image 0 looks along z, (x * 6 // E, y * 6 // E), image 1 along x, (y, z) likewise,
E the lattice extent.  A point is invisible in an image, (-1, -1), when its 4 x 4 x 4 voxel block has
(bx + by + bz + image) % 3 == 0: roughly a third of the entries, in blocks that cover whole stride-2 clusters, so that
some clusters have every child invalid.  Scene 1 has no second image: that column is (-1, -1) throughout.
After one pooling level a mean is a sum of integers over a count of at most 8, so it is either an integer (and the
division exact) or at least 1 / 8 away from one: the truncated patch index is the same for any correctly rounded mean.
The script asserts that, and: every loss has pairs in every student scene (make_golden_sonata's rule), at least 20
occupied patches, a patch with pairs from more than one point, a point with pairs in more than one view.

Stored in concerto_tiny.npz (+ concerto_tiny_part{i}.npz, each file under the size limit): the inputs; the patch
permutation and point mask; the three match indices (teacher rows of the UNROLLED matrix); the shared teacher logits, the
student logits of both heads and the up-cast features they were computed from; the student's level-1 up-cast features
(enc2d_feat) with the level-1 offsets and that pooling's inverse and idx_ptr; the pooled correspondences, patch ids, patch means, projected rows and encoder
rows; the five losses; every student gradient as float16 of grad / max|grad| plus that maximum, `nograd`; the teacher's
parameters and the 2D teacher prototype after one after_step at momentum 0.9 - and, as `gap_*`, the largest difference of
each tensor between this fp32 run and the same computation in float64.
Also lists the state_dict of the class built from configs/concerto/pretrain-concerto-v1m1-0-base.py with StubEncoder.
usage: python tests/golden/make_golden_concerto.py"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

from make_golden_sonata import GRID, SEED, PERM_SEED, MOMENTUM, PAIRINGS, PART_BYTES, TINY_BACKBONE, sonata_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

LOSSES = ("mask_loss", "roll_mask_loss", "unmask_loss", "enc2d_loss", "loss")
IMG_NUM = (2, 1)
PATCH, PIXELS, ENC_CHANNELS = 6, 12, 24
TINY_BACKBONE4 = dict(TINY_BACKBONE, stride=(2, 2, 2), enc_depths=(1, 1, 1, 1), enc_channels=(16, 16, 32, 32),
                      enc_num_head=(1, 1, 2, 2), enc_patch_size=(16, 16, 16, 16))
TINY_KW = dict(image_weight_name="stub", image_weight_path=None, backbone=TINY_BACKBONE4, head_in_channels=64,
               backbone_out_channels=80, embedding_channels=16, patch_w=PATCH, patch_h=PATCH, head_hidden_channels=64,
               head_embed_channels=16, head_num_prototypes=100, enc2d_head_in_channels=ENC_CHANNELS,
               enc2d_head_hidden_channels=32, enc2d_head_embed_channels=16, enc2d_head_num_prototypes=20,
               num_global_view=2, num_local_view=2, mask_size_start=1.0, mask_ratio_start=0.5, mask_jitter=None,
               match_max_r=0.04, mask_loss_weight=1 / 8, roll_mask_loss_weight=1 / 8, unmask_loss_weight=2 / 8,
               enc2d_loss_weight=4 / 8, up_cast_level=1, enc2d_upcast_level=2, enc2d_cos_shift=True,
               sonata_model_type="online")


class StubEncoder(nn.Module):
    """A deterministic stand-in for the frozen image encoder: non-overlapping patches through one convolution, behind a
    zero class token.  `tokens` x `tokens` patches of `pixels // tokens` pixels, `channels` wide."""

    def __init__(self, channels=ENC_CHANNELS, tokens=PATCH, pixels=PIXELS):
        super().__init__()
        self.proj = nn.Conv2d(3, channels, kernel_size=pixels // tokens, stride=pixels // tokens)

    def forward(self, x):
        y = self.proj(x).flatten(2).transpose(1, 2)
        return types.SimpleNamespace(last_hidden_state=torch.cat([torch.zeros_like(y[:, :1]), y], dim=1))


def with_stub_encoder(cls, **stub_kw):
    """`cls` (the reference's Concerto or the library's) with load_enc2d returning a StubEncoder"""
    return type(cls.__name__, (cls,), dict(load_enc2d=lambda self, name, weight: StubEncoder(**stub_kw).eval()))


def concerto_state_dict(model):
    """Loads the seeded weights into `model` (the reference class or the library's) and returns its state_dict."""
    return sonata_state_dict(model)


def load_golden(golden_dir):
    """{name: array} of concerto_tiny.npz and exactly the `parts` files it names"""
    out = {}
    with np.load(os.path.join(golden_dir, "concerto_tiny.npz")) as g:
        out.update({k: g[k] for k in g.files})
    want = [f"concerto_tiny_part{i}.npz" for i in range(int(out.pop("parts")))]
    have = sorted(f for f in os.listdir(golden_dir) if f.startswith("concerto_tiny_part"))
    assert have == want, (have, want)
    for fname in want:
        with np.load(os.path.join(golden_dir, fname)) as g:
            out.update({k: g[k] for k in g.files})
    return out


def make_data():
    from make_golden_sonata import make_data as sonata_data
    data = sonata_data()
    g = torch.Generator().manual_seed(77)
    data["images"] = torch.rand(sum(IMG_NUM), 3, PIXELS, PIXELS, generator=g)
    data["img_num"] = torch.tensor(IMG_NUM, dtype=torch.int64)
    vox = torch.round(data["global_origin_coord"] / GRID).long()
    vox = vox - vox.min(0)[0]
    extent = int(vox.max()) + 1
    cell = vox * PATCH // extent
    block = (vox // 4).sum(1)
    corr = -torch.ones(vox.shape[0], max(IMG_NUM), 2)
    ends = data["global_offset"].tolist()
    view = torch.bucketize(torch.arange(vox.shape[0]), data["global_offset"], right=True)
    for image, axes in enumerate(([0, 1], [1, 2])):
        seen = ((block + image) % 3 != 0) & (torch.tensor(IMG_NUM)[view // 2] > image)
        corr[seen, image] = cell[seen][:, axes].float()
    assert len(ends) == 2 * len(IMG_NUM)
    data["global_correspondence"] = corr
    return data


def _install_stubs():
    import ref_loader
    import make_golden_sonata as S
    S._install_stubs()

    def scatter_mean(src, index, dim=0, dim_size=None):
        assert dim == 0
        total = torch.zeros((dim_size,) + src.shape[1:], dtype=src.dtype).index_add_(0, index, src)
        count = torch.zeros(dim_size, dtype=src.dtype).index_add_(0, index, torch.ones(index.shape[0], dtype=src.dtype))
        return total / count.clamp(min=1).view((-1,) + (1,) * (src.dim() - 1))

    sys.modules["torch_scatter"].scatter_mean = scatter_mean
    torch.Tensor.cuda = lambda self, *a, **k: self
    ref_loader._bare_pkg("pointcept.models.concerto", os.path.join(ref_loader.REF, "pointcept", "models", "concerto"))
    return importlib.import_module("pointcept.models.concerto.concerto_v1m1_base")


def _run(cls, kw, sd, data, perm, dtype):
    """one training forward + backward of the reference class in `dtype`, everything the tests need captured"""
    cast = lambda v: v.to(dtype) if v.is_floating_point() else v  # noqa: E731
    kw = dict(kw, backbone=sys.modules["addict"].Dict(kw["backbone"]))
    model = cls(**kw).to(dtype)
    model.load_state_dict({k: cast(v) for k, v in sd.items()}, strict=True)
    model.train()
    cap = {"match": [], "target": [], "perm": []}
    ts = sys.modules["torch_scatter"]
    real_randperm, real_sk, real_match, real_pool, real_scatter = (torch.randperm, cls.sinkhorn_knopp,
                                                                   cls.match_neighbour, cls.pool_corr, ts.scatter_mean)

    def randperm(n, **kwargs):
        if "device" not in kwargs:          # the order shuffle of a GridPooling: torch's CPU generator, seeded below
            return real_randperm(n, **kwargs)
        out = real_randperm(n, generator=torch.Generator().manual_seed(PERM_SEED)) if perm is None else perm
        assert out.shape[0] == n
        cap["perm"].append(out)
        return out

    def sinkhorn(feat, temp, num_iter=3):
        out = real_sk(feat, temp, num_iter)
        cap["target"].append(out.detach().clone())
        return out

    def match(self, *args):
        out = real_match(self, *args)
        cap["match"].append(out.clone())
        return out

    def pool_corr(point, correspondence):
        cap["level1_offset"] = point.offset.clone()
        cap["pool_inverse"], cap["pool_idx_ptr"] = point["pooling_inverse"].clone(), point["idx_ptr"].clone()
        out = real_pool(point, correspondence)
        cap["pooled_corr"], cap["enc2d_feat"] = out["correspondence"].detach().clone(), out["feat"].detach().clone()
        return out

    def scatter_mean(src, index, dim=0, dim_size=None):
        out = real_scatter(src, index, dim=dim, dim_size=dim_size)
        cap["pair_patch"] = index.clone()
        cap["patch_ids"] = torch.unique(index)
        cap["patch_mean"] = out.detach()[cap["patch_ids"]].clone()
        return out

    def generate_mask(coord, offset, real=model.generate_mask):
        cap["mask"], cap["cluster"] = real(coord, offset)
        return cap["mask"], cap["cluster"]

    def up_cast(point, upcast_level=None, real=model.up_cast):
        out = real(point, upcast_level=upcast_level)
        cap.setdefault("offsets", []).append(out.offset.clone())
        return out

    def encoder(x, real=model.ENC2D_forward):
        out = real(x)
        cap["encoder"] = out.detach().reshape(-1, out.shape[-1]).clone()
        return out

    hooks = [model.patch_proj.register_forward_hook(lambda m, i, o: cap.update(projected_all=o.detach().clone()))]
    for key, head in (("student_mask_head", model.student.mask_head), ("student_unmask_head", model.student.unmask_head),
                      ("teacher_mask_head", model.teacher.mask_head)):
        hooks.append(head.register_forward_hook(
            lambda m, i, o, key=key: cap.update({key + "_in": i[0].detach().clone(), key + "_out": o.detach().clone()})))
    torch.randperm, cls.sinkhorn_knopp, cls.match_neighbour = randperm, staticmethod(sinkhorn), match
    cls.pool_corr, ts.scatter_mean = staticmethod(pool_corr), scatter_mean
    model.generate_mask, model.ENC2D_forward, model.up_cast = generate_mask, encoder, up_cast
    try:
        torch.manual_seed(SEED)
        out = model({k: cast(v) for k, v in data.items()})
        out["loss"].backward()
    finally:
        torch.randperm, cls.sinkhorn_knopp, cls.match_neighbour = real_randperm, real_sk, real_match
        cls.pool_corr, ts.scatter_mean = staticmethod(real_pool), real_scatter
    for h in hooks:
        h.remove()
    assert len(cap["perm"]) == 1 and len(cap["match"]) == 3 and len(cap["target"]) == 3, \
        [len(cap[k]) for k in ("perm", "match", "target")]
    res = {k: out[k].detach() for k in LOSSES}
    res["patch_index"], res["point_mask"] = cap["perm"][0], cap["mask"]
    for name, m, t in zip(PAIRINGS, cap["match"], cap["target"]):
        res["match_" + name], res["target_" + name] = m, t
    for key in ("student_mask_head", "student_unmask_head", "teacher_mask_head"):
        res[key + "_in"], res[key + "_out"] = cap[key + "_in"], cap[key + "_out"]
    for key in ("pooled_corr", "patch_ids", "patch_mean", "enc2d_feat", "pair_patch", "pool_inverse", "pool_idx_ptr"):
        res[key] = cap[key]
    assert len(cap["offsets"]) == 4 and torch.equal(cap["offsets"][3], cap["level1_offset"])
    res["offset_teacher"], res["offset_mask"], res["offset_local"], res["offset_enc2d"] = cap["offsets"]
    res["projected"] = cap["projected_all"][cap["patch_ids"]]
    res["encoder_rows"] = cap["encoder"][cap["patch_ids"]]
    res["nograd"] = [k for k, p in model.named_parameters() if p.grad is None]
    for k, p in model.named_parameters():
        if p.grad is not None:
            res["fullgrad_" + k] = p.grad.detach().clone()
    model.momentum = MOMENTUM
    model.after_step()
    for k, p in model.teacher.named_parameters():
        res["ema_teacher." + k] = p.detach().clone()
    for k, p in model.enc2d_head_teacher.named_parameters():
        res["ema_enc2d_head_teacher." + k] = p.detach().clone()
    return res, model


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    from transformers import AutoModel  # noqa: F401  before ref_loader's bare `timm` stub, which transformers cannot probe
    import ref_loader
    from make_golden_keypoint_regression import write_listing
    from make_golden_swin3d import _cfg
    ref_loader.load()
    ref = _install_stubs()
    cls = with_stub_encoder(ref.Concerto)
    data = make_data()
    probe = cls(**dict(TINY_KW, backbone=sys.modules["addict"].Dict(TINY_BACKBONE4)))
    sd0 = concerto_state_dict(probe)
    r32, _ = _run(cls, TINY_KW, sd0, data, None, torch.float32)
    r64, _ = _run(cls, TINY_KW, sd0, data, r32["patch_index"], torch.float64)
    assert torch.equal(r32["point_mask"], r64["point_mask"]) and r32["nograd"] == r64["nograd"]
    # what the tests rely on
    assert 0.2 < float(r32["point_mask"].float().mean()) < 0.8
    t_off = r32["offset_teacher"]
    for k in ("offset_teacher", "offset_mask", "offset_local", "offset_enc2d"):
        assert torch.equal(r32[k], r64[k]), k
    # the roll and the principal views at the teacher's level: the tests index the UNROLLED teacher matrix
    starts = [0] + t_off.tolist()
    roll_perm = torch.cat([torch.arange(starts[i], starts[i + 1]) for i in (1, 0, 3, 2)])
    t_batch = torch.bucketize(torch.arange(int(t_off[-1])), t_off, right=True)
    principal = (t_batch % 2 == 0).nonzero().squeeze(1)
    for name in PAIRINGS:
        assert torch.equal(r32["match_" + name], r64["match_" + name]), name
        off = r32["offset_local"] if name == "unmask" else r32["offset_mask"]
        scene = torch.bucketize(r32["match_" + name][:, 0].contiguous(), off, right=True)
        assert torch.bincount(scene, minlength=len(off)).min() >= 4, (name, torch.bincount(scene, minlength=len(off)))
        fix = r32["match_" + name].clone()
        if name == "roll_mask":
            fix[:, 1] = roll_perm[fix[:, 1]]
        elif name == "unmask":
            fix[:, 1] = principal[fix[:, 1]]
        r32["match_" + name] = fix
    corr = data["global_correspondence"]
    share = float((corr == -1).all(-1).float().mean())
    assert 0.25 < share < 0.75, share
    # exactness: a pooled mean is an integer or at least 1 / 8 away from one, so its truncation does not depend on
    # how the mean was rounded
    p32, p64 = r32["pooled_corr"], r64["pooled_corr"]
    assert torch.equal(p32.long(), p64.long()) and torch.equal(p32 == -1, p64 == -1)
    frac = p64 - p64.floor()
    assert bool(((frac == 0) | ((frac >= 0.125 - 1e-12) & (frac <= 0.875 + 1e-12))).all())
    assert bool(((p32 == -1).all(-1)).any()), "no cluster with every child invalid"
    assert not bool(((p32 == -1).any(-1) != (p32 == -1).all(-1)).any()), "a pooled pair with exactly one entry -1"
    assert torch.equal(r32["patch_ids"], r64["patch_ids"]) and r32["patch_ids"].numel() >= 20, r32["patch_ids"].numel()
    assert int(torch.bincount(r32["pair_patch"]).max()) > 1, "no patch with pairs from more than one point"
    assert bool(((p32 != -1).any(-1).sum(1) > 1).any()), "no point with pairs in more than one view"
    r32.pop("pair_patch"), r64.pop("pair_patch")

    res = {"in_" + k: v.numpy() for k, v in data.items()}
    res["nograd"] = np.array(r32.pop("nograd"))
    r64.pop("nograd")
    res["roll_perm"] = roll_perm.numpy()
    for k, v in r32.items():
        v32 = v.detach()
        if not v32.is_floating_point():
            res[k] = v32.numpy()
            continue
        gap = np.float64((v32.double() - r64[k].detach().double()).abs().max().item())
        if k.startswith("fullgrad_"):
            name = k[len("fullgrad_"):]
            top = v32.abs().max().clamp(min=1e-30)
            res["grad_" + name] = (v32 / top).to(torch.float16).numpy()
            res["gmax_" + name] = top.numpy()
            res["gap_grad_" + name] = gap
        else:
            res[k] = v32.numpy()
            res["gap_" + k] = gap
    print({k: float(res[k]) for k in LOSSES}, "pairs", {n: int(res["match_" + n].shape[0]) for n in PAIRINGS},
          "patches", int(res["patch_ids"].shape[0]), "invalid share", share)
    print("gaps:", {k: float(v) for k, v in res.items() if k.startswith("gap_") and "grad_" not in k and "ema_" not in k})
    parts, room = [{}], PART_BYTES
    for k in sorted(k for k in res if res[k].nbytes > 16 * 1024):
        if res[k].nbytes > room:
            parts.append({})
            room = PART_BYTES
        parts[-1][k] = res.pop(k)
        room -= parts[-1][k].nbytes
    for old in os.listdir(HERE):
        if old.startswith("concerto_tiny_part"):
            os.remove(os.path.join(HERE, old))
    res["parts"] = np.int32(len(parts))
    files = {f"concerto_tiny_part{i}.npz": q for i, q in enumerate(parts)}
    files["concerto_tiny.npz"] = res
    for name, part in files.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        print(" ", name, os.path.getsize(path) // 1024, "KiB")
        assert os.path.getsize(path) <= 1000 * 1024, path
    cfg = _cfg("configs/concerto/pretrain-concerto-v1m1-0-base.py")
    cfg["backbone"] = sys.modules["addict"].Dict(cfg["backbone"])
    cfg.pop("type")
    base = with_stub_encoder(ref.Concerto, channels=8, tokens=cfg["patch_h"], pixels=cfg["patch_h"])
    write_listing(base(**cfg), "state_dict_concerto_base.txt")


if __name__ == "__main__":
    main()
