"""Time OctFormer's hot paths with HIP events (median of --steps calls after --warmup), per stage depth of the fork
config (channels 96 / 192 / 384 / 384, heads 6 / 12 / 24 / 24, patch 26, dilation 1 and 4):
  * ops.octree_attention (ptv3_octree_attn_fwd) beside ops.octree_attention_torch, the torch composition of the same
    plan (padded copy, dilation transpose, gathered RPE, -1e3 mask, softmax: the reference's algorithm), with the
    bytes of the (patches, K, K, 3, H) table gather that composition materialises;
  * ops.octree_dwconv (ptv3_octree_dwconv) beside ops.octree_dwconv_torch;
  * the whole KeypointOctFormer eval forward, fused beside set_fused(False), with the distance between their
    predictions and the time of ops.octree_build.
Input: --scenes ellipsoid surfaces grid-sampled at 0.02 (the generator of tools/bench_strat.py).
Prints one JSON line per measurement and appends them to profiles/octformer/bench_octformer.jsonl.
usage: python tools/bench_octformer.py [--steps 20] [--warmup 3] [--scenes 8] [--out profiles/octformer/bench_octformer.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

from bench_strat import _time, make_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "octformer", "bench_octformer.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_octformer.py measures on the GPU; there is no CPU timing"
    from pointcept.models import build_model
    from ptv3_hip import ops
    from ptv3_hip.configs import KEYPOINT_OCTFORMER_CFG as CFG
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    data = make_batch(args.scenes, dev)
    n = data["coord"].shape[0]
    rows = []

    def emit(**kw):
        kw.update(scenes=args.scenes, points=n, steps=args.steps)
        print(json.dumps(kw), flush=True)
        rows.append(kw)

    model = build_model(dict(CFG)).to(dev).eval()
    with torch.no_grad():
        oct = model.points2octree(data["coord"], data["feat"], data["offset"])
        emit(what="octree_build", ms=_time(lambda: model.points2octree(data["coord"], data["feat"], data["offset"]),
                                          args.steps, args.warmup),
             nodes={d: oct.nnum[d] for d in sorted(oct.nnum)})
        top = CFG["octree_depth"] - CFG["stem_down"]
        k = CFG["patch_size"]
        for i, (c, heads) in enumerate(zip(CFG["channels"], CFG["num_heads"])):
            depth = top - i
            n_t = oct.nnum[depth]
            x = torch.randn(n_t, c, device=dev)
            qkv = torch.randn(n_t, 3 * c, device=dev)
            for dil in (1, CFG["dilation"]):
                bnd = int(0.8 * k * dil ** 0.5)
                table = 0.02 * torch.randn(3 * (2 * bnd + 1), heads, device=dev)
                a = (qkv, oct.xyz[depth], oct.batch[depth], table, heads, k, dil, bnd, (c // heads) ** -0.5)
                fused = ops.octree_attention(*a, fused=True)
                comp = ops.octree_attention_torch(*a)
                patches = -(-n_t // (k * dil)) * dil
                emit(what="attention", depth=depth, rows=n_t, c=c, heads=heads, dilation=dil,
                     kernel_ms=_time(lambda: ops.octree_attention(*a, fused=True), args.steps, args.warmup),
                     composed_ms=_time(lambda: ops.octree_attention_torch(*a), args.steps, args.warmup),
                     rpe_gather_mb=patches * k * k * 3 * heads * 4 / 1e6,
                     max_abs_diff=(fused - comp).abs().max().item())
            w = torch.randn(27, 1, c, device=dev) / 5
            scale, shift = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev)
            nbr = oct.neighbors(depth)
            emit(what="dwconv", depth=depth, rows=n_t, c=c,
                 kernel_ms=_time(lambda: ops.octree_dwconv(x, w, nbr, scale, shift), args.steps, args.warmup),
                 composed_ms=_time(lambda: ops.octree_dwconv_torch(x, w[:, 0], nbr, scale, shift), args.steps, args.warmup),
                 max_abs_diff=(ops.octree_dwconv(x, w, nbr, scale, shift)
                               - ops.octree_dwconv_torch(x, w[:, 0], nbr, scale, shift)).abs().max().item())
        fused = model.set_fused(True)(dict(data))["pred"]
        fused_ms = _time(lambda: model(dict(data)), args.steps, args.warmup)
        plain = model.set_fused(False)(dict(data))["pred"]
        plain_ms = _time(lambda: model(dict(data)), max(3, args.steps // 4), 1)
        emit(what="eval_forward", fused_ms=fused_ms, composed_ms=plain_ms,
             max_abs_diff=(fused - plain).abs().max().item())
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
