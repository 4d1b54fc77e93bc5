"""Time the KeypointPTv2 kernels with HIP events (median of --steps calls after --warmup):
  * ops.grouped_vector_attention at the fork's (C, G, ns) - the patch embed, the four encoder stages and the four decoder
    stages - on 8 x 20 000 random points in the unit cube, at the row counts the fork's grid sizes give each level,
    beside the torch-op composition of the same formula (indexing gathers, folded BatchNorm, matmul, softmax, mask);
    with the achieved TFLOP/s of the W_p2 product (2 n ns C^2 flop) against the 157 TF fp32 matrix peak;
  * the whole KeypointPTv2 eval forward on that batch, fused kernels beside the torch composition (set_fused(False)),
    with the distance between their predictions.
Prints one JSON line per measurement.
usage: python tools/bench_ptv2.py [--steps 20] [--warmup 3] [--scenes 8] [--points 20000]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402

FP32_MATRIX_PEAK_TF = 157.0


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(steps):
        start.record()
        fn()
        end.record()
        end.synchronize()
        ms.append(start.elapsed_time(end))
    ms.sort()
    return ms[len(ms) // 2]


def _composition(layer, p, q, k, v, idx):
    """The kernel's formula as torch ops in fp32 (running-statistic BatchNorm as its folded scale and shift)."""
    from ptv3_hip import ops

    def bn(m, t):
        scale, shift = ops.fold_batchnorm(m.norm)
        return t * scale + shift
    n, ns = idx.shape
    c, g = q.shape[1], layer.groups
    have = (idx >= 0).float().unsqueeze(-1)
    j = idx.long().clamp(min=0)
    lp, lw = layer.linear_p_bias, layer.weight_encoding
    peb = lp[3](torch.relu(bn(lp[1], lp[0]((p[j] - p.unsqueeze(1)) * have))))
    r = k[j] * have - q.unsqueeze(1) + peb
    w = torch.softmax(lw[3](torch.relu(bn(lw[1], lw[0](r)))), dim=1) * have
    return ((v[j] * have + peb).view(n, ns, g, c // g) * w.unsqueeze(-1)).sum(1).reshape(n, c)


def levels(cfg, scenes, points, dev):
    """[(coord, offset)] of levels 0..4: random points in the unit cube pooled by the fork's grid sizes."""
    from ptv3_hip import ops
    g = torch.Generator(device=dev).manual_seed(1)
    coord = torch.rand(scenes * points, 3, device=dev, generator=g)
    offset = torch.arange(1, scenes + 1, device=dev, dtype=torch.int32) * points
    out = [(coord, offset)]
    for size in cfg["grid_sizes"]:
        plan = ops.grid_pool_plan(coord, offset, size)
        coord, offset = ops.segment_mean3(coord, plan.order, plan.seg_start, plan.n_out), plan.offset.int()
        out.append((coord, offset))
    return out


def bench_attention(cfg, lv, steps, warmup, dev):
    import pointops
    from ptv3_hip import ops
    from pointcept.models.point_transformer_v2.point_transformer_v2m2_base import GroupedVectorAttention
    shapes = [("patch_embed", 0, cfg["patch_embed_channels"], cfg["patch_embed_groups"], cfg["patch_embed_neighbours"])]
    for i in range(4):
        shapes.append((f"enc{i}", i + 1, cfg["enc_channels"][i], cfg["enc_groups"][i], cfg["enc_neighbours"][i]))
    for i in range(4):
        shapes.append((f"dec{i}", i, cfg["dec_channels"][i], cfg["dec_groups"][i], cfg["dec_neighbours"][i]))
    for name, level, c, g, ns in shapes:
        torch.manual_seed(c)
        layer = GroupedVectorAttention(c, g).to(dev).eval()
        p, off = lv[level]
        n = p.shape[0]
        idx, _ = pointops.knn_query(ns, p, off)
        q, k, v = (torch.randn(n, c, device=dev) for _ in range(3))
        lp, lw = layer.linear_p_bias, layer.weight_encoding
        f = lambda t: t.detach().float().contiguous()   # noqa: E731
        args = (q, k, v, p, idx, g, f(lp[0].weight), *ops.fold_batchnorm(lp[1].norm, lp[0].bias), f(lp[3].weight),
                f(lp[3].bias), f(lw[0].weight), *ops.fold_batchnorm(lw[1].norm, lw[0].bias), f(lw[3].weight),
                f(lw[3].bias))
        with torch.no_grad():
            fused = _time(lambda: ops.grouped_vector_attention(*args), steps, warmup)
            torch_ms = _time(lambda: _composition(layer, p, q, k, v, idx), steps, warmup)
            err = (ops.grouped_vector_attention(*args) - _composition(layer, p, q, k, v, idx)).abs().max().item()
        tf = 2.0 * n * ns * c * c / (fused * 1e-3) / 1e12
        print(json.dumps({"op": "grouped_vector_attention", "layer": name, "c": c, "groups": g, "ns": ns, "rows": n,
                          "fused_ms": round(fused, 4), "torch_composition_ms": round(torch_ms, 4),
                          "speedup": round(torch_ms / fused, 2), "w_p2_tflops": round(tf, 2),
                          "w_p2_fraction_of_fp32_matrix_peak": round(tf / FP32_MATRIX_PEAK_TF, 4),
                          "max_abs_diff": err}), flush=True)


def bench_model(lv, steps, warmup, dev):
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_PTV2_CFG
    torch.manual_seed(0)
    model = build_model(KEYPOINT_PTV2_CFG).to(dev).eval()
    coord, offset = lv[0]
    data = dict(coord=coord, feat=torch.randn(coord.shape[0], 4, device=dev), offset=offset)

    def forward():
        with torch.no_grad():
            return model(dict(data))["pred"]
    fused = _time(forward, steps, warmup)
    pred = forward()
    model.set_fused(False)
    plain = _time(forward, steps, warmup)
    diff = (forward() - pred).abs().max().item()
    print(json.dumps({"op": "KeypointPTv2 eval", "scenes": offset.shape[0], "points": coord.shape[0],
                      "fused_ms": round(fused, 3), "torch_composition_ms": round(plain, 3),
                      "speedup": round(plain / fused, 2), "max_abs_diff_pred": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ptv2 measures on the GPU only"
    dev = torch.device("cuda:0")
    from ptv3_hip.configs import KEYPOINT_PTV2_CFG
    cfg = KEYPOINT_PTV2_CFG["backbone_conf"]
    lv = levels(cfg, args.scenes, args.points, dev)
    print(json.dumps({"op": "levels", "rows": [c.shape[0] for c, _ in lv]}), flush=True)
    bench_attention(cfg, lv, args.steps, args.warmup, dev)
    bench_model(lv, args.steps, args.warmup, dev)


if __name__ == "__main__":
    main()
