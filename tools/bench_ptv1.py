"""Time the KeypointPTv1 kernels with HIP events (median of --steps calls after --warmup):
  * farthest point sampling, the four strided stages (n -> n/4 -> n/16 -> n/64 -> n/256) of one 100 000-point scene and of
    8 x 20 000 points (beside nothing: there is no other implementation on this machine);
  * ops.vector_attention at the five (c, ns) shapes, at the row counts the stages of an 8 x 20 000 batch have, beside the
    torch-op composition of the same formula (indexing gathers, folded BatchNorm, matmul, softmax);
  * the KeypointPTv1-50 eval forward at 8 x 20 000 points, fused kernels beside the torch composition (set_fused(False)).
Prints one JSON line per measurement.
usage: python tools/bench_ptv1.py [--steps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402


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


def _ends(sizes):
    out, total = [], 0
    for s in sizes:
        total += s
        out.append(total)
    return out


def bench_fps(sizes, steps, warmup, dev):
    from ptv3_hip import ops
    g = torch.Generator(device=dev).manual_seed(1)
    xyz = torch.rand(sum(sizes), 3, device=dev, generator=g)
    total = 0.0
    for stage in range(2, 6):
        new_sizes = [s // 4 for s in sizes]
        ends, new_ends = _ends(sizes), _ends(new_sizes)
        off = torch.tensor(ends, dtype=torch.int32, device=dev)
        noff = torch.tensor(new_ends, dtype=torch.int32, device=dev)
        ms = _time(lambda: ops.farthest_point_sampling(xyz, off, noff, ends, new_ends), steps, warmup)
        idx = ops.farthest_point_sampling(xyz, off, noff, ends, new_ends)
        total += ms
        print(json.dumps({"op": "farthest_point_sampling", "stage": stage, "scenes": len(sizes), "scene_points": sizes[0],
                          "samples_per_scene": new_sizes[0], "ms": round(ms, 3),
                          "us_per_selection": round(1e3 * ms / max(new_sizes[0] - 1, 1), 3)}), flush=True)
        xyz, sizes = xyz[idx.long()].contiguous(), new_sizes
    print(json.dumps({"op": "farthest_point_sampling", "stage": "all", "ms": round(total, 3)}), flush=True)


def _composition(layer, p, x_q, x_k, x_v, idx):
    """The kernel's formula as torch ops in fp32 (running-statistic BatchNorm as its folded scale and shift)."""
    from ptv3_hip import ops

    def bn(m, t):
        scale, shift = ops.fold_batchnorm(m)
        return t * scale + shift
    n, ns = idx.shape
    c = x_q.shape[1]
    have = (idx >= 0).float().unsqueeze(-1)
    j = idx.long().clamp(min=0)
    lp, lw = layer.linear_p, layer.linear_w
    p_r = lp[3](torch.relu(bn(lp[1], lp[0]((p[j] - p.unsqueeze(1)) * have))))
    r = x_k[j] * have - x_q.unsqueeze(1) + p_r
    w = torch.softmax(lw[5](torch.relu(bn(lw[3], lw[2](torch.relu(bn(lw[0], r)))))), dim=1)
    return ((x_v[j] * have + p_r).view(n, ns, 8, c // 8) * w.unsqueeze(2)).sum(1).reshape(n, c)


def bench_attention(steps, warmup, dev):
    import pointops
    from ptv3_hip import ops
    from pointcept.models.point_transformer.point_transformer_seg import PointTransformerLayer
    for c, ns, per_scene in ((32, 8, 20000), (64, 16, 5000), (128, 16, 1250), (256, 16, 312), (512, 16, 78)):
        torch.manual_seed(c)
        layer = PointTransformerLayer(c, c, 8, ns).to(dev).eval()
        n = 8 * per_scene
        p = torch.rand(n, 3, device=dev)
        off = torch.tensor(_ends([per_scene] * 8), dtype=torch.int32, device=dev)
        idx, _ = pointops.knn_query(ns, p, off)
        x_q, x_k, x_v = (torch.randn(n, c, device=dev) for _ in range(3))
        lp, lw = layer.linear_p, layer.linear_w
        f = lambda t: t.detach().float().contiguous()   # noqa: E731
        args = (x_q, x_k, x_v, p, idx, f(lp[0].weight), *ops.fold_batchnorm(lp[1], lp[0].bias), f(lp[3].weight),
                f(lp[3].bias), *ops.fold_batchnorm(lw[0]), f(lw[2].weight), *ops.fold_batchnorm(lw[3], lw[2].bias),
                f(lw[5].weight), f(lw[5].bias))
        with torch.no_grad():
            fused = _time(lambda: ops.vector_attention(*args), steps, warmup)
            torch_ms = _time(lambda: _composition(layer, p, x_q, x_k, x_v, idx), steps, warmup)
            err = (ops.vector_attention(*args) - _composition(layer, p, x_q, x_k, x_v, idx)).abs().max().item()
        print(json.dumps({"op": "vector_attention", "c": c, "ns": ns, "rows": n, "fused_ms": round(fused, 4),
                          "torch_composition_ms": round(torch_ms, 4), "speedup": round(torch_ms / fused, 2),
                          "max_abs_diff": err}), flush=True)


def bench_model(steps, warmup, dev):
    import ptv3_scenes as S
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_PTV1_CFG
    torch.manual_seed(0)
    model = build_model(KEYPOINT_PTV1_CFG).to(dev).eval()
    data = {k: v.to(dev) for k, v in S.make_batch([20000] * 8, in_channels=4, extent=None, seed=7).items()}

    def forward():
        with torch.no_grad():
            return model(dict(data))["pred"]
    fused = _time(forward, steps, warmup)
    pred = forward()
    model.set_fused(False)
    plain = _time(forward, steps, warmup)
    diff = (forward() - pred).abs().max().item()
    print(json.dumps({"op": "KeypointPTv1-50 eval", "scenes": 8, "scene_points": 20000, "fused_ms": round(fused, 3),
                      "torch_composition_ms": round(plain, 3), "speedup": round(plain / fused, 2),
                      "max_abs_diff_pred": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ptv1 measures on the GPU only"
    dev = torch.device("cuda:0")
    fps_steps = max(3, args.steps // 4)
    bench_fps([100000], fps_steps, 1, dev)
    bench_fps([20000] * 8, fps_steps, 1, dev)
    bench_attention(args.steps, args.warmup, dev)
    bench_model(max(3, args.steps // 2), 2, dev)


if __name__ == "__main__":
    main()
