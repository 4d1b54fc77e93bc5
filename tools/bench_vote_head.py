"""Time the voting keypoint head of KeypointSwin3DVote (K = 6, 3K = 18 vote columns) at 1 x 100k and 8 x 100k points:
 (a) ops.scene_median (memset + five launches) on random votes and on clustered votes (every column's values differ in
     the low 8 mantissa bits only: the case in which a histogram's high digits all land on one bin),
 (b) the reference's formulation on the same device - per scene a boolean mask, a gather and median(dim=0)
     (keypoint_swin3d_plus.py:172-187), restated here,
 (c) the fused vote loss forward + backward against the torch composition of :86-164, restated here,
and the KeypointSwin3DVote eval forward against the backbone-only forward on the fork config.  CUDA-event medians, with
the 10th-90th percentile spread of the steps; prints one JSON line per size.  Device times come from running this tool
under `rocprofv3 --kernel-trace --stats` in a run of its own (--no-model keeps that run to the head's kernels).
usage: python tools/bench_vote_head.py [--steps 50] [--warmup 10] [--no-model]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

K = 6


def _time(fn, steps, warmup):
    """(median, p10, p90) in microseconds."""
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
    return [round(ms[i] * 1e3, 1) for i in (len(ms) // 2, len(ms) // 10, len(ms) - 1 - len(ms) // 10)]


def reference_median(votes, coord, batch_idx):
    """The eval branch of the reference: B read back, then per scene mask -> gather -> median."""
    per_point = coord.unsqueeze(1) + votes.view(-1, K, 3)
    preds = []
    for b in range(int(batch_idx.max()) + 1):
        sample = per_point[batch_idx == b]
        preds.append(sample.median(dim=0).values if sample.shape[0] > 0 else per_point.new_zeros(K, 3))
    return torch.stack(preds)


def reference_loss(votes, coord, target, batch_idx, scale, radius):
    """The training branch of the reference as a torch composition (loss and the 1 + K curves)."""
    b = int(batch_idx.max()) + 1
    per_point = coord.unsqueeze(1) + votes.view(-1, K, 3)
    tpp = target.view(b, K, 3)[batch_idx]
    dist = torch.norm(coord.unsqueeze(1) - tpp, p=2, dim=-1)
    mask = (dist < radius).float()
    div = mask.sum().clamp(min=1.0)
    loss = (F.smooth_l1_loss(per_point, tpp, reduction="none").mean(dim=-1) * mask).sum() / div
    with torch.no_grad():
        real = dist * scale[batch_idx].unsqueeze(-1)
        curves = [(real * mask).sum() / div]
        for k in range(K):
            curves.append((real[:, k] * mask[:, k]).sum() / mask[:, k].sum().clamp(min=1.0))
    return loss, curves


def swin_batch(sizes, dev):
    """Scenes of the fork's Swin3D config (4 feature channels), each on a room-like sheet."""
    from bench_swin import surface
    rng = np.random.default_rng(0)
    coords, grids, offs, total = [], [], [], 0
    for i, n in enumerate(sizes):
        g = surface(n, int((n / 1.2) ** 0.5), 1 + i)[:, 1:].astype(np.int64)
        grids.append(g)
        coords.append(((g + rng.random(g.shape)) * 0.02).astype(np.float32))
        total += len(g)
        offs.append(total)
    return {"coord": torch.from_numpy(np.concatenate(coords)).to(dev),
            "grid_coord": torch.from_numpy(np.concatenate(grids)).to(dev),
            "feat": torch.from_numpy(np.clip(rng.normal(size=(total, 4)) * 0.5, -1, 1).astype(np.float32)).to(dev),
            "offset": torch.tensor(offs, device=dev)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    from ptv3_hip import ops
    from ptv3_hip import autograd as A
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for sizes in ([100000], [100000] * 8):
        n, b = sum(sizes), len(sizes)
        off = torch.tensor(np.cumsum(sizes), device=dev)
        batch_idx = torch.repeat_interleave(torch.arange(b, device=dev), torch.tensor(sizes, device=dev))
        coord = torch.rand(n, 3, device=dev)
        target = torch.rand(b * K, 3, device=dev) * 0.7 + 0.15
        scale = torch.rand(b, device=dev) + 0.5
        votes = (target.view(b, K, 3)[batch_idx] - coord.unsqueeze(1) + torch.randn(n, K, 3, device=dev) * 0.05) \
            .reshape(n, 3 * K).contiguous()
        base = (torch.randn(1, 3 * K, device=dev) * 3).view(torch.int32) & ~0xFF
        clustered = (base | torch.randint(0, 256, (n, 3 * K), device=dev, dtype=torch.int32)).view(torch.float32)
        res = {"points": n, "scenes": b}
        with torch.no_grad():
            assert torch.equal(ops.scene_median(votes, coord, off).view(b, K, 3), reference_median(votes, coord, batch_idx))
            res["median_us"] = _time(lambda: ops.scene_median(votes, coord, off), args.steps, args.warmup)
            res["median_random_nocoord_us"] = _time(lambda: ops.scene_median(votes, None, off), args.steps, args.warmup)
            res["median_clustered_nocoord_us"] = _time(lambda: ops.scene_median(clustered, None, off), args.steps,
                                                       args.warmup)
            res["reference_median_us"] = _time(lambda: reference_median(votes, coord, batch_idx), args.steps, args.warmup)
        res["median_speedup"] = round(res["reference_median_us"][0] / res["median_us"][0], 2)
        vh, vr = votes.clone().requires_grad_(True), votes.clone().requires_grad_(True)

        def fused():
            vh.grad = None
            A.vote_loss(vh, coord, target, off, 0.4, scale)[0].backward()

        def composed():
            vr.grad = None
            reference_loss(vr, coord, target, batch_idx, scale, 0.4)[0].backward()
        res["vote_loss_fwd_bwd_us"] = _time(fused, args.steps, args.warmup)
        res["reference_loss_fwd_bwd_us"] = _time(composed, args.steps, args.warmup)
        res["loss_speedup"] = round(res["reference_loss_fwd_bwd_us"][0] / res["vote_loss_fwd_bwd_us"][0], 2)
        if not args.no_model:
            from pointcept.models import build_model
            from ptv3_hip.configs import KEYPOINT_SWIN3D_VOTE_CFG
            torch.manual_seed(0)
            model = build_model(KEYPOINT_SWIN3D_VOTE_CFG).to(dev).eval()
            data = swin_batch(sizes, dev)

            def whole():
                with torch.no_grad():
                    model(dict(data))

            def backbone():
                with torch.no_grad():
                    d = dict(data)
                    d["coord_feat"] = d["feat"]
                    model.backbone(d)
            steps = max(5, args.steps // 10)
            res["model_eval_ms"] = round(_time(whole, steps, 2)[0] / 1e3, 3)
            res["backbone_ms"] = round(_time(backbone, steps, 2)[0] / 1e3, 3)
            res["model_over_backbone"] = round(res["model_eval_ms"] / res["backbone_ms"], 4)
            del model
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
