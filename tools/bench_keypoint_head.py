"""Time the global-regression keypoint head of KeypointPTv3 (fork config, C = 64, H = 256, 3K = 18, bf16 features):
pooling + head alone (ptv3_scene_mean_head: two launches), and the whole KeypointPTv3 eval forward against the
backbone-only forward, at 1 x 100k and 8 x 100k points.  Prints one JSON line per size.
usage: python tools/bench_keypoint_head.py [--steps 50] [--warmup 10]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import ptv3_scenes as S
    from pointcept.models import build_model
    from pointcept.models.keypoint_ptv3 import regress
    from ptv3_hip.configs import KEYPOINT_PTV3_CFG
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(KEYPOINT_PTV3_CFG).to(dev).eval()
    model.backbone.compute_dtype = torch.bfloat16
    for sizes in ([100000], [100000] * 8):
        n = sum(sizes)
        off = torch.tensor([100000 * (i + 1) for i in range(len(sizes))], device=dev)
        feat = torch.randn(n, 64, device=dev).to(torch.bfloat16)
        with torch.no_grad():
            head_ms = _time(lambda: regress(model.reg_head, feat, off, False), args.steps, args.warmup)
        data = {k: v.to(dev) for k, v in S.make_batch(sizes, in_channels=4, extent=None, seed=7).items()}

        def whole():
            torch.manual_seed(9)
            with torch.no_grad():
                model(dict(data))

        def backbone():
            torch.manual_seed(9)
            with torch.no_grad():
                model.backbone(dict(data))
        steps = max(5, args.steps // 5)
        model_ms = _time(whole, steps, 3)
        bb_ms = _time(backbone, steps, 3)
        print(json.dumps({"points": n, "scenes": len(sizes), "pool_head_us": round(head_ms * 1e3, 2),
                          "model_eval_ms": round(model_ms, 3), "backbone_ms": round(bb_ms, 3),
                          "head_share": round(model_ms / bb_ms - 1, 4)}), flush=True)


if __name__ == "__main__":
    main()
