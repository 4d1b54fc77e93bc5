"""Time forward + backward of LovaszLoss and FocalLoss on the HIP path (csrc/seg_loss.hip) and with use_hip = False (the
torch composition of the same function, losses/lovasz.py / losses/misc.py) at (N, C) = (100k, 2), (100k, 13), (100k, 200),
and one training step (forward + backward) of PIGSEG_PTV3_CFG on 8 x 12 000 points both ways.  The two variants of a
shape are timed in the same process, alternating in blocks, after a warm-up of each; CUDA-event medians with the
10th - 90th percentile spread; one JSON line per shape.  Both variants' losses and gradients are compared first.
usage: python tools/bench_seg_loss.py [--steps 30] [--warmup 5] [--no-model]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402


def _time_pair(fns, steps, warmup, rounds=3):
    """Per function (median, p10, p90) in microseconds; the functions alternate in `rounds` blocks of steps / rounds."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = [[] for _ in fns]
    per = max(1, steps // rounds)
    for _ in range(rounds):
        for k, fn in enumerate(fns):
            for _ in range(per):
                start.record()
                fn()
                end.record()
                end.synchronize()
                ms[k].append(start.elapsed_time(end))
    out = []
    for m in ms:
        m.sort()
        out.append([round(m[i] * 1e3, 1) for i in (len(m) // 2, len(m) // 10, len(m) - 1 - len(m) // 10)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_seg_loss.py measures on the GPU only"
    from pointcept.models.losses import FocalLoss, LovaszLoss
    dev = torch.device("cuda:0")
    for n, c in ((100000, 2), (100000, 13), (100000, 200)):
        g = torch.Generator().manual_seed(c)
        logits = (torch.randn(n, c, generator=g) * 2).to(dev)
        present = min(c, 30)
        labels = torch.randperm(c, generator=g)[:present][torch.randint(0, present, (n,), generator=g)]
        labels[torch.rand(n, generator=g) < 0.1] = -1
        labels = labels.to(dev)
        res = {"points": n, "classes": c}
        for name, make in (("lovasz", lambda: LovaszLoss(mode="multiclass", loss_weight=3.0, ignore_index=-1)),
                           ("focal", lambda: FocalLoss(gamma=2.0, alpha=[0.1, 0.9] if c == 2 else 0.25, ignore_index=-1))):
            hip, comp = make(), make()
            comp.use_hip = False
            xs = [logits.clone().requires_grad_(True) for _ in range(2)]

            def step(module, x):
                x.grad = None
                loss = module(x, labels)
                loss.backward()
                return loss
            lh, lc = step(hip, xs[0]).item(), step(comp, xs[1]).item()
            gdiff = (xs[0].grad - xs[1].grad).abs().max().item() / xs[1].grad.abs().max().item()
            th, tc = _time_pair([lambda: step(hip, xs[0]), lambda: step(comp, xs[1])], args.steps, args.warmup)
            res[name] = {"hip_us": th, "composition_us": tc, "speedup": round(tc[0] / th[0], 2),
                         "loss_hip": lh, "loss_composition": lc, "grad_rel_diff": gdiff}
        print(json.dumps(res), flush=True)
    if args.no_model:
        return
    import ptv3_scenes as S
    from pointcept.models import build_model
    from ptv3_hip.configs import PIGSEG_PTV3_CFG
    torch.manual_seed(0)
    model = build_model(PIGSEG_PTV3_CFG).to(dev).train()
    data = {k: v.to(dev) for k, v in S.make_batch([12000] * 8, in_channels=4, extent=128, seed=1).items()}
    n = data["coord"].shape[0]
    g = torch.Generator().manual_seed(2)
    segment = torch.randint(0, 2, (n,), generator=g)
    segment[torch.rand(n, generator=g) < 0.05] = -1
    data["segment"] = segment.to(dev)

    def train_step(use_hip):
        for m in model.criteria.criteria:
            m.use_hip = use_hip
        model.zero_grad(set_to_none=True)
        torch.manual_seed(3)
        loss = model(dict(data))["loss"]
        loss.backward()
        return loss
    lh, lc = train_step(True).item(), train_step(False).item()
    th, tc = _time_pair([lambda: train_step(True), lambda: train_step(False)], max(6, args.steps // 2), 3)
    print(json.dumps({"model": "PIGSEG_PTV3_CFG", "points": n, "scenes": 8, "train_step_hip_ms": [round(t / 1e3, 3) for t in th],
                      "train_step_composition_ms": [round(t / 1e3, 3) for t in tc], "loss_hip": lh,
                      "loss_composition": lc}), flush=True)


if __name__ == "__main__":
    main()
