"""Time the batch head of DefaultClassifier / PigBodyRegressor (fork config: C = 64, widths 256 / 128 / 7, bf16 features)
against its composition from the per-layer entry points (`set_fused(False)`), both in one process, alternating, median of
`--windows` windows of `--calls` calls each:
  eval   pooling + head + L1 loss + the seven column errors on given features
  train  the head in training mode on pooled rows, forward + backward down to the gradient of the pooled rows
  step   a whole training step (forward + backward) of PIG_WEIGHT_PTV3_CFG
at B x 20 000 points for B in 4, 8, 32 (step: B = 8 only), and eval at 1 x 100 000.  Prints one JSON line per
measurement.  `--eval-only` runs the fused eval head alone (for a kernel trace).
usage: python tools/bench_cls_head.py [--windows 12] [--calls 20] [--eval-only] [--no-step]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402


def _window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def _ab(model, fn, windows, calls, warmup=3):
    """median ms per call of fn() with the fused head and with the composed one, windows alternating"""
    ms = {True: [], False: []}
    for fused in (True, False):
        model.set_fused(fused)
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    for _ in range(windows):
        for fused in (True, False):
            model.set_fused(fused)
            ms[fused].append(_window(fn, calls))
    model.set_fused(True)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    return med[True], med[False], min(ms[True]), min(ms[False])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--eval-only", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    import ptv3_scenes as S
    from pointcept.models import build_model
    from ptv3_hip.configs import PIG_WEIGHT_PTV3_CFG
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(PIG_WEIGHT_PTV3_CFG).to(dev)
    model.backbone.compute_dtype = torch.bfloat16
    # the model composes above fused_eval_max_scenes: lift the cap, so that "fused" is the fused kernel at every size
    model.fused_eval_max_scenes = 1 << 30

    def report(what, sizes, res):
        f, c, fmin, cmin = res
        print(json.dumps({"what": what, "scenes": len(sizes), "points": sum(sizes), "fused_us": round(f * 1e3, 2),
                          "composed_us": round(c * 1e3, 2), "fused_min_us": round(fmin * 1e3, 2),
                          "composed_min_us": round(cmin * 1e3, 2), "speedup": round(c / f, 3)}), flush=True)

    for sizes in ([20000] * 4, [20000] * 8, [20000] * 32, [100000]):
        b, n = len(sizes), sum(sizes)
        off = torch.tensor([sum(sizes[:i + 1]) for i in range(b)], device=dev)
        feat = torch.randn(n, 64, device=dev).to(torch.bfloat16)
        batch = {"category": torch.rand(b, 7, device=dev) + 0.3}

        def head_eval():
            with torch.no_grad():
                logits, loss, stats = model._head(feat, off, batch)
                if stats is None:   # the composed path: the errors as PigBodyRegressor forms them
                    (logits.view(-1, 7) * 100.0 - batch["category"].view(-1, 7) * 100.0).abs().mean(dim=0)

        model.eval()
        if args.eval_only:
            for _ in range(args.calls):
                head_eval()
            torch.cuda.synchronize()
            continue
        report("eval", sizes, _ab(model, head_eval, args.windows, args.calls))
        if b == 1:
            continue
        pooled = torch.randn(b, 64, device=dev).requires_grad_(True)   # the head starts from the pooled rows

        def head_train():
            pooled.grad = None
            logits, loss, stats = model._head(pooled, None, batch)
            if stats is None:
                with torch.no_grad():
                    (logits.detach().view(-1, 7) * 100.0 - batch["category"].view(-1, 7) * 100.0).abs().mean(dim=0)
            loss.backward()

        model.train()
        report("train", sizes, _ab(model, head_train, args.windows, args.calls))
    if args.eval_only or args.no_step:
        return
    sizes = [20000] * 8
    data = {k: v.to(dev) for k, v in S.make_batch(sizes, in_channels=4, extent=None, seed=7).items()}
    data["category"] = torch.rand(len(sizes), 7, device=dev) + 0.3

    def step():
        model.zero_grad(set_to_none=True)
        torch.manual_seed(9)
        model(dict(data))["loss"].backward()

    model.train()
    report("step", sizes, _ab(model, step, args.windows, 1, warmup=2))


if __name__ == "__main__":
    main()
