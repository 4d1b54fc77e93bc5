"""Time the eval head of "PPT-v1m1" in its three forms, in one process, windows alternating, median and minimum of
`--windows` windows of at least `--calls` calls and at least 30 ms each:
  reference   the reference's statement order in torch: Linear(C -> D), row norm, division, product with the K valid
              class embeddings, scale (point_prompt_training_v1m1_language_guided.py:98-107)
  collapsed   the collapsed operands of ops.ppt_head_collapse composed in torch: x @ B + bias, row norm of the first C
              columns, one division
  kernel      ptv3_ppt_head_fwd (csrc/ppt_head.hip) on the same operands
for (K, C) in {13, 20, 25, 36, 200} x {64, 96} at D = 512 and 100 000 and 1 000 000 rows.  One JSON line per shape, with
the bytes and multiply-adds the kernel needs and the largest difference of the three results.
With --model it times instead one eval forward and one training step (forward, backward, fused AdamW) of
PPT_PTV3_SCANNET_CFG on `--scenes` scenes of `--points` points with the resolution of non-adaptive PDNorms to their
active plain norm (point_transformer_v3m1_base.RESOLVE_PDNORM) on and off, windows alternating.
The reference's own CUDA run is not timed here.
usage: python tools/bench_ppt.py [--windows 7] [--calls 2] [--only 20x64] [--rows 100000 1000000] [--model]
       [--scenes 8] [--points 12000]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402

KS, CS, ROWS, WIDTH = (13, 20, 25, 36, 200), (64, 96), (100000, 1000000), 512
MIN_WINDOW_MS = 30.0


def _window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def _alternate(fns, windows, calls, warmup=2):
    """ms per call of the callables, windows alternating: {name: (median, min, calls per window)}.  A window holds at
    least `calls` calls and at least MIN_WINDOW_MS of work (sized from one timed call after the warm-up)."""
    ms, per = {k: [] for k in fns}, {}
    for k, fn in fns.items():
        for _ in range(warmup):
            fn()
        per[k] = max(calls, int(MIN_WINDOW_MS / max(_window(fn, 1), 1e-3)) + 1)
    torch.cuda.synchronize()
    for _ in range(windows):
        for k, fn in fns.items():
            ms[k].append(_window(fn, per[k]))
    return {k: (sorted(v)[len(v) // 2], min(v), per[k]) for k, v in ms.items()}


def bench_head(args):
    from pointcept.models.point_prompt_training import point_prompt_training_v1m1_language_guided as M
    from ptv3_hip import ops
    dev = torch.device("cuda:0")
    for n in (args.rows or ROWS):
        for c in CS:
            for k in KS:
                if args.only and args.only != f"{k}x{c}":
                    continue
                g = torch.Generator().manual_seed(1000 * k + c)
                W = (torch.randn(WIDTH, c, generator=g) / c ** 0.5).to(dev)
                b = (0.1 * torch.randn(WIDTH, generator=g)).to(dev)
                E = torch.randn(k, WIDTH, generator=g)
                E = (E / E.norm(dim=1, keepdim=True)).to(dev)
                scale = torch.tensor(4.6052, device=dev)
                x = torch.randn(n, c, generator=g).to(dev)
                B, bias, beta, s = ops.ppt_head_collapse(W, b, E, scale)
                fns = {"reference": lambda: M.head_reference(x, W, b, E, scale),
                       "collapsed": lambda: M.head_collapsed(x, B, bias, beta, s),
                       "kernel": lambda: ops.ppt_head(x, B, bias, beta, s)}
                outs = {name: fn() for name, fn in fns.items()}
                diff = max((outs[a] - outs["reference"]).abs().max().item() for a in ("collapsed", "kernel"))
                res = _alternate(fns, args.windows, args.calls)
                bytes_ = 4 * (n * c + n * k + c * (c + k))
                fma = n * c * (c + k)
                line = {"what": "head", "K": k, "C": c, "D": WIDTH, "rows": n, "max_abs_diff": round(diff, 6),
                        "kernel_bytes": bytes_, "kernel_fma": fma}
                for name, (med, low, per) in res.items():
                    line.update({name + "_ms": round(med, 4), name + "_min_ms": round(low, 4), name + "_calls": per})
                line["kernel_GBps"] = round(bytes_ / res["kernel"][0] / 1e6, 1)
                line["kernel_TFMAps"] = round(fma / res["kernel"][0] / 1e9, 3)
                line["kernel_vs_best_composition"] = round(min(res["reference"][0], res["collapsed"][0]) / res["kernel"][0], 3)
                print(json.dumps(line), flush=True)


def bench_model(args):
    import ptv3_scenes as S
    from pointcept.models import build_model
    from pointcept.models.point_transformer_v3 import point_transformer_v3m1_base as V3
    from ptv3_hip.configs import PPT_PTV3_SCANNET_CFG
    from ptv3_hip.optim import FusedAdamW
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(PPT_PTV3_SCANNET_CFG)
    model.set_class_embedding(torch.randn(*model.class_embedding.shape))
    model = model.to(dev)
    batch = S.make_batch([args.points] * args.scenes, in_channels=6, extent=256, seed=1)
    data = {k: batch[k].to(dev) for k in ("grid_coord", "feat", "offset", "coord")}
    n = data["feat"].shape[0]
    data["segment"] = torch.randint(0, 20, (n,), generator=torch.Generator().manual_seed(2)).to(dev)
    data["condition"] = ["ScanNet"]
    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.05)

    def evaluate(resolve):
        def run():
            V3.RESOLVE_PDNORM = resolve
            with torch.no_grad():
                model(dict(data))
            V3.RESOLVE_PDNORM = True
        return run

    def train(resolve):
        def run():
            V3.RESOLVE_PDNORM = resolve
            model(dict(data))["loss"].backward()
            opt.step()
            opt.zero_grad(set_to_none=True)
            V3.RESOLVE_PDNORM = True
        return run

    for what, make in (("model_eval", evaluate), ("model_train_step", train)):
        model.train(what == "model_train_step")
        res = _alternate({"resolved": make(True), "generic": make(False)}, args.windows, args.calls)
        line = {"what": what, "scenes": args.scenes, "points": n}
        for name, (med, low, per) in res.items():
            line.update({name + "_ms": round(med, 3), name + "_min_ms": round(low, 3), name + "_calls": per})
        line["generic_over_resolved"] = round(res["generic"][0] / res["resolved"][0], 3)
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--only", default="")
    ap.add_argument("--rows", type=int, nargs="*", default=None)
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--points", type=int, default=12000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ppt.py needs the GPU"
    (bench_model if args.model else bench_head)(args)


if __name__ == "__main__":
    main()
