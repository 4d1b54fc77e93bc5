"""Time the Sonata self-distillation loss of one pairing (csrc/sonata_loss.hip through ptv3_hip.autograd.sonata_loss) against
the composed path of this library (pointcept/models/sonata: sonata_loss_torch, the same scaling form in torch), both in
one process, windows alternating, median and minimum of `--windows` windows of at least `--calls` calls and at least 30 ms
each:
  loss fwd        three Sinkhorn-Knopp sweeps and the cross entropy
  loss fwd+bwd    and the gradient of the student logits
and each kernel on its own, with the bytes it has to read and write and the rate that makes:
  sk_pass first / sk_pass next   one sweep (M K logits read, gathered), without and with u
  ce_fwd                         2 M K logits read
  ce_bwd                         2 M K logits read, Ns K gradient written
at K = 4096 prototypes (`--protos`, a list) and M in {20 000, 100 000} pairs, fp32 and bf16 logits; the student has
1.25 M rows in 8 scenes, the teacher M rows of which the match index repeats some.  Prints one JSON line per measurement.
The reference's own CUDA run is not timed here.
usage: python tools/bench_sonata.py [--windows 7] [--calls 3] [--pairs 20000,100000] [--protos 4096,2048] [--dtypes fp32,bf16]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402

MIN_WINDOW_MS = 30.0
T, TAU = 0.04, 0.1


def _window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def _ab(fns, windows, calls, warmup=2):
    """ms per call of the callables, windows alternating: (median, min, calls per window) of each"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--pairs", default="20000,100000")
    ap.add_argument("--protos", default="4096")
    ap.add_argument("--dtypes", default="fp32,bf16")
    args = ap.parse_args()
    from pointcept.models.sonata import sonata_v1m1_base as M
    from ptv3_hip import ops
    from ptv3_hip import autograd as A
    dev = torch.device("cuda:0")
    unit = lambda rows, c=64: torch.nn.functional.normalize(torch.randn(rows, c, device=dev), dim=1)  # noqa: E731

    def report(what, k, m, dtype, res, bytes_):
        f, co = res["fused"], res.get("composed")
        line = {"what": what, "K": k, "M": m, "dtype": dtype, "fused_ms": round(f[0], 4), "fused_min_ms": round(f[1], 4),
                "fused_calls": f[2]}
        if co is not None:
            line.update(composed_ms=round(co[0], 4), composed_min_ms=round(co[1], 4), composed_calls=co[2],
                        speedup=round(co[0] / f[0], 3))
        if bytes_:
            line.update(kernel_bytes=int(bytes_), fused_GBps=round(bytes_ / f[0] / 1e6, 1))
        print(json.dumps(line), flush=True)

    for k, name in [(int(v), n) for v in args.protos.split(",") for n in args.dtypes.split(",")]:
        dtype = dict(fp32=torch.float32, bf16=torch.bfloat16)[name]
        size = 4 if dtype == torch.float32 else 2
        for m in [int(v) for v in args.pairs.split(",")]:
            torch.manual_seed(0)
            ns = m + m // 4
            x = (unit(m) @ unit(k).t()).to(dtype)
            s = (unit(ns) @ unit(k).t()).to(dtype)
            idx_t = torch.randint(0, m, (m,), device=dev)
            idx_s = torch.randperm(ns, device=dev)[:m].sort()[0]
            offset = torch.tensor([ns * (i + 1) // 8 for i in range(8)], device=dev)
            sg = s.clone().requires_grad_(True)
            row = m * k * size

            def fwd(fn):
                with torch.no_grad():
                    fn(s, x, idx_t, idx_s, offset, T, TAU)

            def fwd_bwd(fn):
                sg.grad = None
                fn(sg, x, idx_t, idx_s, offset, T, TAU).backward()

            res = _ab({"fused": lambda: fwd(A.sonata_loss), "composed": lambda: fwd(M.sonata_loss_torch)},
                      args.windows, args.calls)
            report("loss fwd", k, m, name, res, 5 * row)
            res = _ab({"fused": lambda: fwd_bwd(A.sonata_loss), "composed": lambda: fwd_bwd(M.sonata_loss_torch)},
                      args.windows, args.calls)
            report("loss fwd+bwd", k, m, name, res, 7 * row + ns * k * size)

            u = A.sonata_scaling(x, idx_t, 1.0 / T)
            loss, d, lse, gscale = ops.sonata_ce(x, idx_t, 1.0 / T, u, s, idx_s, 1.0 / TAU, offset)
            dloss = torch.ones(1, device=dev)
            for what, fn, bytes_ in (
                    ("sk_pass first", lambda: ops.sonata_sk_pass(x, idx_t, 1.0 / T), row),
                    ("sk_pass next", lambda: ops.sonata_sk_pass(x, idx_t, 1.0 / T, u, m), row),
                    ("ce_fwd", lambda: ops.sonata_ce(x, idx_t, 1.0 / T, u, s, idx_s, 1.0 / TAU, offset), 2 * row),
                    ("ce_bwd", lambda: ops.sonata_ce_bwd(dloss, x, idx_t, 1.0 / T, u, s, idx_s, 1.0 / TAU, offset, d, lse,
                                                         gscale), 2 * row + ns * k * size)):
                report(what, k, m, name, _ab({"fused": fn}, args.windows, args.calls), bytes_)
            del x, s, sg
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
