"""Time the kernels of the context-aware classifier head (csrc/cac.hip) against the composed path of this library
(`set_fused(False)`: the torch functions of pointcept/models/context_aware_classifier), both in one process, windows
alternating, median and minimum of `--windows` windows of at least `--calls` calls and at least 30 ms each:
  proto_softmax / proto_label   forward, and forward + backward (gradient of the features)
  cos_logits                    forward, per scene and shared prototypes
  distill                       forward, and forward + backward (gradient of the refined logits)
  head_eval                     seg_head + the eval tail of CACSegmentor.head on given features
  head_train                    the training head, forward + backward down to the gradient of the features
                                (criteria: CrossEntropyLoss alone, so that the head is what is timed)
at the six (K, C) of the semseg-cac-v1m1 configs - C = 96 (SpUNet) / 48 (PT-v2m2), K = 20 / 100 / 200 - on `--scenes`
scenes of `--points` points.  Prints one JSON line per measurement, with the bytes and multiply-adds each kernel needs.
The reference's own CUDA run is not timed here.
usage: python tools/bench_cac.py [--scenes 12] [--points 100000] [--windows 9] [--calls 5] [--only 200x96]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402

SHAPES = [(20, 96), (100, 96), (200, 96), (20, 48), (100, 48), (200, 48)]
TINY_BACKBONE = dict(type="SpUNet-v1m1", in_channels=4, num_classes=0, base_channels=16,
                     channels=(16, 32, 32, 64, 64, 32, 16, 16), layers=(1, 2, 1, 1, 1, 1, 2, 1))


def _window(fn, calls):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


MIN_WINDOW_MS = 30.0


def _ab(fused, composed, windows, calls, warmup=2):
    """ms per call of the two callables, windows alternating: (median, min, calls per window) of each.  A window holds
    at least `calls` calls and at least MIN_WINDOW_MS of work (sized from one timed call after the warm-up), so that a
    0.3 ms kernel is not timed over a millisecond."""
    fns = {"fused": fused, "composed": composed}
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
    ap.add_argument("--scenes", type=int, default=12)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    from pointcept.models import build_model
    from pointcept.models.context_aware_classifier import context_aware_classifier_v1m1_base as M
    from ptv3_hip import ops
    from ptv3_hip import autograd as A
    dev = torch.device("cuda:0")
    b, n = args.scenes, args.scenes * args.points
    ends = [args.points * (i + 1) for i in range(b)]
    cuts = list(zip([0] + ends[:-1], ends))
    offset = torch.tensor(ends, device=dev)

    def report(what, k, c, res, bytes_, fma):
        f, co = res["fused"], res["composed"]
        print(json.dumps({"what": what, "K": k, "C": c, "scenes": b, "points": n, "fused_ms": round(f[0], 4),
                          "composed_ms": round(co[0], 4), "fused_min_ms": round(f[1], 4),
                          "composed_min_ms": round(co[1], 4), "speedup": round(co[0] / f[0], 3),
                          "fused_calls": f[2], "composed_calls": co[2],
                          "kernel_bytes": int(bytes_), "kernel_fma": int(fma),
                          "fused_GBps": round(bytes_ / f[0] / 1e6, 1), "fused_TFMAps": round(fma / f[0] / 1e9, 3)}),
              flush=True)

    for k, c in SHAPES:
        if args.only and args.only != f"{k}x{c}":
            continue
        torch.manual_seed(0)
        x = torch.randn(n, c, device=dev)
        logits = torch.randn(n, k, device=dev) * 3.0
        labels = torch.randint(-1, k, (n,), device=dev)
        dproto = torch.randn(b, k, c, device=dev)
        xg = x.clone().requires_grad_(True)
        nk, nc = 4 * n * k, 4 * n * c

        # ---- prototypes, softmax form --------------------------------------------------------------------------
        def comp_softmax(inp):
            return torch.stack([M.softmax_proto_torch(inp[s:e], logits[s:e], 0.75) for s, e in cuts])

        def fb(fn, inp, seed):
            inp.grad = None
            (fn(inp) * seed).sum().backward()

        with torch.no_grad():
            res = _ab(lambda: ops.cac_proto(x, logits=logits, offset=offset, conf_thresh=0.75),
                      lambda: comp_softmax(x), args.windows, args.calls)
        report("proto_softmax fwd", k, c, res, nk + nc, n * k * (c + 1))
        res = _ab(lambda: fb(lambda t: A.cac_proto_softmax(t, logits, offset, 0.75)[0], xg, dproto),
                  lambda: fb(comp_softmax, xg, dproto), args.windows, args.calls)
        report("proto_softmax fwd+bwd", k, c, res, 2 * nk + 2 * nc, n * k * (2 * c + 1))

        # ---- prototypes, label form ----------------------------------------------------------------------------
        with torch.no_grad():
            res = _ab(lambda: ops.cac_proto(x, labels=labels, num_classes=k),
                      lambda: M.label_proto_torch(x, labels, k), args.windows, args.calls)
        report("proto_label fwd", k, c, res, 8 * n + nc, n * k * (c + 1))
        res = _ab(lambda: fb(lambda t: A.cac_proto_label(t, labels, k)[0], xg, dproto[0]),
                  lambda: fb(lambda t: M.label_proto_torch(t, labels, k)[0], xg, dproto[0]), args.windows, args.calls)
        report("proto_label fwd+bwd", k, c, res, 16 * n + 2 * nc, n * k * (2 * c + 1))

        # ---- cosine logits -------------------------------------------------------------------------------------
        q = torch.randn(b, k, c, device=dev)
        with torch.no_grad():
            res = _ab(lambda: ops.cac_cos_logits(x, q, offset, 15.0),
                      lambda: torch.cat([M.get_pred(x[s:e], q[i]) for i, (s, e) in enumerate(cuts)]) * 15,
                      args.windows, args.calls)
            report("cos_logits per scene", k, c, res, nk + nc, n * k * c)
            res = _ab(lambda: ops.cac_cos_logits(x, q[0].contiguous(), None, 15.0),
                      lambda: M.get_pred(x, q[0]) * 15, args.windows, args.calls)
            report("cos_logits shared", k, c, res, nk + nc, n * k * c)

        # ---- distillation loss ---------------------------------------------------------------------------------
        soft = torch.randn(n, k, device=dev) * 3.0
        pg = logits.clone().requires_grad_(True)
        with torch.no_grad():
            res = _ab(lambda: ops.cac_distill(logits, soft, labels),
                      lambda: M.distill_loss_torch(logits, soft, labels), args.windows, args.calls)
        report("distill fwd", k, c, res, 2 * nk + 8 * n, 0)

        def dist(fn):
            pg.grad = None
            fn(pg, soft, labels).backward()

        res = _ab(lambda: dist(A.cac_distill), lambda: dist(M.distill_loss_torch), args.windows, args.calls)
        report("distill fwd+bwd", k, c, res, 5 * nk + 16 * n, 0)
        del soft, pg, q

        # ---- the head ------------------------------------------------------------------------------------------
        model = build_model(dict(type="CAC-v1m1", num_classes=k, backbone_out_channels=c, backbone=TINY_BACKBONE,
                                 criteria=[dict(type="CrossEntropyLoss", loss_weight=1.0, ignore_index=-1)],
                                 conf_thresh=0.75, detach_pre_logits=True)).to(dev)
        with torch.no_grad():
            model.seg_head.weight.mul_(8.0)
        data = dict(offset=offset, segment=labels)

        def head_eval(fused):
            model.set_fused(fused)
            with torch.no_grad():
                model.head(x, dict(offset=offset))

        def head_train(fused):
            model.set_fused(fused)
            xg.grad = None
            model.head(xg, data)["loss"].backward()

        model.eval()
        res = _ab(lambda: head_eval(True), lambda: head_eval(False), args.windows, args.calls)
        report("head_eval", k, c, res, 0, 0)
        model.train()
        res = _ab(lambda: head_train(True), lambda: head_train(False), args.windows, max(1, args.calls // 2))
        report("head_train fwd+bwd", k, c, res, 0, 0)
        del model, x, xg, logits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
