"""Time the evaluator kernels (csrc/evaluator.hip) against the same function composed in torch ON THE SAME GPU, and one
InsSegEvaluator scene end to end.  The torch composition is the baseline; the reference's CUDA path is not timed here.

  seg_confusion     N in {10 000, 100 000, 1 000 000} x K in {13, 20, 200}, from logits and from a prediction, without and
                    with an inverse 1.6 x longer.  Baseline: argmax, gather, masked write and three bincounts.
  insseg_associate  masks (P, 150 000) int32 about 1 % dense, P in {100, 400, 800}, and (100, 20 000); G in {30, 100},
                    without and with an idx 1.6 x longer (240 000 / 32 000; the kernel's time includes inverting it).
                    Two baselines: masks.ne(0).float() @ [one_hot(code), 1, void] on the matrix cores, and the
                    index_add_ form (ops.insseg_associate_torch).
  insseg_scene      InsSegEvaluator.eval() on one 20 000-point scene of PG_PTV3_SCANNET_CFG (the blobs of
                    tools/bench_pointgroup.py as its proposals), with the model's device results on and off.

Device events around `calls` calls, `windows` windows per path, the paths alternating; per path the median, the fastest
and the slowest window.  "ahead" is true when the kernel's SLOWEST window beats the FASTEST window of the best baseline:
the difference then exceeds the run-to-run spread seen in this very run.  Results are checked equal before timing.
usage: python tools/bench_evaluator.py [--windows 10] [--calls 10] [--only seg|ins|scene]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def event_ab(fns, windows, calls):
    """{path: {"median", "min", "max"}} in us per call: device events, windows alternating between the paths"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(calls):
                fn()
            end.record()
            end.synchronize()
            us[k].append(start.elapsed_time(end) / calls * 1e3)
    return {k: {"median": round(sorted(v)[len(v) // 2], 2), "min": round(min(v), 2), "max": round(max(v), 2)}
            for k, v in us.items()}


def verdict(us, kernel="kernel"):
    base = {k: v for k, v in us.items() if k != kernel}
    best = min(base, key=lambda k: base[k]["median"])
    return {"best_baseline": best, "speedup": round(base[best]["median"] / us[kernel]["median"], 2),
            "ahead": us[kernel]["max"] < base[best]["min"]}


def bench_seg_confusion(dev, windows, calls):
    from ptv3_hip import ops
    ignore = -1
    for n in (10_000, 100_000, 1_000_000):     # 10 000: where the wiring threshold of the hooks is drawn
        for k in (13, 20, 200):
            g = torch.Generator().manual_seed(n + k)
            logits = torch.randn(n, k, generator=g).to(dev)
            for with_inverse in (False, True):
                m = n * 8 // 5 if with_inverse else n
                inverse = torch.randint(0, n, (m,), generator=g).to(dev) if with_inverse else None
                target = torch.randint(-1, k, (m,), generator=g).to(dev)
                for form in ("logits", "pred"):
                    src = logits if form == "logits" else logits.max(1)[1]

                    def composed():
                        pred = src.max(1)[1] if form == "logits" else src
                        pred = pred[inverse] if inverse is not None else pred.clone()
                        pred.masked_fill_(target == ignore, ignore)

                        def hist(x):
                            return torch.bincount(torch.where((x >= 0) & (x < k), x, k), minlength=k + 1)[:k]

                        return torch.stack([hist(torch.where(pred == target, pred, -1)), hist(pred), hist(target)])

                    def kernel():
                        return ops.seg_confusion(src, target, k, ignore, inverse=inverse)

                    assert torch.equal(kernel(), composed())
                    us = event_ab({"kernel": kernel, "composed": composed}, windows, calls)
                    print(json.dumps({"what": "seg_confusion", "n": n, "k": k, "form": form, "m": m,
                                      "inverse": with_inverse, "us": us, **verdict(us)}), flush=True)


def bench_insseg_associate(dev, windows, calls):
    from ptv3_hip import ops
    # (20 000, 100): one voxelised scene with few proposals, where the wiring threshold of the hook is drawn
    for nm, p in ((20_000, 100), (150_000, 100), (150_000, 400), (150_000, 800)):
        g = torch.Generator().manual_seed(p)
        masks = (torch.rand(p, nm, generator=g) < 0.01).int().to(dev)
        for gt in (30, 100):
            for with_idx in (False, True):
                n = nm * 8 // 5 if with_idx else nm
                idx = torch.randint(0, nm, (n,), generator=g).to(dev) if with_idx else None
                code = torch.randint(0, gt + 1, (n,), generator=g).int()
                code = torch.where(torch.rand(n, generator=g) < 0.2, code + ops.INSSEG_VOID, code).to(dev)

                def matmul():
                    on = masks.ne(0)
                    if idx is not None:
                        on = on[:, idx]
                    cols = torch.cat([F.one_hot((code & 0x7FFFFFFF).long(), gt + 1).float(),
                                      torch.ones(n, 1, device=dev), (code < 0).float()[:, None]], 1)
                    out = (on.float() @ cols).int()
                    return out[:, :gt + 1], out[:, gt + 1], out[:, gt + 2]

                def index_add():
                    return ops.insseg_associate_torch(masks, code, gt, idx)

                def kernel():
                    return ops.insseg_associate(masks, code, gt, idx)

                want = kernel()
                for other in (matmul(), index_add()):
                    assert all(torch.equal(a, b) for a, b in zip(want, other))
                us = event_ab({"kernel": kernel, "matmul": matmul, "index_add": index_add}, windows, max(calls // 2, 1))
                print(json.dumps({"what": "insseg_associate", "p": p, "nm": nm, "g": gt, "idx": n if with_idx else 0,
                                  "us": us, **verdict(us)}), flush=True)


def bench_insseg_scene(dev, reps):
    """Wall clock around hook.eval() closed by a synchronisation: forward, association, the host copy, the matching."""
    import types
    import ptv3_scenes as S
    from bench_pointgroup import blobs, _offsets0, RADIUS, MIN_POINTS, PROPOSE
    from pointcept.models import build_model
    from pointcept.engines.hooks.builder import HOOKS
    import pointcept.engines.hooks  # noqa: F401
    from ptv3_hip import ops
    from ptv3_hip.configs import PG_PTV3_SCANNET_CFG
    n = 20000
    torch.manual_seed(0)
    model = build_model(PG_PTV3_SCANNET_CFG).to(dev).eval()
    data = {k: v.to(dev) for k, v in S.make_batch([n], in_channels=6, extent=None, seed=7).items()}
    data["instance_centroid"] = data["coord"].clone()
    center, prob, offset = blobs([n], dev)
    seg = prob.argmax(1)
    cell = torch.round(center / 8.0).long()
    data["segment"] = seg
    data["instance"] = torch.unique(cell[:, 0] * 10000 + cell[:, 1] * 100 + cell[:, 2], return_inverse=True)[1]

    def tail(*a):   # the blobs stand in for the model's own predictions (random weights predict no clusters)
        idxs, offs, large = ops.pg_cluster(center, seg.int(), _offsets0(offset), RADIUS, MIN_POINTS, PROPOSE)
        out = dict(zip(("pred_classes", "pred_scores", "pred_masks"), ops.pg_proposals(idxs, offs, prob, seg, PROPOSE,
                                                                                       large)))
        return out if model._device_results else {k: v.cpu() for k, v in out.items()}

    model._proposals = tail

    class HostResults:   # the same model to a hook that cannot switch it: CPU results, as the reference returns them
        def eval(self):
            return self

        def __call__(self, d):
            return model(d)

    hook = HOOKS.build(dict(type="InsSegEvaluator", segment_ignore_index=(-1, 0, 1), instance_ignore_index=-1))
    ms, proposals = {"device_results": [], "host_results": []}, None
    for rep in range(reps + 2):     # two warm-up repetitions; the two variants alternate
        for name, m in (("device_results", model), ("host_results", HostResults())):
            hook.trainer = types.SimpleNamespace(
                val_loader=[dict(data, name=["scene"])], model=m, logger=types.SimpleNamespace(info=lambda s: None),
                writer=None, epoch=0, comm_info={}, cfg=types.SimpleNamespace(evaluate=True, enable_wandb=False,
                data=types.SimpleNamespace(num_classes=20, ignore_index=-1, names=[f"c{i}" for i in range(20)])))
            hook.before_train()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hook.eval()
            torch.cuda.synchronize()
            if rep >= 2:
                ms[name].append((time.perf_counter() - t0) * 1e3)
            proposals = int(hook.scenes["scene"]["vert_count"].shape[0])
    for name, v in ms.items():
        v = sorted(v)
        print(json.dumps({"what": "insseg_scene", "results": name, "points": n, "proposals": proposals,
                          "median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3)}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=("seg", "ins", "scene"), default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timings come from the GPU; there is nothing to fall back to"
    dev = torch.device("cuda:0")
    if args.only in (None, "seg"):
        bench_seg_confusion(dev, args.windows, args.calls)
    if args.only in (None, "ins"):
        bench_insseg_associate(dev, args.windows, args.calls)
    if args.only in (None, "scene"):
        bench_insseg_scene(dev, args.reps)


if __name__ == "__main__":
    main()
