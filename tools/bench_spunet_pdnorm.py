"""Time the one-launch modulation of SpUNet-v1m3's PDBatchNorms (csrc/pdnorm.hip) against the per-layer composition from
ops that predate it (SiLU, the M = 1 GEMM of the library's Linear, the element-wise products), with HIP events: medians of
--steps windows after --warmup, the two paths timed alternately.  One JSON line per measurement.
  (a) kernels alone, at the 59 layers of PPT_SPUNET_SCANNET_CFG's backbone (Cc = 256, 17.6 MB of modulation weights) and at
      the 33 of SPUNET_PDNORM_TINY_CFG (Cc = 24): the taped forward, forward + backward, the backward alone (over a retained
      graph) and the eval fold with its cache emptied before every call.  Every figure is the time of a CALL issued from
      Python - launch and host overhead included - not of the kernels alone, and the `*_call_gbs` fields divide bytes by
      that time (the modulation weights once per forward or fold; read once and written once for the backward): they
      are a lower bound of what the kernels reach, which is not measured here.
  (b) PPT_SPUNET_SCANNET_CFG at 8 x 20 000 sites, each with set_modulation(True) against set_modulation(False): the eval
      forward with the modulation caches emptied ("first"; the conv weight caches stay filled, so the difference is the
      modulation's alone), the steady eval forward (both paths read their cache: expected equal), one training step
      (forward, backward, FusedAdamW); and the steady eval forward next to SpUNet-v1m1 of the same widths.
  (c) device kernels launched by one training step and by one "first" eval forward on either path (torch.profiler;
      "not measured" if the profiler gives no device events).
Nothing here reads a reference tree.  Not measured: bf16 / autocast, other batch shapes, multi-GPU.
usage: python tools/bench_spunet_pdnorm.py [--steps 20] [--warmup 3] [--skip-model]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402

INNER = 10          # calls per timed window of the kernels-alone measurements
FP32_TOL = 1e-4


def _time_pair(fa, fb, steps, warmup, inner):
    """medians (ms per call) of fa and fb, timed alternately; a window holds `inner` back-to-back calls between two
    events and one synchronise"""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = ([], [])
    for _ in range(steps):
        for k, fn in enumerate((fa, fb)):
            start.record()
            for _ in range(inner):
                fn()
            end.record()
            end.synchronize()
            ms[k].append(start.elapsed_time(end) / inner)
    return [sorted(v)[len(v) // 2] for v in ms]


def _emit(**kw):
    print(json.dumps({k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in kw.items()}), flush=True)


def _same(what, a, b):
    diff, scale = (a - b).abs().max().item(), b.abs().max().item()
    if not diff <= FP32_TOL * max(scale, 1.0):
        raise AssertionError(f"{what}: outputs differ by {diff:.3e} at scale {scale:.3e}")
    return diff


def bench_kernels(name, cfg, condition, steps, warmup, dev):
    from pointcept.models import build_model
    from pointcept.models.sparse_unet.spconv_unet_v1m3_pdnorm import Prompt
    torch.manual_seed(0)
    bb = build_model(cfg).to(dev)
    for m in bb.pdnorms():      # a zero modulation would hide nothing from the clock, but would from the comparison
        torch.nn.init.normal_(m.modulation[1].weight, std=0.05)
    pds = bb.pdnorms()
    cc = bb.context_channels
    context = torch.randn(1, cc, device=dev, requires_grad=True)
    weights = sum(m.modulation[1].weight.numel() for m in pds) * 4
    total = sum(m.num_features for m in pds)
    grads = [torch.randn(m.num_features, device=dev) for m in pds]

    def one_fwd():
        return bb.modulation_pairs(condition, context)

    def per_fwd():
        return [m.pair(m.active(condition), context) for m in pds]

    inputs = [context]
    for m in pds:
        bn = m.active(condition)
        inputs += [p for p in (m.modulation[1].weight, m.modulation[1].bias, bn.weight, bn.bias) if p is not None]
    last = {}

    def with_bwd(fwd):
        def run():      # autograd.grad: no accumulate-add into .grad on either path
            pairs = fwd()
            outs = [t for p in zip(*pairs) for t in p]
            last["dcontext"] = torch.autograd.grad(outs, inputs, grads + grads)[0]
        return run

    bb.train()
    a, b = _time_pair(one_fwd, per_fwd, steps, warmup, INNER)
    diff = max(_same("pair", x, y) for p, q in zip(one_fwd(), per_fwd()) for x, y in zip(p, q))
    _emit(op="modulation forward (taped)", model=name, layers=len(pds), channels=total, cc=cc, weight_mb=weights / 1e6,
          one_launch_ms=a, per_layer_ms=b, speedup=b / a, one_launch_call_gbs=weights / a / 1e6, max_abs_diff=diff)
    c, d = _time_pair(with_bwd(one_fwd), with_bwd(per_fwd), steps, warmup, INNER)
    with_bwd(one_fwd)()
    g1 = last["dcontext"].clone()
    with_bwd(per_fwd)()
    _emit(op="modulation forward + backward", model=name, layers=len(pds), one_launch_ms=c, per_layer_ms=d,
          speedup=d / c, max_abs_diff_dcontext=_same("dcontext", g1, last["dcontext"]))

    def bwd_only(fwd):
        outs = [t for p in zip(*fwd()) for t in p]
        return lambda: torch.autograd.grad(outs, inputs, grads + grads, retain_graph=True)
    g, h = _time_pair(bwd_only(one_fwd), bwd_only(per_fwd), steps, warmup, INNER)
    _emit(op="modulation backward alone (retained graph)", model=name, layers=len(pds), one_launch_ms=g, per_layer_ms=h,
          speedup=h / g, one_launch_call_gbs=2 * weights / g / 1e6)

    bb.eval()
    ctx = context.detach()

    def one_fold():
        bb.forget_modulation()
        with torch.no_grad():
            return bb.modulation_folds(condition, ctx)

    def per_fold():
        bb.forget_modulation()
        with torch.no_grad():
            return [m.folded(Prompt(condition, ctx)) for m in pds]
    e, f = _time_pair(one_fold, per_fold, steps, warmup, INNER)
    diff = max(_same("fold", x, y) for p, q in zip(one_fold(), per_fold()) for x, y in zip(p, q))
    _emit(op="eval fold, cache emptied", model=name, layers=len(pds), one_launch_ms=e, per_layer_ms=f, speedup=f / e,
          one_launch_call_gbs=weights / e / 1e6, max_abs_diff=diff)


def _kernel_count(fn):
    """device kernels launched by fn(), or None where the profiler records no device events"""
    try:
        from torch.profiler import profile, ProfilerActivity
        from torch.autograd import DeviceType
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for ev in prof.events() if ev.device_type == DeviceType.CUDA)
        return n or None
    except Exception as exc:      # the profiler is not what is measured here
        print(f"# kernel count not measured: {type(exc).__name__}: {exc}", file=sys.stderr)
        return None


def bench_model(steps, warmup, dev):
    import ptv3_scenes as S
    from pointcept.models import build_model
    from ptv3_hip.configs import PPT_SPUNET_SCANNET_CFG
    from ptv3_hip.optim import FusedAdamW
    torch.manual_seed(0)
    model = build_model(PPT_SPUNET_SCANNET_CFG)
    model.set_class_embedding(torch.randn(tuple(model.class_embedding.shape)))
    model = model.to(dev)
    bb = model.backbone
    data = S.make_batch([20000] * 8, in_channels=6, extent=None, seed=7)
    data = {k: v.to(dev) for k, v in data.items() if k in ("grid_coord", "feat", "offset", "coord")}
    n = data["feat"].shape[0]
    data["segment"] = torch.randint(0, 20, (n,), device=dev)
    data["condition"] = ["ScanNet"]
    bare = {k: v for k, v in data.items() if k != "segment"}
    forget = bb.forget_modulation

    def evaluate(mode, first):
        def run():
            bb.set_modulation(mode)
            if first:
                forget()
            with torch.no_grad():
                return model(dict(bare))["seg_logits"]
        return run
    model.eval()
    a, b = _time_pair(evaluate(True, True), evaluate(False, True), steps, warmup, 1)
    c, d = _time_pair(evaluate(True, False), evaluate(False, False), steps, warmup, 1)
    diff = _same("seg_logits", evaluate(True, True)(), evaluate(False, True)())
    _emit(op="PPT-v1m1 / SpUNet-v1m3 eval forward", scenes=8, scene_sites=20000, first_one_launch_ms=a,
          first_per_layer_ms=b, first_speedup=b / a, steady_one_launch_ms=c, steady_per_layer_ms=d, max_abs_diff=diff)

    v1m1 = build_model(dict(type="SpUNet-v1m1", in_channels=6, num_classes=0)).to(dev).eval()

    def plain():
        with torch.no_grad():
            return v1m1(dict(bare))

    def backbone_only():
        bb.set_modulation(None)
        ctx = model.embedding_table.weight[1:2].detach()
        with torch.no_grad():
            return bb(dict(bare, context=ctx, context_source=model.embedding_table.weight))
    e, f = _time_pair(backbone_only, plain, steps, warmup, 1)
    _emit(op="steady eval forward, backbone alone", scenes=8, scene_sites=20000, spunet_v1m3_ms=e, spunet_v1m1_ms=f,
          ratio=e / f)

    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=0.01)

    def step(mode):
        def run():
            bb.set_modulation(mode)
            model.train()
            opt.zero_grad(set_to_none=True)
            out = model(dict(data))
            out["loss"].backward()
            opt.step()
            return out["loss"]
        return run
    g, h = _time_pair(step(True), step(False), max(steps // 2, 5), warmup, 1)
    _emit(op="PPT-v1m1 / SpUNet-v1m3 training step", scenes=8, scene_sites=20000, one_launch_ms=g, per_layer_ms=h,
          speedup=h / g, optimizer="FusedAdamW")

    model.eval()
    counts = dict(train_one_launch=_kernel_count(step(True)), train_per_layer=_kernel_count(step(False)))
    model.eval()
    counts.update(first_eval_one_launch=_kernel_count(evaluate(True, True)),
                  first_eval_per_layer=_kernel_count(evaluate(False, True)),
                  steady_eval=_kernel_count(evaluate(True, False)))
    _emit(op="device kernels per call", **{k: (v if v is not None else "not measured") for k, v in counts.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_spunet_pdnorm measures on the GPU only"
    dev = torch.device("cuda:0")
    from ptv3_hip.configs import PPT_SPUNET_SCANNET_CFG, SPUNET_PDNORM_TINY_CFG
    bench_kernels("default (59 layers)", PPT_SPUNET_SCANNET_CFG["backbone"], "ScanNet", args.steps, args.warmup, dev)
    bench_kernels("tiny (33 layers)", SPUNET_PDNORM_TINY_CFG, "B", args.steps, args.warmup, dev)
    if not args.skip_model:
        bench_model(args.steps, args.warmup, dev)


if __name__ == "__main__":
    main()
