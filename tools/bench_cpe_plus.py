"""Time the bottleneck-CPE kernels of PT-v3m1-Plus with HIP events (median of --steps calls after --warmup) at the shapes
of every level of the fork config (configs/my_dataset/keypoint_ptv3_plus.py) on 8 x 20 000 and 1 x 100 000 sites, fp32
and bf16:
  * ptv3_subm_conv_ln (5^3, c = mid) beside its composition from the kernels that were there before it
    (ptv3_gemm with the neighbour table -> ptv3_layernorm -> ReLU), with the gathered GB/s: bytes of the x rows the
    present taps read, over the time;
  * ptv3_rows_linear_ln (C -> mid) beside ptv3_gemm -> ptv3_layernorm -> ReLU;
  * the KeypointPTv3Plus eval forward, fused beside set_fused(False), and one training step (forward + backward);
  * library calls issued per BlockPlus both ways (a library call is one launch except a split-K GEMM).
Outputs are compared at the timed sizes.  Prints one JSON line per measurement and appends it to --out.
usage: python tools/bench_cpe_plus.py [--steps 20] [--warmup 3] [--out profiles/ptv3_plus/bench_cpe_plus.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402

OUT = None


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


def _emit(**kw):
    line = json.dumps({k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in kw.items()})
    print(line, flush=True)
    if OUT is not None:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def _levels(model, data):
    """(name, C, mid, sparse tensor) of the first block of every encoder / decoder stage, from one eval forward."""
    from pointcept.models.keypoint_ptv3_plus import BlockPlus
    seen = []
    handles = []
    bb = model.backbone
    stages = [(f"enc{s}", st) for s, st in enumerate(bb.enc_stages)] + list(bb.dec.named_children())
    for name, stage in stages:
        first = next(m for m in stage.children() if isinstance(m, BlockPlus))
        handles.append(first.register_forward_pre_hook(
            lambda m, args, name=name: seen.append((name, m.channels, m.cpe[3].in_channels, args[0].sparse_conv_feat))))
    torch.manual_seed(1)
    with torch.no_grad():
        model(dict(data))
    for h in handles:
        h.remove()
    return seen


def bench_kernels(levels, scene, steps, warmup, dev):
    from ptv3_hip import ops
    eps = 1e-5
    for name, c_in, mid, spt in levels:
        nbr = spt.neighbors(5, "stage" + name[-1])
        m = nbr.shape[0]
        taps = int((nbr >= 0).sum().item())
        for dtype in (torch.float32, torch.bfloat16):
            esz = 4 if dtype == torch.float32 else 2
            torch.manual_seed(m % 1000 + mid)
            x = torch.randn(m, mid, device=dev).to(dtype)
            w = (torch.randn(mid, 125 * mid, device=dev) / (8 * mid) ** 0.5).to(dtype)
            bias, gamma, beta = (torch.randn(mid, device=dev) * s + o for s, o in ((0.1, 0), (0.1, 1), (0.1, 0)))

            def fused():
                return ops.subm_conv_ln(x, w, nbr, bias, gamma, beta, eps, ops.ACT_RELU, row_order=spt.row_order)

            def composed():
                y = ops.gemm(x, w, bias=bias, nbr=nbr, kvol=125, row_order=spt.row_order)
                return ops.affine_act(ops.layernorm(y, gamma, beta, eps), None, None, ops.ACT_RELU)
            a, b = _time(fused, steps, warmup), _time(composed, steps, warmup)
            _emit(op="subm_conv_ln", scene=scene, level=name, rows=m, c=mid, kvol=125, dtype=str(dtype)[6:],
                  present_taps_per_row=taps / m, fused_ms=a, composed_ms=b, speedup=b / a,
                  gathered_gbs_fused=taps * mid * esz / a / 1e6, gathered_gbs_composed=taps * mid * esz / b / 1e6,
                  max_abs_diff=(fused().float() - composed().float()).abs().max().item())

            xin = torch.randn(m, c_in, device=dev).to(dtype)
            wd = (torch.randn(mid, c_in, device=dev) / c_in ** 0.5).to(dtype)

            def fused_front():
                return ops.rows_linear_ln(xin, wd, None, gamma, beta, eps, ops.ACT_RELU)

            def composed_front():
                return ops.affine_act(ops.layernorm(ops.gemm(xin, wd), gamma, beta, eps), None, None, ops.ACT_RELU)
            a, b = _time(fused_front, steps, warmup), _time(composed_front, steps, warmup)
            nbytes = esz * (m * c_in + m * mid + mid * c_in)
            _emit(op="rows_linear_ln", scene=scene, level=name, rows=m, c=c_in, cout=mid, dtype=str(dtype)[6:],
                  fused_ms=a, composed_ms=b, speedup=b / a, fused_gbs=nbytes / a / 1e6,
                  max_abs_diff=(fused_front().float() - composed_front().float()).abs().max().item())


def bench_model(model, data, scene, steps, warmup):
    from ptv3_hip.lib import lib
    from pointcept.models.keypoint_ptv3_plus import BlockPlus

    def forward():
        torch.manual_seed(1)
        with torch.no_grad():
            return model(dict(data))["pred"]

    for dtype in (torch.float32, torch.bfloat16):
        model.backbone.compute_dtype = dtype
        res = {}
        for fused in (True, False):
            model.set_fused(fused)
            res[fused] = (_time(forward, steps, warmup), forward())
        _emit(op="eval_forward", scene=scene, dtype=str(dtype)[6:], fused_ms=res[True][0], composed_ms=res[False][0],
              speedup=res[False][0] / res[True][0], max_abs_diff=(res[True][1] - res[False][1]).abs().max().item())
    model.backbone.compute_dtype = None
    # library calls of one BlockPlus (the first of the encoder), counted on the ctypes handle
    block = next(m for m in model.modules() if isinstance(m, BlockPlus))
    dll = lib.load()
    for fused in (True, False):
        model.set_fused(fused)
        count = {"n": 0, "on": False}
        names = [n for n in ("ptv3_gemm", "ptv3_layernorm", "ptv3_affine_act", "ptv3_rows_linear_ln", "ptv3_subm_conv_ln",
                             "ptv3_block_head", "ptv3_block_tail", "ptv3_window_attn_fwd", "ptv3_rows_linear",
                             "ptv3_window_attn_varlen_fwd")]
        originals = {n: getattr(dll, n) for n in names}

        def wrap(fn):
            def call(*a):
                count["n"] += count["on"]
                return fn(*a)
            return call
        for n in names:
            setattr(dll, n, wrap(originals[n]))
        pre = block.register_forward_pre_hook(lambda m, a: count.__setitem__("on", True))
        post = block.register_forward_hook(lambda m, a, o: count.__setitem__("on", False))
        forward()
        pre.remove()
        post.remove()
        for n in names:
            setattr(dll, n, originals[n])
        _emit(op="block_plus_library_calls", scene=scene, fused=fused, calls=count["n"])
    model.set_fused(True)


def bench_train(model, data, scene, steps, warmup):
    model.train()
    data = dict(data)
    b = data["offset"].shape[0]
    data["target"] = torch.zeros(b * 6, 3, device=data["feat"].device)

    def step():
        torch.manual_seed(1)
        model.zero_grad(set_to_none=True)
        model(dict(data))["loss"].backward()
    _emit(op="train_step_fwd_bwd", scene=scene, dtype="float32", ms=_time(step, steps, warmup))
    model.eval()


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ptv3_plus", "bench_cpe_plus.jsonl"))
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no CPU fallback"
    # lines go to a side file that replaces --out only after a complete run: a partial run keeps the earlier results
    OUT = args.out + ".partial"
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    open(OUT, "w").close()
    import ptv3_scenes as S
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_PTV3_PLUS_CFG
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = build_model(KEYPOINT_PTV3_PLUS_CFG).to(dev).eval()
    for scene, sizes in (("8x20000", [20000] * 8), ("1x100000", [100000])):
        data = {k: v.to(dev) for k, v in S.make_batch(sizes, in_channels=4, extent=None, seed=7).items()}
        levels = _levels(model, data)
        bench_kernels(levels, scene, args.steps, args.warmup, dev)
        del levels
        bench_model(model, data, scene, args.steps, args.warmup)
        if not args.no_train and len(sizes) > 1:      # one scene cannot train (batch-statistic BatchNorm of the head)
            bench_train(model, data, scene, max(3, args.steps // 4), 1)
    os.replace(OUT, args.out)


if __name__ == "__main__":
    main()
