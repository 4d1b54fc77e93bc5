"""Time the OA-CNNs kernels with HIP events (median of --steps calls after --warmup) at the fork's shapes: 8 x 20 000
sites, channels 64 / 64 / 128 / 256, grids of configs/my_dataset/keypoint_oa_cnns.py.
  * ptv3_down2_conv / ptv3_up2_conv of every level beside their torch compositions (child-table gather + matmul;
    per-tap gather + matmul + row scatter), with the bytes the shapes imply;
  * ptv3_cluster_center / _softmax_sum / _mix of every stage and grid beside the torch statements of the reference
    (index_add scatter, gather), with achieved GB/s against the 8.0 TB/s HBM3E peak (6.3 TB/s measured copy rate);
  * the KeypointOACNNs eval forward, fused beside set_fused(False), and one training step (forward + backward + AdamW);
  * library calls and torch ops issued per BasicBlock, both ways (a library call is one launch except a split-K GEMM).
Outputs are compared at the timed sizes.  Prints one JSON line per measurement.
usage: python tools/bench_oacnns.py [--steps 20] [--warmup 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0


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
    print(json.dumps({k: (float(f"{v:.4g}") if isinstance(v, float) else v) for k, v in kw.items()}), flush=True)


def _levels(dev):
    """Site lists and down plans of the four levels under an 8 x 20 000 batch."""
    import ptv3_scenes as S
    from ptv3_hip import ops
    data = S.make_batch([20000] * 8, in_channels=4, extent=None, seed=7)
    grid = data["grid_coord"]
    batch = torch.repeat_interleave(torch.arange(8), 20000)
    idx = torch.cat([batch[:, None], grid], 1).int().to(dev)
    shape = (grid.max(0).values + 1).tolist()
    plans = []
    for _ in range(4):
        plan = ops.down2_plan(idx, shape, 8)
        plans.append(plan)
        idx, shape = plan.coarse.contiguous(), plan.out_shape
    return data, plans


def bench_convs(plans, cfg, steps, warmup, dev):
    from ptv3_hip import ops
    enc = [cfg["embed_channels"]] + cfg["enc_channels"]
    dec = cfg["dec_channels"] + [cfg["enc_channels"][-1]]
    for i, plan in enumerate(plans):
        for kind, cin, cout in (("down2_conv", enc[i], enc[i + 1]), ("up2_conv", dec[i + 1], dec[i])):
            torch.manual_seed(i)
            rows_in, rows_out = (plan.n, plan.m_out) if kind == "down2_conv" else (plan.m_out, plan.n)
            x = torch.randn(rows_in, cin, device=dev)
            w = torch.randn(cout, 2, 2, 2, cin, device=dev) / (8 * cin) ** 0.5
            scale, shift = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev)
            child, parent, rows, inv = plan.long_indices()
            ts = plan.tap_start

            def fused():
                fn = ops.down2_conv if kind == "down2_conv" else ops.up2_conv
                return fn(x, w, plan, scale, shift, ops.ACT_RELU)

            def torch_down():
                g = torch.cat([x, x.new_zeros(1, cin)])[child.reshape(-1)].view(plan.m_out, 8 * cin)
                return torch.relu(g @ w.view(cout, -1).T * scale + shift)

            def torch_up():
                wt = w.view(cout, 8, cin)
                parts = [x[parent[rows[ts[t]:ts[t + 1]]]] @ wt[:, t].T for t in range(8)]
                parts.append(x.new_zeros(plan.dropped, cout))
                return torch.relu(torch.cat(parts)[inv] * scale + shift)
            comp = torch_down if kind == "down2_conv" else torch_up
            a, b = _time(fused, steps, warmup), _time(comp, steps, warmup)
            nbytes = 4 * (rows_in * cin + rows_out * cout + w.numel()) + 4 * (plan.m_out * 8 if kind == "down2_conv" else 2 * plan.n)
            _emit(op=kind, level=i, rows_in=rows_in, rows_out=rows_out, cin=cin, cout=cout, hip_ms=a,
                  torch_composition_ms=b, speedup=b / a, bytes=nbytes, hip_gbs=nbytes / a / 1e6,
                  gflops=2.0 * (plan.n - plan.dropped) * cin * cout / a / 1e6,     # one tap per fine site, both ways
                  max_abs_diff=(fused() - comp()).abs().max().item())


def bench_clusters(plans, cfg, steps, warmup, dev):
    from ptv3_hip import ops
    for i, plan in enumerate(plans):
        c, m = cfg["enc_channels"][i], plan.m_out
        idx = plan.coarse.contiguous()
        low = idx[:, 1:].amin(0).contiguous()
        grids = cfg["point_grid_size"][i]
        cps = {g: ops.cluster_plan(idx, low, g) for g in set(grids)}
        torch.manual_seed(i)
        wide = torch.randn(m, 3 * c, device=dev)
        x, p, v = wide[:, :c], (wide[:, c:2 * c] * 2).contiguous(), wide[:, 2 * c:]
        gmax = torch.amax(p)
        for g in sorted(cps):
            cp = cps[g]
            k, ids = cp.count(), cp.cluster
            size = torch.bincount(ids, minlength=k).float().unsqueeze(1)

            def seg(t):
                return t.new_zeros(k, t.shape[1]).index_add_(0, ids, t)

            def t_center():
                return x - (seg(x) / size)[ids]

            def t_ssum():
                e = torch.exp(p - p.max())
                return seg(v * (e / (seg(e)[ids] + 1e-6)))
            for name, hip, comp, nbytes in (
                    ("cluster_center", lambda: ops.cluster_center(x, cp), t_center, 4 * 3 * m * c),
                    ("cluster_softmax_sum", lambda: ops.cluster_softmax_sum(p, v, gmax, cp)[:k], t_ssum,
                     4 * (2 * m * c + k * c))):
                a, b = _time(hip, steps, warmup), _time(comp, steps, warmup)
                _emit(op=name, stage=i, rows=m, c=c, grid=g, clusters=k, hip_ms=a, torch_composition_ms=b, speedup=b / a,
                      bytes=nbytes, hip_gbs=nbytes / a / 1e6, hbm_peak_fraction=nbytes / a / 1e6 / HBM_PEAK_GBS,
                      max_abs_diff=(hip() - comp()).abs().max().item())
        pl = [cps[g] for g in grids]
        logits = torch.randn(m, len(grids), device=dev)
        aggs = [torch.randn(m, c, device=dev) for _ in grids]

        def t_mix():
            adp = torch.softmax(logits, 1)
            feats = torch.stack([a[q.cluster] for a, q in zip(aggs, pl)], 1)
            return torch.einsum("l n, l n c -> l c", adp, feats)
        a, b = _time(lambda: ops.cluster_mix(logits, aggs, pl), steps, warmup), _time(t_mix, steps, warmup)
        nbytes = 4 * m * c * (len(grids) + 1)
        _emit(op="cluster_mix", stage=i, rows=m, c=c, grids=len(grids), hip_ms=a, torch_composition_ms=b, speedup=b / a,
              bytes=nbytes, hip_gbs=nbytes / a / 1e6, hbm_peak_fraction=nbytes / a / 1e6 / HBM_PEAK_GBS,
              max_abs_diff=(ops.cluster_mix(logits, aggs, pl) - t_mix()).abs().max().item())


class _Count(torch.utils._python_dispatch.TorchDispatchMode):
    """aten ops that compute (views and metadata ops excluded)"""
    SKIP = ("view", "slice", "select", "expand", "unsqueeze", "squeeze", "transpose", "permute", "reshape", "detach",
            "alias", "as_strided", "t.default", "empty", "_unsafe_view", "sym_", "size", "stride", "is_")

    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func).replace("aten.", "")
        if not any(name.startswith(s) for s in self.SKIP):
            self.n += 1
        return func(*args, **(kwargs or {}))


def bench_model(data, steps, warmup, dev):
    from pointcept.models import build_model
    from ptv3_hip.configs import KEYPOINT_OACNNS_CFG
    from ptv3_hip.lib import lib
    torch.manual_seed(0)
    model = build_model(KEYPOINT_OACNNS_CFG).to(dev).eval()
    data = {k: v.to(dev) for k, v in data.items() if k in ("grid_coord", "feat", "offset")}
    data["target"] = torch.randn(48, 3, device=dev) * 0.5

    def forward():
        with torch.no_grad():
            return model(dict(data))["pred"]

    def block_calls():
        """(library calls, torch ops) of the first BasicBlock of stage 0 in one forward"""
        block, calls = model.enc[0].blocks[0], [0, 0]
        inner, check = block.forward, type(lib).check

        def counted(x, clusters):
            def tick(self, rc, what):
                calls[0] += 1
                return check(self, rc, what)
            type(lib).check = tick
            try:
                with _Count() as cnt:
                    out = inner(x, clusters)
            finally:
                type(lib).check = check
            calls[1] = cnt.n
            return out
        block.forward = counted
        forward()
        del block.forward
        return calls
    fused = _time(forward, steps, warmup)
    pred, calls_fused = forward(), block_calls()
    model.set_fused(False)
    plain = _time(forward, steps, warmup)
    diff, calls_plain = (forward() - pred).abs().max().item(), block_calls()
    _emit(op="KeypointOACNNs eval", scenes=8, scene_sites=20000, fused_ms=fused, torch_composition_ms=plain,
          speedup=plain / fused, max_abs_diff_pred=diff)
    _emit(op="BasicBlock issue count", grids=4, fused_library_calls=calls_fused[0], fused_torch_ops=calls_fused[1],
          composed_library_calls=calls_plain[0], composed_torch_ops=calls_plain[1])
    model.set_fused(True).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=0.05)

    def step():
        opt.zero_grad(set_to_none=True)
        model(dict(data))["loss"].backward()
        opt.step()
    _emit(op="KeypointOACNNs training step", scenes=8, scene_sites=20000, ms=_time(step, max(3, steps // 4), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_oacnns measures on the GPU only"
    dev = torch.device("cuda:0")
    from ptv3_hip.configs import KEYPOINT_OACNNS_CFG as CFG
    data, plans = _levels(dev)
    _emit(op="levels", rows=[plans[0].n] + [q.m_out for q in plans], dropped=[q.dropped for q in plans])
    bench_convs(plans, CFG, args.steps, args.warmup, dev)
    bench_clusters(plans, CFG, args.steps, args.warmup, dev)
    bench_model(data, args.steps, args.warmup, dev)


if __name__ == "__main__":
    main()
