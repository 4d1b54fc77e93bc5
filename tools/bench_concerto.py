"""Time the three steps of Concerto's image branch (csrc/concerto.hip) against the composed path of this library
(pointcept/models/concerto: the same arithmetic in torch, occupied patches only) and against the reference's literal
formulation written in torch (per-image sort and segment sums; gather, dense scatter-mean over every patch row, the
projection over all of them, then the select; shift, CosineSimilarity, mean), all in one process, windows alternating,
median and minimum of `--windows` windows of at least `--calls` calls and at least 30 ms each:
  pool_corr           one pooling level of the correspondences, level 0 -> level 1
  mean+proj fwd       patch plan, patch mean, patch_proj;  fwd+bwd: and the gradients of the features and of patch_proj
  cos fwd / fwd+bwd   the centred cosine loss and the gradient of the projected rows
and each kernel on its own, with the bytes it has to read and write and the rate that makes.  A window calls a kernel
repeatedly over the same buffers, so whatever of them the last-level cache holds is served from there: the rates are no
HBM rates.

Shapes (`--configs`): C = 1184 with D = 1536 (pretrain-concerto-v1m1-0-base: 48 + 96 + 192 + 384 + 512 - 48 channels at
level 1) and C = 1664 with D = 1536 (the large config), 37 x 37 patches per image.  One rank's batch is taken as 4 scenes
of 2 global views with 60 000 points a view after grid sampling (the order of an indoor scene at the configs' 2 cm
grid), so 480 000 level-0 points; a stride-2 pooling leaves about a quarter, 120 000 level-1 rows of which the 60 000 of the
principal views take part; 4 images per scene, V = 4 and 16 images = 21 904 patch rows; a point is visible in an image with
probability 0.3, and its pixel is uniform over the image, so nearly every patch is occupied (U close to 21 904) by
about 3 pairs.  Prints one JSON line per measurement.  The reference's own CUDA run is not timed here.
usage: python tools/bench_concerto.py [--windows 7] [--calls 3] [--configs 1184:1536,1664:1536] [--dtypes fp32,bf16]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402

MIN_WINDOW_MS = 30.0
SCENES, VIEW_POINTS, IMAGES, PATCH, VISIBLE = 4, 60000, 4, 37, 0.3


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


# ---- the reference's literal formulation ----------------------------------------------------------------------------
def literal_pool(corr, inverse, idx_ptr):
    _, indices = torch.sort(inverse)
    lengths = idx_ptr[1:] - idx_ptr[:-1]
    minus = torch.tensor([-1.0, -1.0], device=corr.device)
    out = []
    for image in range(corr.shape[1]):
        both = torch.all(corr[:, image] != minus, dim=1).float()
        counts = torch.segment_reduce(both[indices], "sum", lengths=lengths, unsafe=True)
        counts[counts == 0] = 100000
        filled = corr[:, image].clone()
        filled[filled == -1] = 0
        mean = torch.segment_reduce(filled[indices], "sum", lengths=lengths, axis=0, unsafe=True) / counts.unsqueeze(1)
        mean[counts == 100000] = -1
        out.append(mean)
    return torch.stack(out, dim=1)


def literal_mean_proj(feat, corr, rows, scene, img_base, proj, n_patches):
    sub = corr[rows]
    r, v = torch.where(torch.any(sub != torch.tensor([-1.0, -1.0], device=corr.device), dim=2))
    c = sub[r, v].long()
    index = (img_base[scene[r]] + v) * PATCH * PATCH + c[:, 0] * PATCH + c[:, 1]
    gathered = feat[rows][r]
    total = gathered.new_zeros((n_patches, feat.shape[1])).index_add_(0, index, gathered)
    count = gathered.new_zeros(n_patches).index_add_(0, index, torch.ones_like(index, dtype=gathered.dtype))
    dense = proj(total / count.clamp(min=1).unsqueeze(1))
    ids = torch.unique(index)
    return dense[ids], ids


def literal_cos(a, b, ids):
    b = b[ids]
    b = b - b.mean(dim=-1, keepdim=True)
    a = a - a.mean(dim=-1, keepdim=True)
    return (1 - torch.nn.CosineSimilarity(dim=1, eps=1e-6)(b, a)).mean() * 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--configs", default="1184:1536,1664:1536")
    ap.add_argument("--dtypes", default="fp32,bf16")
    args = ap.parse_args()
    from pointcept.models.concerto import concerto_v1m1_base as M
    from ptv3_hip import ops
    from ptv3_hip import autograd as A
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    def report(what, shape, dtype, res, bytes_=0):
        f = res["fused"]
        line = dict(what=what, **shape, dtype=dtype, fused_ms=round(f[0], 4), fused_min_ms=round(f[1], 4), fused_calls=f[2])
        for other in ("composed", "literal"):
            if other in res:
                o = res[other]
                line.update({other + "_ms": round(o[0], 4), other + "_min_ms": round(o[1], 4), other + "_calls": o[2],
                             "speedup_vs_" + other: round(o[0] / f[0], 3)})
        if bytes_:
            line.update(kernel_bytes=int(bytes_), fused_GBps=round(bytes_ / f[0] / 1e6, 1))
        print(json.dumps(line), flush=True)

    # ---- the geometry: one pooling level and the level-0 correspondences ------------------------------------------
    n0 = SCENES * 2 * VIEW_POINTS
    n1 = n0 // 4
    inverse = torch.randint(0, n1, (n0,), device=dev)
    inverse[:n1] = torch.arange(n1, device=dev)                              # no empty cluster
    order = torch.sort(inverse, stable=True)[1]
    idx_ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.cumsum(torch.bincount(inverse, minlength=n1), 0)])
    seg_start = idx_ptr.int()
    view0 = torch.arange(n0, device=dev) // VIEW_POINTS
    # a level-1 cluster sees an image or it does not (visibility is spatially coherent), its children share a pixel cell
    seen = torch.rand(n1, IMAGES, device=dev) < VISIBLE
    cell = torch.randint(0, PATCH, (n1, IMAGES, 2), device=dev).float()
    corr0 = torch.where(seen[inverse].unsqueeze(-1), cell[inverse], -torch.ones(n0, IMAGES, 2, device=dev)).contiguous()
    shape = dict(n0=n0, n1=n1, V=IMAGES)
    with torch.no_grad():
        res = _ab({"fused": lambda: ops.concerto_pool_corr(corr0, order, seg_start),
                   "composed": lambda: M.pool_corr_torch(corr0, inverse, n1),
                   "literal": lambda: literal_pool(corr0, inverse, idx_ptr)}, args.windows, args.calls)
    report("pool_corr", shape, "fp32", res, n0 * IMAGES * 8 + n0 * 8 + n1 * IMAGES * 8)
    corr1 = ops.concerto_pool_corr(corr0, order, seg_start)
    assert torch.equal(corr1, literal_pool(corr0, inverse, idx_ptr))

    # level 1: the rows of the principal views (the first of every two views of n1 / (2 SCENES) rows)
    per_view = n1 // (2 * SCENES)
    rows = torch.cat([torch.arange(2 * b * per_view, (2 * b + 1) * per_view, device=dev) for b in range(SCENES)])
    scene = torch.arange(SCENES, device=dev).repeat_interleave(per_view)
    img_base = torch.arange(SCENES, device=dev) * IMAGES
    n_patches = SCENES * IMAGES * PATCH * PATCH

    for c, d in [tuple(int(v) for v in cfg.split(":")) for cfg in args.configs.split(",")]:
        proj = torch.nn.Linear(c, d).to(dev)
        for name in args.dtypes.split(","):
            dtype = dict(fp32=torch.float32, bf16=torch.bfloat16)[name]
            size = 4 if dtype == torch.float32 else 2
            cast = torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16)
            feat = torch.randn(n1, c, device=dev).to(dtype)
            fg = feat.clone().requires_grad_(True)
            plan = ops.concerto_plan(corr1, rows, scene, img_base, PATCH, PATCH, n_patches, check=True)
            pairs, u = int(plan.seg_start[plan.u]), plan.u
            shape = dict(C=c, D=d, n1=n1, rows=int(rows.shape[0]), pairs=pairs, U=u, patches=n_patches)

            def fused(f):
                p = ops.concerto_plan(corr1, rows, scene, img_base, PATCH, PATCH, n_patches)
                with cast:
                    return proj(A.concerto_patch_mean(f, p))

            def composed(f):
                ids, slot, count, pair_row = M.patch_plan_torch(corr1, rows, scene, img_base, PATCH, PATCH)
                with cast:
                    return proj(M.patch_mean_torch(f, pair_row, slot, count))

            def literal(f):
                with cast:
                    return literal_mean_proj(f, corr1, rows, scene, img_base, proj, n_patches)[0]

            def fwd(fn):
                with torch.no_grad():
                    fn(feat)

            def fwd_bwd(fn):
                fg.grad = None
                proj.zero_grad(set_to_none=True)
                fn(fg).float().square().sum().backward()

            variants = dict(fused=fused, composed=composed, literal=literal)
            report("mean+proj fwd", shape, name, _ab({k: (lambda fn=fn: fwd(fn)) for k, fn in variants.items()},
                                                     args.windows, args.calls))
            report("mean+proj fwd+bwd", shape, name, _ab({k: (lambda fn=fn: fwd_bwd(fn)) for k, fn in variants.items()},
                                                         args.windows, args.calls))
            dmean = torch.randn(u, c, device=dev)
            report("plan", shape, name, _ab({"fused": lambda: ops.concerto_plan(corr1, rows, scene, img_base, PATCH, PATCH,
                                                                                n_patches)}, args.windows, args.calls))
            report("patch_mean_fwd", shape, name, _ab({"fused": lambda: ops.concerto_patch_mean(feat, plan)}, args.windows,
                                                      args.calls), pairs * c * size + u * c * 4)
            report("patch_mean_bwd", shape, name, _ab({"fused": lambda: ops.concerto_patch_mean_bwd(dmean, plan, dtype)},
                                                      args.windows, args.calls), pairs * c * 4 + n1 * c * size)

            # ---- the cosine loss on U projected rows ----------------------------------------------------------------
            a = torch.randn(u, d, device=dev).to(dtype)
            ag = a.clone().requires_grad_(True)
            b = torch.randn(n_patches, d, device=dev)
            ids = plan.patch_ids
            losses = dict(fused=lambda x: A.concerto_cos_loss(x, b, ids, True),
                          composed=lambda x: M.cos_loss_torch(x, b, ids, True), literal=lambda x: literal_cos(x, b, ids))

            def cos_fwd(fn):
                with torch.no_grad():
                    fn(a)

            def cos_fwd_bwd(fn):
                ag.grad = None
                fn(ag).backward()

            report("cos fwd", shape, name, _ab({k: (lambda fn=fn: cos_fwd(fn)) for k, fn in losses.items()}, args.windows,
                                               args.calls), u * d * (size + 4))
            report("cos fwd+bwd", shape, name, _ab({k: (lambda fn=fn: cos_fwd_bwd(fn)) for k, fn in losses.items()},
                                                   args.windows, args.calls), u * d * (3 * size + 8))
            one = torch.ones(1, device=dev)
            report("cos_fwd kernel", shape, name, _ab({"fused": lambda: ops.concerto_cos(a, b, ids, True)}, args.windows,
                                                      args.calls), u * d * (size + 4))
            report("cos_bwd kernel", shape, name, _ab({"fused": lambda: ops.concerto_cos_bwd(one, a, b, ids, True)},
                                                      args.windows, args.calls), u * d * (2 * size + 4))
            del feat, fg, a, ag, b
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
