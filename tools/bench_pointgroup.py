"""Time PointGroup's evaluation tail (everything behind the two heads of PG-v1m1 / PG-v1m2) at 8 x 20 000 points and at one
100 000-point scene, per stage, three ways, all from this library's own entry points:
  fused     ptv3_pg_cluster + ptv3_pg_proposals + the three copies to the host               (what the model runs)
  lists     ptv3_pg_ballquery_batch_p (cell grid) + copy + host search + ptv3_pg_proposals   (the model's cap fallback)
  composed  the composition the reference implies: the brute scan of ptv3_ball_query, the copy of the neighbour lists,
            the host search, the dense mask scattered on the host, one masked mean and one copy per proposal
and a whole eval forward of PG_PTV3_SCANNET_CFG with the fused and with the composed tail.  The reference itself (CUDA)
is not timed here.  Inputs are synthetic: blobs of 200 points, each inside one ball and far from the others, one class per
blob, so neighbour counts stay far below 1000; in the whole forward the backbone and heads run on a ptv3_scenes batch and
the tail receives the blobs' centres and probabilities (random weights predict no clusters worth timing).
Host stages make wall-clock the honest measure: every stage is closed by a synchronisation; median of --reps runs.
The paths alternate inside every repetition.  The fused head (ptv3_pg_head_eval) and the fused bias losses are timed
first, against the composition the model runs, with CUDA events.
usage: python tools/bench_pointgroup.py [--reps 7] [--no-forward]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

RADIUS, MIN_POINTS, PROPOSE, BLOB = 1.5, 50, 100, 200


def blobs(sizes, dev, seed=0):
    """centres (N, 3) in voxel units, probabilities (N, 20), offsets: blobs of BLOB points on a jittered lattice 8 apart"""
    g = torch.Generator().manual_seed(seed)
    centre, logit = [], []
    for n in sizes:
        k = (n + BLOB - 1) // BLOB
        side = int(round(k ** (1 / 3))) + 1
        cell = torch.randperm(side ** 3, generator=g)[:k]
        c = torch.stack([cell // (side * side), (cell // side) % side, cell % side], 1).float() * 8.0
        c = c.repeat_interleave(BLOB, 0)[:n] + 0.2 * torch.randn(n, 3, generator=g)
        cls = torch.randint(2, 20, (k,), generator=g).repeat_interleave(BLOB)[:n]
        perm = torch.randperm(n, generator=g)
        centre.append(c[perm])
        logit.append((F.one_hot(cls, 20).float() * 8.0 + torch.randn(n, 20, generator=g))[perm])
    prob = torch.softmax(torch.cat(logit), 1)
    offset = torch.tensor([sum(sizes[:i + 1]) for i in range(len(sizes))])
    return torch.cat(centre).contiguous().to(dev), prob.contiguous().to(dev), offset.to(dev)


class Stages:
    def __init__(self):
        self.t = {}
        self._last = None

    def start(self):
        torch.cuda.synchronize()
        self._last = time.perf_counter()

    def lap(self, name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        if self._last is None:     # a run that was not started (warm-up, equality check): nothing to record
            self._last = now
        self.t[name] = self.t.get(name, 0.0) + (now - self._last) * 1e3
        self._last = now


def _offsets0(offset):
    return F.pad(offset.int(), (1, 0)).contiguous()


def tail_fused(center, prob, seg, offset, st):
    from ptv3_hip import ops
    idxs, offs, large = ops.pg_cluster(center, seg.int(), _offsets0(offset), RADIUS, MIN_POINTS, PROPOSE)
    st.lap("cluster")
    out = ops.pg_proposals(idxs, offs, prob, seg, PROPOSE, large)
    st.lap("proposals")
    res = [t.cpu() for t in out]
    st.lap("copy_out")
    return res


def tail_lists(center, prob, seg, offset, st):
    from ptv3_hip import ops
    import pointgroup_ops
    off0 = _offsets0(offset)
    idx, start_len = ops.pg_ballquery_batch_p(center, None, off0, RADIUS)
    st.lap("ball_query")
    h = seg.int().cpu(), idx.cpu(), start_len.cpu()
    st.lap("copy_lists")
    idxs, offs = pointgroup_ops.bfs_cluster(h[0], h[1], h[2], MIN_POINTS)
    st.lap("host_search")
    large = int(((offs[1:] - offs[:-1]) > PROPOSE).sum())
    out = ops.pg_proposals(idxs.to(center.device), offs.to(center.device), prob, seg, PROPOSE, large)
    st.lap("proposals")
    res = [t.cpu() for t in out]
    st.lap("copy_out")
    return res


def tail_composed(center, prob, seg, offset, st, max_neighbor=256):
    """point_group_v1m1_base.py:128-174 with the library's brute scan in place of the CUDA kernel"""
    from ptv3_hip import ops
    dense = ops.ball_query(RADIUS, max_neighbor, center, offset.int().contiguous())
    hit = dense >= 0
    count = hit.sum(1).int()
    start_len = torch.stack([torch.cumsum(count, 0).int() - count, count], 1).contiguous()
    idx = dense[hit].int()
    st.lap("ball_query")
    h = seg.int().cpu(), idx.cpu(), start_len.cpu()
    st.lap("copy_lists")
    idxs, offs = ops.pg_bfs_cluster_host(h[0], h[1], h[2], MIN_POINTS)
    st.lap("host_search")
    masks = torch.zeros((offs.shape[0] - 1, center.shape[0]), dtype=torch.int)
    masks[idxs[:, 0].long(), idxs[:, 1].long()] = 1
    inst = seg[idxs[:, 1][offs[:-1].long()].long().to(seg.device)]
    big = masks.sum(1) > PROPOSE
    masks, inst = masks[big], inst[big.to(inst.device)]
    st.lap("host_scatter")
    scores, classes = [], []
    for p in range(len(masks)):
        scores.append(prob[masks[p].bool(), inst[p]].mean())
        classes.append(inst[p])
    res = [torch.stack(classes).cpu(), torch.stack(scores).cpu(), masks] if scores else [None, None, masks]
    st.lap("proposal_loop")
    return res


def median_stages(paths, args, reps):
    """per-stage medians (and the spread of the total) of every path, the paths alternating inside each repetition"""
    runs = {name: [] for name, _ in paths}
    for name, fn in paths:
        fn(*args, Stages())  # warm-up
    for _ in range(reps):
        for name, fn in paths:
            st = Stages()
            st.start()
            fn(*args, st)
            runs[name].append(st.t)
    out = {}
    for name, rs in runs.items():
        med = {k: sorted(r[k] for r in rs)[reps // 2] for k in rs[0]}
        totals = sorted(sum(r.values()) for r in rs)
        med.update(total=totals[reps // 2], total_min=totals[0], total_max=totals[-1])
        out[name] = {k: round(v, 3) for k, v in med.items()}
    return out


def _event_ab(fns, windows=12, calls=20):
    """median us per call of each function, CUDA events, windows alternating"""
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
    return {k: round(sorted(v)[len(v) // 2], 2) for k, v in us.items()}


def bench_head_and_losses(dev):
    """the fused head and the fused bias losses against the composition the model runs (library Linear / BatchNorm
    kernels + torch softmax / argmax; the torch composition of the losses), forward and forward + backward"""
    import torch.nn as nn
    from pointcept.models.utils.hip_layers import Linear, BatchNorm1d, ReLU
    from ptv3_hip import ops, autograd as A
    for sizes, c, k in (([20000] * 8, 64, 20), ([20000] * 8, 96, 20), ([100000], 64, 20), ([100000], 96, 200)):
        n = sum(sizes)
        torch.manual_seed(0)
        head = nn.Sequential(Linear(c, c), BatchNorm1d(c, eps=1e-3, momentum=0.01), ReLU(), Linear(c, 3)).to(dev).eval()
        seg = Linear(c, k).to(dev).eval()
        feat, coord = torch.randn(n, c, device=dev), torch.rand(n, 3, device=dev)
        ignore = torch.tensor([-1, 0, 1], device=dev)

        def composed():
            with torch.no_grad():
                bias = head[3](head[2](head[1](head[0](feat))))
                prob = F.softmax(seg(feat), dim=-1)
                pred = torch.max(prob, 1)[1]
                return (coord + bias) / 0.02, ~torch.isin(pred, ignore)

        def fused():
            bn = head[1]
            return ops.pg_head_eval(feat, coord, head[0].weight, head[0].bias, bn.weight, bn.bias, bn.running_mean,
                                    bn.running_var, bn.eps, head[3].weight, head[3].bias, seg.weight, seg.bias, 0.02,
                                    (-1, 0, 1))

        print(json.dumps({"what": "head_eval", "scenes": len(sizes), "points": n, "c": c, "classes": k,
                          "us": _event_ab({"fused": fused, "composed": composed})}), flush=True)
    for sizes in ([20000] * 8, [100000]):
        n = sum(sizes)
        g = torch.Generator().manual_seed(1)
        bias = (torch.randn(n, 3, generator=g) * 0.05).to(dev).requires_grad_(True)
        coord = torch.rand(n, 3, generator=g).to(dev)
        centroid = coord + (torch.randn(n, 3, generator=g) * 0.05).to(dev)
        instance = torch.randint(-1, 30, (n,), generator=g).to(dev)

        def composed_loss():
            mask = (instance != -1).float()
            gt = centroid - coord
            l1 = torch.sum(torch.sum(torch.abs(bias - gt), dim=-1) * mask) / (torch.sum(mask) + 1e-8)
            pn = bias / (torch.norm(bias, p=2, dim=1, keepdim=True) + 1e-8)
            gn = gt / (torch.norm(gt, p=2, dim=1, keepdim=True) + 1e-8)
            return l1 + torch.sum(-(pn * gn).sum(-1) * mask) / (torch.sum(mask) + 1e-8)

        def fused_loss():
            l1, cs = A.pg_bias_loss(bias, coord, centroid, instance, -1)
            return l1 + cs

        def step(fn):
            bias.grad = None
            fn().backward()

        print(json.dumps({"what": "bias_loss", "scenes": len(sizes), "points": n,
                          "fwd_us": _event_ab({"fused": lambda: fused_loss().detach(),
                                               "composed": lambda: composed_loss().detach()}),
                          "fwd_bwd_us": _event_ab({"fused": lambda: step(fused_loss),
                                                   "composed": lambda: step(composed_loss)})}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-forward", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    bench_head_and_losses(dev)
    paths = (("fused", tail_fused), ("lists", tail_lists), ("composed", tail_composed))
    for sizes in ([20000] * 8, [100000]):
        center, prob, offset = blobs(sizes, dev)
        seg = prob.argmax(1)
        ref = tail_fused(center, prob, seg, offset, Stages())
        for name, fn in paths:
            got = fn(center, prob, seg, offset, Stages())
            assert torch.equal(got[2], ref[2]) and torch.equal(got[0], ref[0]), name   # the same proposals three ways
        for name, ms in median_stages(paths, (center, prob, seg, offset), args.reps).items():
            print(json.dumps({"what": "tail", "path": name, "scenes": len(sizes), "points": sum(sizes),
                              "proposals": int(ref[2].shape[0]), "ms": ms}), flush=True)
    if args.no_forward:
        return
    import ptv3_scenes as S
    from pointcept.models import build_model
    from ptv3_hip.configs import PG_PTV3_SCANNET_CFG
    sizes = [20000] * 8
    torch.manual_seed(0)
    model = build_model(PG_PTV3_SCANNET_CFG).to(dev).eval()
    data = {k: v.to(dev) for k, v in S.make_batch(sizes, in_channels=6, extent=None, seed=7).items()}
    data["instance_centroid"] = data["coord"].clone()
    center, prob, offset = blobs(sizes, dev)
    seg = prob.argmax(1)
    tails = (("heads_only", None), ("fused", tail_fused), ("composed", tail_composed))
    ms = {name: [] for name, _ in tails}
    for rep in range(args.reps + 2):     # the first two repetitions warm up; the three variants alternate
        for name, fn in tails:
            def tail(*a, fn=fn):   # the model's own predictions are dropped: see the module docstring
                return {} if fn is None else dict(zip(("pred_classes", "pred_scores", "pred_masks"),
                                                      fn(center, prob, seg, offset, Stages())))

            model._proposals = tail
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                model(dict(data))
            torch.cuda.synchronize()
            if rep >= 2:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    for name, v in ms.items():
        v = sorted(v)
        print(json.dumps({"what": "forward", "tail": name, "scenes": len(sizes), "points": sum(sizes),
                          "median_ms": round(v[len(v) // 2], 3), "min_ms": round(v[0], 3), "max_ms": round(v[-1], 3)}),
              flush=True)


if __name__ == "__main__":
    main()
