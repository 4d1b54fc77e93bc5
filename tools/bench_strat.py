"""Time the Stratified Transformer attention with HIP events (median of --steps calls after --warmup):
  * ops.stratified_attention (ptv3_strat_attn_fwd) beside the pointops2 edge composition of the same formula (what
    set_fused(False) and training run between qkv and proj) at the fork's four (C, heads, window, quant) levels, both
    parities, with the groups, the mean keys per group and the pairs each plan holds, and the time to build the plan;
  * the whole KeypointStratifiedTransformer eval forward, fused beside set_fused(False), with the distance between
    their predictions.
Input: --scenes ellipsoid surfaces of 1.8 x 0.6 x 0.8, grid-sampled at 0.02 (one point per cell), then reduced 4x per
level by the model's own farthest point sampling.
Prints one JSON line per measurement and appends them to profiles/strat/bench_strat.jsonl.
usage: python tools/bench_strat.py [--steps 20] [--warmup 3] [--scenes 8] [--out profiles/strat/bench_strat.jsonl]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]

import torch  # noqa: E402


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


def make_batch(scenes, dev, seed=1):
    """coord (n, 3), feat (n, 4), offset (scenes) int32: per scene 120 000 random directions pushed onto the ellipsoid
    with semi-axes (0.9, 0.3, 0.4) and a little noise, one point kept per 0.02 cell."""
    g = torch.Generator().manual_seed(seed)
    coords, ends, total = [], [], 0
    for _ in range(scenes):
        d = torch.randn(120000, 3, generator=g)
        p = d / d.norm(dim=1, keepdim=True) * torch.tensor([0.9, 0.3, 0.4]) + 0.002 * torch.randn(120000, 3, generator=g)
        cell = torch.floor(p / 0.02).long()
        key = (cell[:, 0] + 512) * (1 << 40) + (cell[:, 1] + 512) * (1 << 20) + (cell[:, 2] + 512)
        _, first = torch.sort(key, stable=True)
        keep = torch.ones_like(key, dtype=torch.bool)
        keep[1:] = key[first][1:] != key[first][:-1]
        p = p[first[keep]]
        coords.append(p[torch.randperm(len(p), generator=g)] + torch.randn(3, generator=g))
        total += len(p)
        ends.append(total)
    coord = torch.cat(coords).float().contiguous()
    return dict(coord=coord.to(dev), feat=torch.randn(total, 4, generator=g).to(dev),
                offset=torch.tensor(ends, dtype=torch.int32, device=dev))


def levels(data, ratio, count):
    """[(coord, SceneOffsets, down_idx)] of the `count` attention levels: TransitionDown's sampling from level to level
    and BasicLayer's own sampled rows at each."""
    from ptv3_hip import ops
    from pointcept.models.point_transformer.point_transformer_seg import SceneOffsets
    from pointcept.models.stratified_transformer.stratified_transformer_v1m2_refine import (
        basic_layer_counts, transition_down_counts, _sizes, _level)
    coord, so = data["coord"], SceneOffsets.read(data["offset"])
    out = []
    for _ in range(count):
        nso = _level(transition_down_counts(_sizes(so.host), ratio), coord.device)
        coord = coord[ops.farthest_point_sampling(coord, so.dev, nso.dev, so.host, nso.host).long()].contiguous()
        so = nso
        dso = _level(basic_layer_counts(_sizes(so.host), ratio), coord.device)
        out.append((coord, so, ops.farthest_point_sampling(coord, so.dev, dso.dev, so.host, dso.host)))
    return out


def edge_attention(qkv, coord, edges, tables, scale, window, quant, rows):
    """WindowAttention.forward between qkv and proj over the edge list (the pointops2 compositions)."""
    import pointops2.pointops as P
    from pointcept.models.stratified_transformer.stratified_transformer_v1m2_refine import _scatter_softmax
    index_0, index_1, offsets = edges
    q, k, v = (qkv[:, i].contiguous() for i in range(3))
    q = q * scale
    rel = P.relative_position_index(coord, index_0, index_1, window, quant, rows)
    attn = P.attention_step1_v2(q, k, index_1, offsets, None) + \
        P.dot_prod_with_idx_v3(q, offsets, None, k, index_1, tables[0], tables[1], rel)
    attn = _scatter_softmax(attn, index_0, qkv.shape[0])
    return P.attention_step2_with_rel_pos_value_v2(attn, v, offsets, None, index_1, tables[2], rel)


def bench_attention(cfg, lv, steps, warmup, emit):
    from ptv3_hip import ops
    for i, (coord, so, down_idx) in enumerate(lv):
        c, heads = cfg["channels"][i + 1], cfg["num_heads"][i]
        w, quant = cfg["window_size"][i], cfg["quant_size"][i]
        rows = 2 * int((2 * w + 1e-4) // quant)
        n, d = coord.shape[0], c // heads
        g = torch.Generator(device=coord.device).manual_seed(i)
        qkv = torch.randn(n, 3, heads, d, device=coord.device, generator=g)
        tables = [0.02 * torch.randn(rows, heads, d, 3, device=coord.device, generator=g) for _ in range(3)]
        packed = [ops.strat_pack_tables(t) for t in tables]
        for shifted in (False, True):
            plan = ops.stratified_plan(coord, so.dev, down_idx, w, shifted)
            plan_ms = _time(lambda: ops.stratified_plan(coord, so.dev, down_idx, w, shifted), steps, warmup)
            nq = (plan.q_ptr[1:] - plan.q_ptr[:-1]).long()
            nk = (plan.k_ptr[1:] - plan.k_ptr[:-1]).long()
            pairs = int((nq * nk).sum().item())
            fused = lambda: ops.stratified_attention(qkv, coord, plan, *packed, d ** -0.5, w, quant)   # noqa: E731
            fused_ms = _time(fused, steps, warmup)
            index_0, index_1 = plan.edges()
            counts = torch.bincount(index_0, minlength=n)
            edges = (index_0, index_1, torch.cat([counts.new_zeros(1), counts.cumsum(0)]))
            plain = lambda: edge_attention(qkv, coord, edges, tables, d ** -0.5, w, quant, rows)   # noqa: E731
            with torch.no_grad():
                plain_ms = _time(plain, steps, warmup)
                diff = (fused().view(n, -1) - plain().view(n, -1)).abs().max().item()
            emit(dict(what="attention", level=i, shifted=shifted, points=n, c=c, heads=heads, window=w, quant=quant,
                      table_rows=rows, groups=plan.n_groups, mean_queries_per_group=n / plan.n_groups,
                      mean_keys_per_group=plan.n_keys / plan.n_groups, max_keys_per_group=int(nk.max().item()),
                      pairs=pairs, plan_ms=plan_ms, fused_ms=fused_ms, composition_ms=plain_ms,
                      ratio=plain_ms / fused_ms, max_abs_diff=diff))
            del edges, index_0, index_1


def bench_model(cfg, data, steps, warmup, emit):
    from pointcept.models import build_model
    torch.manual_seed(0)
    model = build_model(cfg).to(data["coord"].device).eval()
    for layer in model.layers:      # the reference's fresh key and value tables are zero: draw them as well
        for blk in layer.blocks:
            torch.nn.init.trunc_normal_(blk.attn.relative_pos_key_table, std=0.02)
            torch.nn.init.trunc_normal_(blk.attn.relative_pos_value_table, std=0.02)
    with torch.no_grad():
        fused_ms = _time(lambda: model(dict(data)), steps, warmup)
        fused = model(dict(data))["pred"]
        model.set_fused(False)
        plain_ms = _time(lambda: model(dict(data)), steps, warmup)
        plain = model(dict(data))["pred"]
    emit(dict(what="model_eval", points=data["coord"].shape[0], scenes=data["offset"].shape[0], fused_ms=fused_ms,
              composition_ms=plain_ms, ratio=plain_ms / fused_ms, max_abs_pred_diff=(fused - plain).abs().max().item()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strat", "bench_strat.jsonl"))
    ap.add_argument("--skip-model", action="store_true")
    args = ap.parse_args()
    from ptv3_hip.configs import KEYPOINT_STRAT_CFG as cfg
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    data = make_batch(args.scenes, dev)
    sizes = torch.diff(data["offset"], prepend=data["offset"].new_zeros(1)).tolist()
    emit(dict(what="input", scenes=args.scenes, points=data["coord"].shape[0], points_per_scene=sizes,
              steps=args.steps, warmup=args.warmup))
    bench_attention(cfg, levels(data, cfg["down_ratio"], 4), args.steps, args.warmup, emit)
    if not args.skip_model:
        bench_model(cfg, data, args.steps, args.warmup, emit)


if __name__ == "__main__":
    main()
