"""Time the sparse-conv neighbour tables: the per-voxel hash (ptv3_subm_build_table + ptv3_subm_neighbors: -1 pre-fill
and the half-probing kernel) against the 4^3 block table (ptv3_subm_build_block_table + ptv3_subm_neighbors_blocks).
Shapes: the 100k surface scene and the 120k LiDAR scene of bench.py, k = 5 and 3.  HIP events around each call (the
old k-table figure includes its pre-fill), median of --reps after a warm-up; the two tables are compared bitwise.
usage: python tools/bench_neighbors.py [--reps 30] [--which both|old|new] [--scene both|surface|lidar]
(--reps 1 --scene surface under a counter collection: tools/pmc_kernels.py averages over the dispatches of a kernel)"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "pointcept-keypointdetection_amd")]
from ptv3_hip.lib import lib  # noqa: E402
from ptv3_hip.ops import _p, _stream  # noqa: E402
import ptv3_scenes as S  # noqa: E402


def median_us(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(times)


def old_path(idx):
    n = idx.shape[0]
    slots = lib.ptv3_subm_table_slots(n)
    table = torch.empty(slots * 12, dtype=torch.uint8, device=idx.device)
    build = lambda: lib.check(lib.ptv3_subm_build_table(_p(idx), n, _p(table), slots, _stream()), "build")  # noqa: E731
    query = lambda k, nbr: lib.check(lib.ptv3_subm_neighbors(_p(idx), n, _p(table), slots, k, _p(nbr), _stream()), "nbr")  # noqa: E731
    return build, query


def new_path(idx):
    n = idx.shape[0]
    table = torch.empty(lib.ptv3_subm_block_table_bytes(n), dtype=torch.uint8, device=idx.device)
    build = lambda: lib.check(lib.ptv3_subm_build_block_table(_p(idx), n, _p(table), table.numel(), _stream()), "build")  # noqa: E731
    query = lambda k, nbr: lib.check(lib.ptv3_subm_neighbors_blocks(_p(idx), n, _p(table), table.numel(), k, _p(nbr),  # noqa: E731
                                                                    _stream()), "nbr")
    return build, query


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--which", default="both", choices=["both", "old", "new"])
    ap.add_argument("--scene", default="both", choices=["both", "surface", "lidar"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    warm = min(5, args.reps)
    for name, points, extent, kind in (("surface 100k", 100000, None, "surface"), ("lidar 120k", 120000, 2048, "lidar")):
        if args.scene not in ("both", kind):
            continue
        scene = S.make_scene(points, 4, extent, 1000, kind)
        grid = torch.from_numpy(scene["grid_coord"]).int()
        idx = torch.cat([torch.zeros(len(grid), 1, dtype=torch.int32), grid], 1).contiguous().to(dev)
        paths = [(tag, *make(idx)) for tag, make in (("old", old_path), ("new", new_path)) if args.which in ("both", tag)]
        for tag, build, _ in paths:
            print(f"{name:13s} {tag} build      {median_us(build, args.reps, warm):8.1f} us")
        for k in (5, 3):
            got = {}
            for tag, _, query in paths:
                got[tag] = torch.full((idx.shape[0], k ** 3), -7, dtype=torch.int32, device=dev)
                us = median_us(lambda: query(k, got[tag]), args.reps, warm)
                print(f"{name:13s} {tag} k={k} table  {us:8.1f} us")
            if len(got) == 2:
                print(f"{name:13s} k={k} tables equal: {torch.equal(got['old'], got['new'])}")


if __name__ == "__main__":
    main()
