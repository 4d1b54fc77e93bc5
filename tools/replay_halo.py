"""CPU replay of the halo plan of a 3^3 submanifold convolution (csrc/halo_plan.h): how many DISTINCT neighbour rows a
tile of T consecutive sites has when the sites are taken in Morton order (the executor's row_order).  numpy only.

    python tools/replay_halo.py --points 100000 --kind surface --level 0 1 --tile 64 128 256 --cap 384

Per (level, T): active neighbours per site, distinct rows per tile (mean / p99 / max), rows fetched per site, and the
share of tiles with more than --cap distinct rows (the tiles ptv3_conv_halo gathers per tap instead).  Level l is the
scene's grid >> l with duplicates merged, which is what a stride-2 pooling per stage leaves."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pointcept-keypointdetection_amd"))


def morton_order(grid):
    """argsort of the z-order key (x, y, z bit-interleaved, x most significant)"""
    g = grid.astype(np.uint64)
    key = np.zeros(len(g), dtype=np.uint64)
    for b in range(int(g.max()).bit_length() or 1):
        for axis in range(3):
            key |= ((g[:, axis] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + 2 - axis)
    return np.argsort(key, kind="stable")


def neighbour_table(grid):
    """(n, 27) int64: row of the site at offset (a, b, c) - 1, tap 9a + 3b + c; -1 where there is none"""
    g = grid.astype(np.int64) + 1
    m = int(g.max()) + 2
    key = (g[:, 0] * m + g[:, 1]) * m + g[:, 2]
    perm = np.argsort(key)
    skey = key[perm]
    nbr = np.full((len(g), 27), -1, dtype=np.int64)
    for d in range(27):
        off = ((d // 9 - 1) * m + ((d // 3) % 3 - 1)) * m + (d % 3 - 1)
        q = key + off
        pos = np.minimum(np.searchsorted(skey, q), len(skey) - 1)
        hit = skey[pos] == q
        nbr[hit, d] = perm[pos[hit]]
    return nbr


def tile_counts(nbr, order, tile):
    """distinct neighbour rows of every run of `tile` consecutive sites of `order`"""
    counts = []
    for t0 in range(0, len(order), tile):
        v = nbr[order[t0:t0 + tile]].ravel()
        counts.append(len(np.unique(v[v >= 0])))
    return np.asarray(counts)


def replay(grid, level, tiles, cap):
    g = np.unique(grid >> level, axis=0) if level else grid
    nbr = neighbour_table(g)
    order = morton_order(g)
    rows = []
    for t in tiles:
        c = tile_counts(nbr, order, t)
        rows.append(dict(level=level, sites=len(g), active=float((nbr >= 0).sum(1).mean()), tile=t, mean=float(c.mean()),
                         p99=float(np.percentile(c, 99)), max=int(c.max()), per_site=float(c.sum() / len(g)),
                         over_cap=float((c > cap).mean())))
    return rows


def main():
    import ptv3_scenes as S
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--kind", default="surface", choices=["surface", "lidar"])
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--extent", type=int, default=None, help="default: the dense mode bench.py uses")
    ap.add_argument("--level", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--tile", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--cap", type=int, default=384)
    args = ap.parse_args()
    grid = S.make_scene(args.points, 4, args.extent, args.seed, args.kind)["grid_coord"]
    print("| level | sites | active / site | T | distinct rows per tile: mean / p99 / max | rows per site | tiles > %d |" % args.cap)
    print("|---|---|---|---|---|---|---|")
    for level in args.level:
        for r in replay(grid, level, args.tile, args.cap):
            print("| %d | %d | %.2f | %d | %.0f / %.0f / %d | %.2f | %.1f %% |" % (
                r["level"], r["sites"], r["active"], r["tile"], r["mean"], r["p99"], r["max"], r["per_site"],
                100 * r["over_cap"]))


if __name__ == "__main__":
    main()
