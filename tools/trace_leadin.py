"""Lead-in of a forward from a rocprofv3 --kernel-trace CSV of plain `bench.py`: every launch from the level-0
serialization to the first feature kernel (the stem conv), with its start offset and duration, and the geometry kernels
(site hash / block table, neighbour tables, their memsets) of all levels by grid size.  Medians over the last N forwards.
Also the span from the coordinate maximum to the level-0 codes (the host's depth read-back sits in it), the launches per
forward, and median, least and most of every lead-in kernel at its level-0 grid.
usage: python tools/trace_leadin.py <kernel_trace.csv> [num_forwards=20]"""
import collections
import csv
import statistics
import sys


def short(name):
    return name.split("(")[0].replace("void ", "").replace("ptv3::", "")[:44]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    nf = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    # a forward starts at the coordinate maximum where the executor derives the depth itself (the kernels it queues
    # between that and the level-0 serialization belong to the same forward), else at the serialization of its largest level
    top = max(int(r["Grid_Size_X"]) for r in rows if "sfc_encode" in r["Kernel_Name"])
    starts = [i for i, r in enumerate(rows) if "coord_max" in r["Kernel_Name"]][-nf:]
    if not starts:
        starts = [i for i, r in enumerate(rows) if "sfc_encode" in r["Kernel_Name"] and int(r["Grid_Size_X"]) == top][-nf:]
    forwards = [rows[a:b] for a, b in zip(starts, starts[1:] + [len(rows)])]
    walls = [(max(int(r["End_Timestamp"]) for r in f) - int(f[0]["Start_Timestamp"])) / 1e3 for f in forwards]
    print(f"{len(forwards)} forwards, wall under the profiler median {statistics.median(walls):.1f} us")
    first_gemm = min(next(i for i, r in enumerate(f) if "gemm_kernel" in r["Kernel_Name"]) for f in forwards)
    print("lead-in (median start offset / duration, us):")
    for j in range(first_gemm + 1):
        t = [(int(f[j]["Start_Timestamp"]) - int(f[0]["Start_Timestamp"])) / 1e3 for f in forwards]
        print(f"  {j:2d} {short(forwards[-1][j]['Kernel_Name']):44s} queue {forwards[-1][j]['Queue_Id']}  "
              f"start {statistics.median(t):7.1f}  dur {statistics.median(dur(f[j]) for f in forwards):6.1f}  "
              f"grid {forwards[-1][j]['Grid_Size_X']}")
    gemm0 = [(int(next(r for r in f if "gemm_kernel" in r["Kernel_Name"])["Start_Timestamp"]) -
              int(f[0]["Start_Timestamp"])) / 1e3 for f in forwards]
    print(f"forward start -> first stem-conv launch: median {statistics.median(gemm0):.1f} us")
    if "coord_max" in forwards[0][0]["Kernel_Name"]:
        # the host reads the maximum back between these two: what the GPU does not fill of this span is the host bubble
        enc = [(int(next(r for r in f if "sfc_encode" in r["Kernel_Name"])["Start_Timestamp"]) -
                int(f[0]["Start_Timestamp"])) / 1e3 for f in forwards]
        busy = [sum(dur(r) for r in f[:next(i for i, r in enumerate(f) if "sfc_encode" in r["Kernel_Name"])])
                for f in forwards]
        print(f"coord_max start -> sfc_encode start: median {statistics.median(enc):.1f} us, of which kernels "
              f"{statistics.median(busy):.1f} us")
    print(f"launches per forward: median {statistics.median(len(f) for f in forwards):.0f}")
    # the kernels of the lead-in by name: level 0 is the largest grid of each; median and min .. max over the forwards
    print("lead-in kernels at their largest grid (launches per forward, median, min .. max, us):")
    for pat in ("coord_max", "sfc_encode", "radix_hist", "radix_scatter", "make_indices", "bt_sites", "gemm_kernel"):
        sel = [r for f in forwards for r in f[:first_gemm + 1] if pat in r["Kernel_Name"]]
        if not sel:
            continue
        g = max(int(r["Grid_Size_X"]) for r in sel)
        v = [dur(r) for r in sel if int(r["Grid_Size_X"]) == g]
        print(f"  {pat:16s} grid {g:8d}  {len(v) / len(forwards):4.1f}  {statistics.median(v):6.1f}  "
              f"{min(v):6.1f} .. {max(v):6.1f}")
    geo = collections.defaultdict(list)
    for f in forwards:
        for r in f:
            n = short(r["Kernel_Name"])
            if n.startswith(("bt_", "ht_")) or "fillBuffer" in n:
                geo[n, int(r["Grid_Size_X"])].append(dur(r))
    print("geometry kernels of all levels (launches per forward, median / mean duration, us):")
    for (n, g), v in sorted(geo.items()):
        print(f"  {n:44s} grid {g:8d}  {len(v) / len(forwards):4.1f}  {statistics.median(v):6.1f} / {statistics.mean(v):6.1f}")
    print(f"  sum per forward {sum(sum(v) for v in geo.values()) / len(forwards):.1f} us")


if __name__ == "__main__":
    main()
