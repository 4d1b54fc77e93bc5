"""The resident-window attention launches of a forward from a rocprofv3 --kernel-trace CSV of `bench.py`: every
`window_attn_full_kernel` launch in the order of the forward with its template variant (RPE mode, QT), grid and
duration (median, least, most over the last N forwards), the sum per variant and the family's time per forward (median
and least .. most of the per-forward sums: the spread an item's effect is held against).
usage: python tools/trace_attn.py <kernel_trace.csv> [num_forwards=20]"""
import collections
import csv
import re
import statistics
import sys


def variant(name):
    """'rpeR,qtQ' from the last two template arguments (the profiler's demangler garbles the ones in front for bf16)"""
    m = re.search(r"window_attn_full_kernel<([^>]*)>", name)
    if m:
        args = [a.strip().split(")")[-1] for a in m.group(1).split(",")]
        return f"rpe{args[-2]},qt{args[-1]}"
    m = re.search(r"window_attn_full_kernelI\w*?Li\d+ELi(\d+)ELi(\d+)E", name)
    return f"rpe{m.group(1)},qt{m.group(2)}" if m else "?"


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    nf = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    top = max(int(r["Grid_Size_X"]) for r in rows if "sfc_encode" in r["Kernel_Name"])
    starts = [i for i, r in enumerate(rows) if "coord_max" in r["Kernel_Name"]]
    if not starts:
        starts = [i for i, r in enumerate(rows) if "sfc_encode" in r["Kernel_Name"] and int(r["Grid_Size_X"]) == top]
    forwards = [rows[a:b] for a, b in zip(starts, starts[1:] + [len(rows)])][-nf:]
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    attn = [[r for r in f if "window_attn_full_kernel" in r["Kernel_Name"]] for f in forwards]
    n = len(attn[-1])
    attn = [a for a in attn if len(a) == n]
    allk = [sum(dur(r) for r in f) for f in forwards]
    print(f"{len(attn)} forwards of {n} attention launches; all kernels per forward: median {statistics.median(allk):.1f} us")
    per_var = collections.defaultdict(list)
    print(" #  variant   workgroups  threads   median    least     most  (us)")
    for j in range(n):
        d = [dur(a[j]) for a in attn]
        r = attn[-1][j]
        wg, th = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_X"])
        print(f"{j:2d}  {variant(r['Kernel_Name']):8s}  {wg:10d}  {th:7d}  {statistics.median(d):7.1f}  {min(d):7.1f}  {max(d):7.1f}")
        per_var[variant(r["Kernel_Name"])].append(d)
    tot = [sum(dur(r) for r in a) for a in attn]
    for v, ds in per_var.items():
        s = [sum(x) for x in zip(*ds)]
        print(f"variant {v}: {len(ds)} launches, per forward median {statistics.median(s):.1f} us ({min(s):.1f} .. {max(s):.1f})")
    print(f"family per forward: median {statistics.median(tot):.1f} us ({min(tot):.1f} .. {max(tot):.1f}), "
          f"spread {max(tot) - min(tot):.1f}")


if __name__ == "__main__":
    main()
