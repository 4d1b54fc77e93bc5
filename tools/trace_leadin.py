"""Lead-in of a forward from a rocprofv3 --kernel-trace CSV of plain `bench.py`: every launch from the level-0
serialization to the first level-0 block kernel (the first launch of the feature stream behind the stem conv, which waits
for the level's geometry), with its start offset and duration, the stem conv's start and end, and the geometry kernels
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
    # the stem conv: its own kernel where the build has one, else the first tile GEMM of the forward
    stem_pat = "stem_conv_kernel" if any("stem_conv_kernel" in r["Kernel_Name"] for r in forwards[-1]) else "gemm_kernel"
    stem_at = lambda f: next(i for i, r in enumerate(f) if stem_pat in r["Kernel_Name"])  # noqa: E731
    # the first level-0 block kernel: the next launch on the stem's queue (the feature stream)
    block_at = lambda f: next(i for i in range(stem_at(f) + 1, len(f)) if f[i]["Queue_Id"] == f[stem_at(f)]["Queue_Id"])  # noqa: E731
    first_gemm = min(block_at(f) for f in forwards)
    print("lead-in (median start offset / duration, us):")
    # a launch is named by its kernel and its occurrence in the forward, not by its position: the two streams interleave
    # differently from forward to forward once the stem conv runs beside the sort
    def keyed(f):
        seen, out = collections.Counter(), {}
        for r in f[:block_at(f) + 1]:
            seen[r["Kernel_Name"]] += 1
            out[r["Kernel_Name"], seen[r["Kernel_Name"]]] = r
        return out
    per = [keyed(f) for f in forwards]
    for j, (key, last) in enumerate(per[-1].items()):
        hit = [(k[key], f) for k, f in zip(per, forwards) if key in k]
        t = [(int(r["Start_Timestamp"]) - int(f[0]["Start_Timestamp"])) / 1e3 for r, f in hit]
        print(f"  {j:2d} {short(last['Kernel_Name']):44s} queue {last['Queue_Id']}  "
              f"start {statistics.median(t):7.1f}  dur {statistics.median(dur(r) for r, _ in hit):6.1f}  "
              f"grid {last['Grid_Size_X']}")
    off = lambda f, i, key: (int(f[i][key]) - int(f[0]["Start_Timestamp"])) / 1e3  # noqa: E731
    gemm0 = [off(f, stem_at(f), "Start_Timestamp") for f in forwards]
    stem_end = [off(f, stem_at(f), "End_Timestamp") for f in forwards]
    block0 = [off(f, block_at(f), "Start_Timestamp") for f in forwards]
    print(f"forward start -> first stem-conv launch: median {statistics.median(gemm0):.1f} us")
    print(f"stem conv ({stem_pat}): start {statistics.median(gemm0):.1f}, end {statistics.median(stem_end):.1f} us")
    print(f"forward start -> first level-0 block kernel ({short(forwards[-1][block_at(forwards[-1])]['Kernel_Name'])}): "
          f"median {statistics.median(block0):.1f} us, {min(block0):.1f} .. {max(block0):.1f} "
          f"(spread {max(block0) - min(block0):.1f})")
    if "coord_max" in forwards[0][0]["Kernel_Name"]:
        # the host reads the maximum back between these two: what the GPU does not fill of this span is the host bubble
        enc = [(int(next(r for r in f if "sfc_encode" in r["Kernel_Name"])["Start_Timestamp"]) -
                int(f[0]["Start_Timestamp"])) / 1e3 for f in forwards]
        busy = [sum(dur(r) for r in f[:next(i for i, r in enumerate(f) if "sfc_encode" in r["Kernel_Name"])]
                    if r["Queue_Id"] == f[0]["Queue_Id"]) for f in forwards]   # the geometry stream's own kernels
        print(f"coord_max start -> sfc_encode start: median {statistics.median(enc):.1f} us, of which kernels "
              f"{statistics.median(busy):.1f} us")
    print(f"launches per forward: median {statistics.median(len(f) for f in forwards):.0f}")
    # the kernels of the lead-in by name: level 0 is the largest grid of each; median and min .. max over the forwards
    print("lead-in kernels at their largest grid (launches per forward, median, min .. max, us):")
    for pat in ("coord_max", "sfc_encode", "radix_hist", "radix_scatter", "make_indices", "bt_sites", "bt_claim", "bt_base",
                "bt_payload", ("bt_neighbors_kernel<5", "bt_neighbors_kernelILi5E"),
                ("bt_neighbors_kernel<3", "bt_neighbors_kernelILi3E"), "window_plan", stem_pat):
        alts = pat if isinstance(pat, tuple) else (pat,)   # a template argument, demangled or not
        pat = alts[0]
        sel = [r for f in forwards for r in f[:first_gemm + 1] if any(a in r["Kernel_Name"] for a in alts)]
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
