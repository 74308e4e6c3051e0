#!/usr/bin/env python3
"""What a chunk's host path costs on the GPU's timeline, from one rocprofv3 run of bench.py:

    rocprofv3 --kernel-trace --memory-copy-trace --hip-trace --stats --output-format csv -d <dir> -- python3 bench.py ...
    tools/chunk_path_trace.py <dir> [steps to skip at the start, default 8]

A step is delimited by its pack_tiles_kernel dispatch.  The runtime carries the chunk's copies out with blit kernels
(__amd_rocclr_copyBuffer), which are in the kernel trace and not in the memory-copy trace, so a copy here is either: such a dispatch, or a
row of the memory-copy trace.  Per steady-state step: the copies behind packing (up to the next step's first other kernel: the downloads,
and uploads that precede the next step's first kernel) and inside the step, the dispatches of each symbolize variant, the GPU's idle time
from the end of packing to the first copy and to the bitstream copy (the longest copy behind packing), and from the last copy to the next
step's first kernel.  Medians over the steps, times in microseconds."""
import collections
import csv
import glob
import os
import statistics
import sys


def rows_of(d, suffix):
    out = []
    for p in glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True):
        out += list(csv.DictReader(open(p)))
    return out


def short_name(name):
    """the kernel's name without its argument list (stripped from the right: template arguments and `(anonymous namespace)` stay)"""
    name = name.strip()
    if name.endswith("]") and " [" in name:   # "... [clone .kd]"
        name = name[:name.rindex(" [")]
    if name.endswith(".kd"):
        name = name[:-3]
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += name[i] == ")"
            depth -= name[i] == "("
            if depth == 0:
                name = name[:i]
                break
    return name[5:] if name.startswith("void ") else name


def main():
    d = sys.argv[1]
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    every = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short_name(r["Kernel_Name"])) for r in rows_of(d, "kernel_trace.csv"))
    copies = [k for k in every if "copyBuffer" in k[2]]
    copies += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Direction", "copy")) for r in rows_of(d, "memory_copy_trace.csv")]
    copies.sort()
    kernels = [k for k in every if "copyBuffer" not in k[2]]
    packs = [k for k in kernels if "pack_tiles_kernel" in k[2]]
    if len(packs) < skip + 3:
        raise SystemExit("only %d steps in the trace" % len(packs))
    per = collections.defaultdict(list)
    names = collections.Counter()
    for i in range(skip, len(packs) - 1):
        lo, hi = packs[i - 1][1], packs[i][1]           # (end of the previous step's packing, end of this step's]
        in_step = [k for k in kernels if lo < k[0] <= hi]
        for k in in_step:
            names[k[2][:110]] += 1
        first = in_step[0][0]
        nxt = [k for k in kernels if k[0] >= hi]
        first_next = nxt[0][0] if nxt else packs[i + 1][0]
        inside = [c for c in copies if first <= c[0] < hi]
        behind = [c for c in copies if hi <= c[0] < first_next]
        per["copies inside the step"].append(len(inside))
        per["copies behind packing, before the next step's first kernel"].append(len(behind))
        per["dispatches symbolize<true,...>"].append(sum(1 for k in in_step if "symbolize_tile_kernel<true" in k[2]))
        per["dispatches symbolize<false,...>"].append(sum(1 for k in in_step if "symbolize_tile_kernel<false" in k[2]))
        per["kernel dispatches (without copies)"].append(len(in_step))
        if behind:
            big = max(behind, key=lambda c: c[1] - c[0])
            per["idle: packing end -> first copy start"].append((behind[0][0] - hi) / 1e3)
            per["packing end -> bitstream copy start"].append((big[0] - hi) / 1e3)
            per["bitstream copy duration"].append((big[1] - big[0]) / 1e3)
            per["packing end -> last copy end"].append((max(c[1] for c in behind) - hi) / 1e3)
            per["idle: last copy end -> next step's first kernel"].append((first_next - max(c[1] for c in behind)) / 1e3)
            per["packing end -> next step's first kernel"].append((first_next - hi) / 1e3)
        per["step period (packing end to packing end)"].append((hi - lo) / 1e3)
    n = len(per["step period (packing end to packing end)"])
    print("%d steady-state steps (the first %d skipped)" % (n, skip))
    for k, v in per.items():
        print("  %-62s median %9.2f   min %9.2f   max %9.2f" % (k, statistics.median(v), min(v), max(v)))
    print("kernels per step (without copies):")
    for k, v in sorted(names.items(), key=lambda kv: -kv[1]):
        print("  %6.2f  %s" % (v / n, k))


if __name__ == "__main__":
    main()
