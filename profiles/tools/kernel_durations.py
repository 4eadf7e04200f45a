#!/usr/bin/env python3
"""Per-dispatch durations of named kernels from a counter-free kernel trace of the graph-replayed step.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --gpus 1 --steps 6 --warmup 2
    python3 profiles/tools/kernel_durations.py DIR [TAG] [NAME ...]

For every NAME (substring of the kernel name; default: the fused heads pass and its yardsticks) the median / min / max of its
LAST six dispatches -- the timed, replayed steps; the dispatches before them are the eager warm-up and the capture -- in us.
profiles/r25_heads_small.md: five such traces each of two builds of the library, alternating on one box.
"""
import csv
import glob
import statistics
import sys


def main():
    d = sys.argv[1]
    tag = sys.argv[2] if len(sys.argv) > 2 else ""
    pats = sys.argv[3:] or ["heads_fused_kernel", "heads_small_kernel", "head_wgrad_blocked", "adam"]
    acc, total = {}, 0.0
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
                total += dur
                for p in pats:
                    if p in r["Kernel_Name"]:
                        acc.setdefault(p, []).append(dur)
    for p, v in sorted(acc.items()):
        last = v[-6:]
        print("%s %-22s n=%3d  last6: median %8.1f  min %8.1f  max %8.1f us" % (tag, p, len(v), statistics.median(last), min(last), max(last)))
    print("%s all kernels %.1f us" % (tag, total))


if __name__ == "__main__":
    main()
