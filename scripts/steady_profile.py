#!/usr/bin/env python3
"""Steady-state kernel table from a rocprofv3 kernel trace of bench.py,
in the format of profiles/*_steady.txt.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run \\
        -- python bench.py --gpus 1 --steps 10 --warmup 4
    python scripts/steady_profile.py DIR --title "..." > profiles/x.txt

A step starts at each dispatch of the marker kernel (the 3->4 channel
pad, the first kernel of a step). The table is the mean over the last
STEPS complete steps before the last marker."""
import argparse
import collections
import csv
import glob
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--title", default="")
    ap.add_argument("--marker", default="k_pad_ch3to4_nhwc")
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    files = glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"),
                      recursive=True)
    if len(files) != 1:
        sys.exit("expected one *kernel_trace.csv under %s, found %r"
                 % (args.dir, files))
    rows = []
    with open(files[0], newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "elementwise_kernel_manual_unroll" in name:
                name = name[:64] + " grid=" + r.get("Grid_Size_X",
                                                    r.get("Grid_Size", "?"))
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                         name))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if args.marker in r[2]]
    if len(marks) < args.steps + 1:
        sys.exit("only %d marker dispatches" % len(marks))
    lo, hi = marks[-1 - args.steps], marks[-1]
    win = rows[lo:hi]
    k = float(args.steps)
    wall = (rows[hi][0] - rows[lo][0]) / 1e6 / k
    busy = sum(e - s for s, e, _ in win) / 1e6 / k
    cnt = collections.Counter()
    ms = collections.Counter()
    for s, e, name in win:
        cnt[name] += 1
        ms[name] += (e - s) / 1e6
    if args.title:
        print(args.title)
    print("steady state, mean of %d steps: wall %.3f ms/step, GPU-busy "
          "%.3f ms/step, %.1f dispatches/step"
          % (args.steps, wall, busy, len(win) / k))
    print("%-100s %8s %9s" % ("kernel", "n/step", "ms/step"))
    for name, t in sorted(ms.items(), key=lambda kv: -kv[1]):
        print("%-100s %8.1f %9.4f" % (name[:100], cnt[name] / k, t / k))


if __name__ == "__main__":
    main()
