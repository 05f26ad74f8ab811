#!/usr/bin/env python3
"""How many solve launches really run side by side: read from a kernel trace of the benchmark.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python bench.py --gpus 1 --steps 96 --warmup 8
    python scripts/queue_regime.py [--steps 96] [--label TEXT] DIR-or-kernel_trace.csv ...

For every trace: the durations of the solve kernel in the timed region (its last `--steps` dispatches), the mean number of solve kernels
running at once, the share of the region's wall time with fewer than 2, 3 and 4 of them running, the hardware queues the dispatches
used, and what the small kernels around a solve launch (the two launch-order kernels, share_init_kernel) cost: their own time and the
time from the end of the kernel before them on their queue to their own end (what they add to that queue's chain).
profiles/r10_queue_regime.txt is this script's output.
"""
import argparse
import csv
import glob
import os
import sys

import numpy as np


def find_trace(path):
    if os.path.isfile(path):
        return path
    hits = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    if not hits:
        raise SystemExit("no *kernel_trace.csv under %s" % path)
    return hits[-1]


def read_trace(path):
    rows = []
    for r in csv.DictReader(open(path)):
        rows.append((r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?")))
    rows.sort(key=lambda r: r[1])
    return rows


def pct(a, q):
    return float(np.percentile(a, q))


def running_at_once(intervals, t0, t1):
    """Sweep over [t0, t1): time spent with k intervals open, k = 0, 1, ..."""
    ev = []
    for s, e in intervals:
        s, e = max(s, t0), min(e, t1)
        if e > s:
            ev.append((s, 1))
            ev.append((e, -1))
    ev.sort()
    at = {}
    k, t = 0, t0
    for x, d in ev:
        at[k] = at.get(k, 0) + (x - t)
        k, t = k + d, x
    at[k] = at.get(k, 0) + (t1 - t)
    return at


def report(path, steps, label, out):
    rows = read_trace(path)
    solve = [r for r in rows if "solve_kernel" in r[0]]
    if len(solve) < steps:
        raise SystemExit("%s: %d solve dispatches, fewer than --steps %d" % (path, len(solve), steps))
    timed = solve[-steps:]
    t0, t1 = timed[0][1], max(r[2] for r in timed)
    wall = t1 - t0
    dur = np.array([r[2] - r[1] for r in timed]) / 1e6
    name = timed[0][0].split("(")[0].replace("void ", "")
    print("== %s" % (label or path), file=out)
    print("kernel: %s; %d dispatches in the timed region, on %d hardware queue(s); %d solve dispatches in the whole trace"
          % (name, steps, len({r[3] for r in timed}), len(solve)), file=out)
    print("timed region (first start to last end): %.2f ms = %.3f ms per step" % (wall / 1e6, wall / 1e6 / steps), file=out)
    print("solve kernel duration, ms: min %.2f  p10 %.2f  median %.2f  mean %.2f  p90 %.2f  max %.2f   (mean / step time: %.1f)"
          % (dur.min(), pct(dur, 10), pct(dur, 50), dur.mean(), pct(dur, 90), dur.max(), dur.mean() / (wall / 1e6 / steps)), file=out)
    at = running_at_once([(r[1], r[2]) for r in timed], t0, t1)
    mean = sum(k * v for k, v in at.items()) / wall
    print("solve kernels running at once: mean %.2f; share of the wall time with k running: %s"
          % (mean, "  ".join("%d: %.1f %%" % (k, 100.0 * at[k] / wall) for k in sorted(at))), file=out)
    for lim in (2, 3, 4):
        print("  fewer than %d running: %.1f %% of the wall time" % (lim, 100.0 * sum(v for k, v in at.items() if k < lim) / wall), file=out)
    # the small kernels around a solve launch, inside the timed region
    by_queue = {}
    for r in rows:
        by_queue.setdefault(r[3], []).append(r)
    for key in ("order_hist_kernel", "order_scatter_kernel", "share_init_kernel"):
        own, chain = [], []
        for q in by_queue.values():
            for i, r in enumerate(q):
                if key in r[0] and t0 <= r[1] < t1:
                    own.append(r[2] - r[1])
                    prev_end = max((p[2] for p in q[:i]), default=r[1])
                    chain.append(r[2] - max(prev_end, t0))
        if own:
            print("%s: %d dispatches in the timed region; own time mean %.1f us (max %.1f); from the end of the kernel before it on its queue to "
                  "its own end: mean %.1f us (max %.1f), %.2f %% of the wall time in all if it were all serial"
                  % (key, len(own), np.mean(own) / 1e3, np.max(own) / 1e3, np.mean(chain) / 1e3, np.max(chain) / 1e3, 100.0 * sum(chain) / wall), file=out)
        else:
            print("%s: no dispatch in the timed region" % key, file=out)
    print(file=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--label", action="append", default=[])
    ap.add_argument("traces", nargs="+")
    a = ap.parse_args()
    for i, t in enumerate(a.traces):
        report(find_trace(t), a.steps, a.label[i] if i < len(a.label) else None, sys.stdout)


if __name__ == "__main__":
    main()
