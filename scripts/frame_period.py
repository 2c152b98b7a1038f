#!/usr/bin/env python3
"""Frame boundary account from a rocprofv3 --kernel-trace CSV: for the
consecutive dispatches of one kernel (default vx_main_rt_kernel) inside every
back-to-back run of them, the begin-to-begin period, the end-to-begin gap
(negative when two dispatches overlap), the duration, and the queues the
dispatches ran on.  Prints one JSON object; the timed region of the bench
command is the run of exactly --steps dispatches (the longest runs are the
synchronous frames and the kernel clock).

Usage: frame_period.py <kernel_trace.csv | directory> [--kernel NAME] [--steps N]"""
import argparse
import csv
import glob
import gzip
import json
import os
import statistics
import sys


def find_trace(path):
    if os.path.isfile(path):
        return path
    hits = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv*"), recursive=True))
    if not hits:
        sys.exit(f"no *kernel_trace.csv under {path}")
    return hits[0]


def runs_of(rows, kname, max_gap_ns):
    """Runs of consecutive `kname` dispatches (by start time) with no other
    kernel between them and no idle gap of max_gap_ns or more."""
    runs, run, end = [], [], 0
    for st, en, nm, q in rows + [(0, 0, "", "")]:
        if nm == kname and (not run or st - end < max_gap_ns):
            run.append((st, en, q))
            end = max(end, en)
            continue
        if len(run) >= 2:
            runs.append(run)
        run, end = ([(st, en, q)], en) if nm == kname else ([], 0)
    return runs


def account(run):
    per = [b[0] - a[0] for a, b in zip(run, run[1:])]
    gap = [b[0] - a[1] for a, b in zip(run, run[1:])]
    dur = [en - st for st, en, _ in run]
    s = lambda v: {"mean": round(statistics.fmean(v) * 1e-3, 3), "median": round(statistics.median(v) * 1e-3, 3),  # noqa: E731
                   "min": round(min(v) * 1e-3, 3), "max": round(max(v) * 1e-3, 3)}
    return {"dispatches": len(run), "queues": sorted({q for _, _, q in run}),
            "span_per_frame_us": round((max(e for _, e, _ in run) - run[0][0]) / len(run) * 1e-3, 3),
            "period_us": s(per), "end_to_begin_gap_us": s(gap), "duration_us": s(dur),
            "overlapping_pairs": sum(1 for g in gap if g < 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--kernel", default="vx_main_rt_kernel")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--max-gap-us", type=float, default=100.0)
    a = ap.parse_args()
    path = find_trace(a.trace)
    f = gzip.open(path, "rt") if path.endswith(".gz") else open(path)
    rows = sorted(((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"],
                    str(r.get("Queue_Id", ""))) for r in csv.DictReader(f)), key=lambda t: t[0])
    runs = runs_of(rows, a.kernel, int(a.max_gap_us * 1e3))
    out = {"trace": os.path.basename(path), "kernel": a.kernel, "runs": len(runs),
           "timed_region": None, "longest_run": None}
    timed = [r for r in runs if len(r) == a.steps]
    if timed:
        out["timed_region"] = account(timed[0])
    if runs:
        out["longest_run"] = account(max(runs, key=len))
    out["run_lengths"] = [len(r) for r in runs][:40]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
