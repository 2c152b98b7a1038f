#!/usr/bin/env python3
"""Kernel time of progressive path tracing (image pt_accum: k samples of every
path in one launch over one primary pass, per-pixel running sums on the
device) next to the same number of plain path frames on pt_kernel, in one
process on one renderer.

The renderer is configured once (path frame, counters off) and accumulation
begun; after `--warmup` launches of each kind, `--steps` rounds alternate
(a) one accumulation launch of k samples and (b) k plain frames (so drift hits
both alike), each launch started on an idle queue and timed by its HIP events;
(b) is the sum of its k launches.  Series: k = 8, and k = 1 against one plain
frame -- the cost of the record's read-modify-write (32 B per pixel and
launch).  The accumulation launches are steady-state ones (they read their
records; the sample cursor moves on, so their seeds differ round by round,
the plain frames' seed stays).  Median, quartiles and extremes of each, and
the ratio of the medians.  One JSON line for the whole run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(ms):
    a = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(a, (25, 50, 75))
    return {"median_ms": round(float(med), 5), "q1_ms": round(float(q1), 5), "q3_ms": round(float(q3), 5),
            "min_ms": round(float(a.min()), 5), "max_ms": round(float(a.max()), 5), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tekkaman")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--ks", default="8,1")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20 timed rounds per series")
    import torch
    assert torch.cuda.is_available(), "bench_accum needs a GPU"
    from conftest import scene_path
    from skybox_rt_amd import rt
    s = rt.Scene.load(scene_path(args.scene))
    r = rt.Renderer(s)
    r.configure(args.size, args.size, path=True, bounces=args.bounces, counters=False)
    r.accum_begin()
    out = {"bench": "accum", "scene": args.scene, "size": args.size, "bounces": args.bounces,
           "steps": args.steps, "warmup": args.warmup,
           "timer": "HIP events around each launch (started on an idle queue); plain = sum of its k launches",
           "record_bytes_per_launch": 2 * 16 * args.size * args.size, "series": {}}
    for k in [int(x) for x in args.ks.split(",")]:
        r.accum_reset()
        for _ in range(args.warmup):
            r.accumulate(k)
            r.render()
        t_acc, t_plain = [], []
        for _ in range(args.steps):
            r.accumulate(k)
            t_acc.append(r.kernel_ms())
            t = 0.0
            for _ in range(k):
                r.render()
                t += r.kernel_ms()
            t_plain.append(t)
        a, b = spread(t_acc), spread(t_plain)
        out["series"][f"k{k}"] = {"samples_per_launch": k, "accumulate": a, "plain_frames": b,
                                  "accumulate_over_plain": round(a["median_ms"] / b["median_ms"], 4),
                                  "accumulate_ms_per_sample": round(a["median_ms"] / k, 5),
                                  "plain_ms_per_frame": round(b["median_ms"] / k, 5),
                                  "samples_accumulated": r.accum_samples()}
    # at the size timed: one accumulated sample is the plain frame, records included
    r.accum_reset()
    r.accumulate(1)
    fb, rec = r.framebuffer(), r.accum()
    r.render()
    plain = r.framebuffer()
    out["one_sample_equals_plain_frame"] = bool(
        np.array_equal(fb, plain) and np.array_equal(rec[..., 3], np.ones_like(plain)) and
        np.array_equal(rec[..., 0] << 16 | rec[..., 1] << 8 | rec[..., 2], plain & 0xFFFFFF))
    r.close()
    s.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
