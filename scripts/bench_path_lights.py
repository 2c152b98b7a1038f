#!/usr/bin/env python3
"""Kernel time of a path-traced frame lit by K point lights in one launch
(image pt_lights: every bounce ray once, at each path vertex one shadow ray per
light on that light's own shadow lists) next to the K plain single-light path
frames on pt_kernel whose rounded mean it is, in one process on one renderer.

Lights: the first K points of a fixed 4 x 4 grid, side 20, centred on the
default light, in the plane w = 80 (scripts/bench_lights.py's).  After
`--warmup` rounds, `--steps` rounds alternate (a) set_path_lights(K) and one
K-light frame and (b) for each of the K lights set_light with its lists built
at once (list policy 0, settled) and one plain path frame -- so drift hits both
alike; every frame is started on an idle queue and timed by its HIP events,
(b) is the sum of its K frames.  (b) uses only what the renderer had before
several lights.  One more series: accumulate(S) under `--accum-lights` lights
(image pt_lights_accum, one launch) against the host loop it replaces -- per
light set_light and accumulate(S) on pt_accum, the sum of the launches.
Median, quartiles and extremes of each; (a) counts as below (b) where their
quartile ranges do not overlap.  One JSON line for the whole run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def grid_lights(centre=(0.0, 60.0, 80.0), side=20.0, n=4):
    return [(centre[0] - side / 2 + side * i / (n - 1), centre[1] - side / 2 + side * j / (n - 1), centre[2])
            for j in range(n) for i in range(n)]


def spread(ms):
    a = np.asarray(ms, np.float64)
    q1, med, q3 = np.percentile(a, (25, 50, 75))
    return {"median_ms": round(float(med), 5), "q1_ms": round(float(q1), 5), "q3_ms": round(float(q3), 5),
            "min_ms": round(float(a.min()), 5), "max_ms": round(float(a.max()), 5), "n": int(a.size)}


def compare(a, b):
    return {"one_launch": a, "single_light_frames": b,
            "one_launch_over_single": round(a["median_ms"] / b["median_ms"], 4),
            "quartiles_apart": bool(a["q3_ms"] < b["q1_ms"] or b["q3_ms"] < a["q1_ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tekkaman")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--accum-lights", type=int, default=4)
    ap.add_argument("--accum-samples", type=int, default=8)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the record to this file")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20 timed rounds per series")
    import torch
    assert torch.cuda.is_available(), "bench_path_lights needs a GPU"
    from conftest import scene_path
    from skybox_rt_amd import rt
    grid = grid_lights()
    s = rt.Scene.load(scene_path(args.scene))
    r = rt.Renderer(s)
    r.configure(args.size, args.size, path=True, bounces=args.bounces, light=grid[0], counters=False)
    r.set_list_policy(0)
    out = {"bench": "path_lights", "scene": args.scene, "size": args.size, "bounces": args.bounces,
           "steps": args.steps, "warmup": args.warmup,
           "lights": "first K of a 4x4 grid, side 20, centred on (0, 60, 80), plane w = 80",
           "timer": "HIP events around each launch (started on an idle queue); single = sum of its K launches",
           "series": {}}
    rounds = args.warmup + args.steps
    for k in [int(x) for x in args.ks.split(",")]:
        lights = grid[:k]
        t_multi, t_single = [], []
        frames, multi = [], None
        for step in range(rounds):
            r.set_path_lights(lights)
            r.render()
            tm = r.kernel_ms()
            last = step == rounds - 1
            if last:
                multi = r.framebuffer()
                info = r.lights_info()
            ts = 0.0
            for L in lights:
                r.set_light(L)
                ss = r.setup_stats()  # settles the lists
                assert ss["slist_on"] == 1, ss
                r.render()
                ts += r.kernel_ms()
                if last:
                    frames.append(r.framebuffer())
            if step >= args.warmup:
                t_multi.append(tm)
                t_single.append(ts)
        # at the size timed: the K-light frame is the rounded mean of the K plain frames
        want = frames[0] & np.uint32(0xFF000000)
        for sh in (16, 8, 0):
            tot = sum(((c >> np.uint32(sh)) & np.uint32(0xFF)).astype(np.uint64) for c in frames)
            want = want | (((2 * tot + k) // (2 * k)).astype(np.uint32) << np.uint32(sh))
        rec = compare(spread(t_multi), spread(t_single))
        rec.update({"lights": k, "slist_entries": [i["slist_entries"] for i in info],
                    "equals_mean_of_single_frames": bool(np.array_equal(multi, want)),
                    "pixels_differing_between_lights": int(np.any([c != frames[0] for c in frames[1:]], axis=0).sum())
                    if k > 1 else 0})
        out["series"][f"k{k}"] = rec
    # accumulation: S samples under K lights in one launch against the K launches of the host loop
    k, ns = args.accum_lights, args.accum_samples
    lights = grid[:k]
    r.accum_begin()
    t_multi, t_single = [], []
    for step in range(rounds):
        r.set_path_lights(lights)  # (starts the records over)
        r.accumulate(ns)
        tm = r.kernel_ms()
        ts = 0.0
        for L in lights:
            r.set_light(L)
            ss = r.setup_stats()
            assert ss["slist_on"] == 1, ss
            r.accumulate(ns)
            ts += r.kernel_ms()
        if step >= args.warmup:
            t_multi.append(tm)
            t_single.append(ts)
    rec = compare(spread(t_multi), spread(t_single))
    rec.update({"lights": k, "samples": ns})
    out["series"][f"accumulate{ns}_k{k}"] = rec
    r.close()
    s.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
