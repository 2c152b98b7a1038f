#!/usr/bin/env python3
"""Kernel time of a frame lit by K point lights in one launch (image
rt_lights: primary visibility, layers, shading and texel reads once, every
queued shadow ray against each light's own shadow lists) next to the K plain
single-light frames on rt_kernel whose rounded mean it is, in one process on
one renderer.

Lights: the first K points of a fixed 4 x 4 grid, side 20, centred on the
default light, in the plane w = 80 (an area light's sample points).  After
`--warmup` rounds, `--steps` rounds alternate (a) set_lights(K) and one
K-light frame and (b) for each of the K lights set_light with its lists built
at once (list policy 0, settled) and one plain frame -- so drift hits both
alike; every frame is started on an idle queue and timed by its HIP events,
(b) is the sum of its K frames.  (b) uses only what the renderer had before
several lights.  The wall time of set_lights is reported against the K
set_light calls (each settled, as set_lights settles its sets).  Median,
quartiles and extremes of each; (a) counts as below (b) where their quartile
ranges do not overlap.  One JSON line for the whole run."""
import argparse
import json
import os
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tekkaman")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--ks", default="1,2,4,8,16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the record to this file")
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20 timed rounds per series")
    import torch
    assert torch.cuda.is_available(), "bench_lights needs a GPU"
    from conftest import scene_path
    from skybox_rt_amd import rt
    grid = grid_lights()
    s = rt.Scene.load(scene_path(args.scene))
    r = rt.Renderer(s)
    r.configure(args.size, args.size, shadows=True, light=grid[0], counters=False)
    r.set_list_policy(0)
    out = {"bench": "lights", "scene": args.scene, "size": args.size, "steps": args.steps, "warmup": args.warmup,
           "lights": "first K of a 4x4 grid, side 20, centred on (0, 60, 80), plane w = 80",
           "timer": "HIP events around each frame (started on an idle queue); single = sum of its K frames; "
                    "set_lights / set_light: host wall clock, lists settled",
           "series": {}}
    for k in [int(x) for x in args.ks.split(",")]:
        lights = grid[:k]
        t_multi, t_single, w_multi, w_single = [], [], [], []
        frames, multi = [], None
        for step in range(args.warmup + args.steps):
            t0 = time.perf_counter()
            r.set_lights(lights)
            wm = (time.perf_counter() - t0) * 1e3
            r.render()
            tm = r.kernel_ms()
            last = step == args.warmup + args.steps - 1
            if last:
                multi = r.framebuffer()
                info = r.lights_info()
            ts = ws = 0.0
            for L in lights:
                t0 = time.perf_counter()
                r.set_light(L)
                ss = r.setup_stats()  # settles the lists
                ws += (time.perf_counter() - t0) * 1e3
                assert ss["slist_on"] == 1, ss
                r.render()
                ts += r.kernel_ms()
                if last:
                    frames.append(r.framebuffer())
            if step >= args.warmup:
                t_multi.append(tm)
                t_single.append(ts)
                w_multi.append(wm)
                w_single.append(ws)
        # at the size timed: the K-light frame is the rounded mean of the K plain frames
        want = frames[0] & np.uint32(0xFF000000)
        for sh in (16, 8, 0):
            tot = sum(((c >> np.uint32(sh)) & np.uint32(0xFF)).astype(np.uint64) for c in frames)
            want = want | (((2 * tot + k) // (2 * k)).astype(np.uint32) << np.uint32(sh))
        a, b = spread(t_multi), spread(t_single)
        out["series"][f"k{k}"] = {
            "lights": k, "one_launch": a, "single_light_frames": b,
            "one_launch_over_single": round(a["median_ms"] / b["median_ms"], 4),
            "quartiles_apart": bool(a["q3_ms"] < b["q1_ms"] or b["q3_ms"] < a["q1_ms"]),
            "set_lights_wall": spread(w_multi), "set_light_x_k_wall": spread(w_single),
            "slist_on": [i["slist_on"] for i in info], "slist_entries": [i["slist_entries"] for i in info],
            "equals_mean_of_single_frames": bool(np.array_equal(multi, want)),
            "pixels_differing_between_lights": int(np.any([c != frames[0] for c in frames[1:]], axis=0).sum())
            if k > 1 else 0}
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
