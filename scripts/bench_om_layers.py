#!/usr/bin/env python3
"""Kernel time of the ordered-tail RT frame (rt_om_kernel.hip: head traced,
blended / stencil / masked drawcalls folded through the output merger) next
to the raster pipeline's frame (raster_kernel.hip) of the same scene -- the
only other way to render these scenes -- in one process, plain frames.

Per scene: both renderers configured once, a warm-up of each, then `--steps`
rounds that render one frame of each in turn (so drift hits both alike) and
read the launch's HIP-event time; median, quartiles and extremes of each, and
whether the two frames are equal.  One JSON line for the whole run."""
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
    ap.add_argument("--scenes", default="vase,evilskull")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error("--steps: at least 20 timed frames per path")
    import torch
    assert torch.cuda.is_available(), "bench_om_layers needs a GPU"
    from conftest import scene_path
    from skybox_rt_amd import rt
    out = {"bench": "om_layers", "size": args.size, "steps": args.steps, "warmup": args.warmup,
           "timer": "HIP events around the frame's launch", "scenes": {}}
    for name in args.scenes.split(","):
        s_om = rt.Scene.load(scene_path(name), om_layers=True)
        s_ra = rt.Scene.load(scene_path(name))
        r_om, r_ra = rt.Renderer(s_om), rt.Renderer(s_ra)
        r_om.configure(args.size, args.size, shadows=False, counters=False)
        r_ra.configure(args.size, args.size, shadows=False, raster=True, counters=False)
        for _ in range(args.warmup):
            r_om.render()
            r_ra.render()
        t_om, t_ra = [], []
        for _ in range(args.steps):
            r_om.render()
            t_om.append(r_om.kernel_ms())
            r_ra.render()
            t_ra.append(r_ra.kernel_ms())
        equal = bool(np.array_equal(r_om.framebuffer(), r_ra.framebuffer()))
        k, n = s_om.om_split()
        a, b = spread(t_om), spread(t_ra)
        out["scenes"][name] = {"first_tail_drawcall": k, "tail_prims": n, "rt_om": a, "raster": b,
                               "raster_over_rt_om": round(b["median_ms"] / a["median_ms"], 3),
                               "frames_equal": equal}
        r_om.close()
        r_ra.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
