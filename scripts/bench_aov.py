#!/usr/bin/env python3
"""Kernel time of the visibility-record launch (image rt_aov: primary
visibility, the layer resolve and one shadow ray per light traced in place, one
16-byte record per pixel, no shading) next to the frame of the same lights, in
one process on one renderer.

Series k1: the launch under one light against the RT_RENDER_SHADOWS frame
(rt_kernel).  Series k4, k16: the launch under the first K points of
bench_lights.py's 4 x 4 grid against the K-light frame (rt_lights).  Both are
ordinary launches on their image's own grid, each started on an idle queue and
timed by its HIP events.  After `--warmup` launches of each, `--steps` rounds
alternate the two, so drift hits both alike.  Median and quartiles of each and
their ratio; they count as apart where the quartile ranges do not overlap.  At
the size timed the records are checked against the frames: rt_aov_relight of
the unshadowed frame and the masks is the K-light frame.  One JSON line for the
whole run, also written to --out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_lights import grid_lights, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tekkaman")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "aov_1024.json"))
    ap.add_argument("--kernel-dir", default=None, help="a kernel directory (an rt_aov.vxbin of its own: A/B)")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_aov needs a GPU"
    from conftest import scene_path
    from skybox_rt_amd import rt
    grid = grid_lights()
    s = rt.Scene.load(scene_path(args.scene))
    r = rt.Renderer(s, kernel_dir=args.kernel_dir)
    n = args.size
    r.configure(n, n, shadows=False, counters=False)
    r.render()
    plain = r.framebuffer()
    out = {"bench": "aov", "kernel_dir": args.kernel_dir, "scene": args.scene, "size": n, "steps": args.steps,
           "warmup": args.warmup,
           "lights": "k1: the default light (0, 60, 80); k > 1: first K of a 4x4 grid, side 20, centred on it, "
                     "plane w = 80",
           "timer": "HIP events around each launch (an ordinary launch started on an idle queue), alternating "
                    "frame / record launch",
           "series": {}}

    def frame_ms():
        r.render()
        return r.kernel_ms()

    def aov_ms():
        r.aov(wait=False)
        r.wait()
        return r.kernel_ms()

    for k in [int(x) for x in args.ks.split(",")]:
        lights = grid[:k] if k > 1 else [rt.DEFAULT_LIGHT]
        r.configure(n, n, shadows=True, light=lights[0], counters=False)
        if k > 1:
            r.set_lights(lights)
        info = r.lights_info()
        for _ in range(args.warmup):
            frame_ms()
        for _ in range(args.warmup):
            aov_ms()
        t_frame, t_aov = [], []
        for _ in range(args.steps):
            t_frame.append(frame_ms())
            t_aov.append(aov_ms())
        fb = r.framebuffer()
        rec = r.aov_records()
        sray = (rec["depth_flags"] & np.uint32(rt.RT_AOV_SHADOW_RAY)) != 0
        bits = sum(((rec["light_mask"] >> np.uint32(i)) & np.uint32(1)).astype(np.int64) for i in range(16))
        a, b = spread(t_aov), spread(t_frame)
        out["series"][f"k{k}"] = {
            "lights": k, "frame_image": "rt_kernel" if k == 1 else "rt_lights",
            "aov_launch": a, "frame": b, "aov_over_frame": round(a["median_ms"] / b["median_ms"], 4),
            "quartiles_apart": bool(a["q3_ms"] < b["q1_ms"] or b["q3_ms"] < a["q1_ms"]),
            "slist_on": [i["slist_on"] for i in info],
            "shadow_ray_pixels": int(sray.sum()), "mask_bits_set": int(bits.sum()),
            "relight_equals_frame": bool(np.array_equal(rt.aov_relight(plain, rec["light_mask"], k), fb))}
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
