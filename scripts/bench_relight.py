#!/usr/bin/env python3
"""Kernel time of relighting from the visibility records next to the frame it
replaces, in one process on one renderer: the K-light frame (unchanged code: the
yardstick -- rt_kernel under one light, rt_lights under several), the capture
launch (image rt_aov_base: rt_aov's records plus the unshadowed colour per pixel)
and the relight launch (image rt_relight: a streaming pass over records and base
colours into the framebuffer).

Series k1: the default light.  Series k4, k16: the first K points of
bench_lights.py's 4 x 4 grid.  All three are ordinary launches on their image's
own grid, each started on an idle queue and timed by the driver as bench_aov.py's
are.  After `--warmup` launches of each, `--steps` rounds run frame, capture and
relight in turn, so drift hits all alike.  Median and quartiles of each; two
count as apart where their quartile ranges do not overlap.  The relight launch's
bytes -- 24 B per pixel: the 16-B record and the 4-B base colour in, 4 B out --
over its time, against the 8 TB/s peak of the memory; the capture against the sum
of an rt_aov launch and a single-light frame, both timed in the same rounds.  At
the size timed the relit frame under unit weights is checked against the K-light
frame, and under a ramp of weights against the host's restatement.  One JSON line
for the whole run, also written to --out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_lights import grid_lights, spread  # noqa: E402

PEAK_TBS = 8.0
BYTES_PER_PIXEL = 24


def apart(a, b):
    return bool(a["q3_ms"] < b["q1_ms"] or b["q3_ms"] < a["q1_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tekkaman")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "relight_1024.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_relight needs a GPU"
    from conftest import scene_path
    from skybox_rt_amd import rt
    grid = grid_lights()
    s = rt.Scene.load(scene_path(args.scene))
    r = rt.Renderer(s)
    n = args.size
    out = {"bench": "relight", "scene": args.scene, "size": n, "steps": args.steps, "warmup": args.warmup,
           "lights": "k1: the default light (0, 60, 80); k > 1: first K of a 4x4 grid, side 20, centred on it, "
                     "plane w = 80",
           "timer": "the driver's time of each launch (an ordinary launch started on an idle queue), in rounds of "
                    "frame / capture / relight (/ rt_aov launch)",
           "relight_bytes_per_pixel": BYTES_PER_PIXEL, "peak_TBps": PEAK_TBS, "series": {}}

    def timed(fn, *a):
        fn(*a)
        r.wait()
        return r.kernel_ms()

    # the single-light frame the capture is held against (with the rt_aov launch of each series)
    r.configure(n, n, shadows=True, light=rt.DEFAULT_LIGHT, counters=False)
    for _ in range(args.warmup):
        timed(r.render)
    single = spread([timed(r.render) for _ in range(args.steps)])
    out["single_light_frame"] = single

    for k in [int(x) for x in args.ks.split(",")]:
        lights = grid[:k] if k > 1 else [rt.DEFAULT_LIGHT]
        ones = [1] * k
        ramp = [1 + (254 * i) // max(k - 1, 1) for i in range(k)]
        r.configure(n, n, shadows=True, light=lights[0], counters=False)
        if k > 1:
            r.set_lights(lights)
        r.relight_capture()
        for fn, a in ((r.render, ()), (r.relight_capture, (False,)), (r.relight, (ones, False)), (r.aov, (False,))):
            for _ in range(args.warmup):
                timed(fn, *a)
        t = {"frame": [], "capture": [], "relight": [], "aov": []}
        for i in range(args.steps):
            t["frame"].append(timed(r.render))
            t["capture"].append(timed(r.relight_capture, False))
            t["relight"].append(timed(r.relight, ones if i % 2 == 0 else ramp, False))
            t["aov"].append(timed(r.aov, False))
        r.render()
        frame = r.framebuffer().copy()
        r.relight(ones)
        unit_ok = bool(np.array_equal(r.framebuffer(), frame))
        r.relight(ramp)
        rec = r.aov_records()
        ramp_ok = bool(np.array_equal(r.framebuffer(), rt.relight_resolve(r.relight_base(), rec["depth_flags"],
                                                                          rec["light_mask"], ramp)))
        sp = {key: spread(v) for key, v in t.items()}
        rel_s = sp["relight"]["median_ms"] * 1e-3
        cap_ref = sp["aov"]["median_ms"] + single["median_ms"]
        out["series"][f"k{k}"] = {
            "lights": k, "frame_image": "rt_kernel" if k == 1 else "rt_lights",
            "frame": sp["frame"], "capture_launch": sp["capture"], "relight_launch": sp["relight"],
            "aov_launch": sp["aov"],
            "relight_over_frame": round(sp["relight"]["median_ms"] / sp["frame"]["median_ms"], 4),
            "relight_below_frame_quartiles_apart": bool(sp["relight"]["q3_ms"] < sp["frame"]["q1_ms"]),
            "relight_TBps": round(BYTES_PER_PIXEL * n * n / rel_s * 1e-12, 3),
            "relight_share_of_peak": round(BYTES_PER_PIXEL * n * n / rel_s * 1e-12 / PEAK_TBS, 4),
            "capture_over_aov_plus_single_frame": round(sp["capture"]["median_ms"] / cap_ref, 4),
            "capture_over_frame": round(sp["capture"]["median_ms"] / sp["frame"]["median_ms"], 4),
            "capture_frame_quartiles_apart": apart(sp["capture"], sp["frame"]),
            "unit_weights_equal_frame": unit_ok, "ramp_equals_host_resolve": ramp_ok}
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
