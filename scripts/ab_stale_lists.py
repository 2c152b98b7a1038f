#!/usr/bin/env python3
"""Interleaved A/B of env RT_BG_STALE 0 / 1 (the background tier on frames whose
light-space shadow lists are stale) in one process on one GPU: the light moves
before every frame and the lists stay deferred, so every frame's shadow rays
walk the BVH; two renderers, 10 rounds of 200 back-to-back frames after 4
warm-up rounds, the frames compared.  Prints one JSON line
(profiles/r12/ab/r12d_ab_stale_1024.json).

Usage: ab_stale_lists.py [size]"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa
from skybox_rt_amd import rt
size = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
scene = rt.Scene.load(os.path.join(ROOT, "tests/golden/scenes/tekkaman.cgltrace"))
rs = {}
for name, v in (("off", "0"), ("on", "1")):
    os.environ["RT_BG_STALE"] = v
    r = rt.Renderer(scene)
    r.configure(size, size, shadows=True, counters=False)
    r.set_list_policy(1 << 30)
    r.render()
    rs[name] = r
os.environ.pop("RT_BG_STALE")
lights = [(0.0, 60.0, 80.0), (10.0, 40.0, 60.0)]
def run(r, frames=200):
    stream = torch.cuda.ExternalStream(r.device_stream())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    r.set_timing(False)
    try:
        for i in range(3):
            r.set_light(lights[i & 1]); r.start()
        r.wait()
        e0.record(stream)
        for i in range(frames):
            r.set_light(lights[i & 1]); r.start()
        e1.record(stream)
        r.wait(); e1.synchronize()
    finally:
        r.set_timing(True)
    return e0.elapsed_time(e1) / frames
t = {n: [] for n in rs}
for rnd in range(14):
    for n, r in rs.items():
        x = run(r)
        if rnd >= 4: t[n].append(x)
out = {n: {"median_ms": round(float(np.median(v)), 5), "range_ms": round(float(max(v) - min(v)), 5),
           "rounds_ms": [round(x, 5) for x in v], "tier_groups": rs[n].setup_stats()["tier_groups"],
           "slist_stale": rs[n].setup_stats()["slist_stale"], "grid": rs[n].stats()["grid"]} for n, v in t.items()}
a, b = rs["off"].framebuffer(), rs["on"].framebuffer()
out["identical"] = bool(np.array_equal(a, b))
print(json.dumps(out))
