#!/usr/bin/env python3
"""Kernel time of ambient occlusion from the visibility records, in one process:
the tracing launch ao(S) (image rt_ao) for S = 1, 8, 64 at radius inf and 8, next
to the yardstick -- the only way to such rays before it: accumulate(S) of a
one-bounce path frame (image pt_accum), S = 1 and 8, which traces the same
first-bounce rays as closest-hit walks, shades them and adds two shadow rays per
sample -- and the two resolve launches (image rt_ao_resolve: grey 8 B a pixel,
modulate 28 B) next to the relight launch (image rt_relight, 24 B a pixel).

All are ordinary launches on their image's own grid, each started on an idle
queue and timed by the driver as bench_relight.py's are.  After `--warmup`
launches of each, `--steps` rounds run them in turn, so drift hits all alike.
Median and quartiles of each; two count as apart where their quartile ranges do
not overlap.  Every tracing launch of a series resets, so each traces the same
samples.

--ab DIRS (comma-separated kernel directories under lib/variants; default
ao_w1,ao_w4,ao_packet: a block's rounds on 1 or 4 waves in place of the shipped
2, and the 1-wave image built with RT_AO_PACKET, the wave's packet walk in place
of the per-lane walk, to be held against ao_w1): one
more renderer per directory runs the same tracing launches in the same rounds;
its counts must equal the first renderer's.

At the size timed the counts of both renderers are compared, and the resolved
frames are checked against the host's restatement.  One JSON line for the whole
run, also written to --out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_lights import spread  # noqa: E402

PEAK_TBS = 8.0
BYTES = {"relight": 24, "grey": 8, "modulate": 28}
INF = float("inf")


def apart_below(a, b):
    """a measures below b with quartile ranges apart"""
    return bool(a["q3_ms"] < b["q1_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tekkaman")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ab", default="ao_w1,ao_w4,ao_packet")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21", "ao_1024.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_ao needs a GPU"
    from conftest import scene_path
    from skybox_rt_amd import rt
    s = rt.Scene.load(scene_path(args.scene))
    r = rt.Renderer(s)
    rp = rt.Renderer(s)                       # the yardstick's renderer: a path configuration
    vdir = os.path.join(ROOT, "skybox_rt_amd", "lib", "variants")
    rbs = {name: rt.Renderer(s, kernel_dir=os.path.join(vdir, name)) for name in args.ab.split(",") if name}
    n = args.size
    out = {"bench": "ao", "scene": args.scene, "size": n, "steps": args.steps, "warmup": args.warmup,
           "timer": "the driver's time of each launch (an ordinary launch started on an idle queue), in rounds",
           "seed": rt.AO_SEED, "peak_TBps": PEAK_TBS, "bytes_per_pixel": BYTES,
           "ab_kernel_dirs": [os.path.relpath(os.path.join(vdir, name), ROOT) for name in rbs]}

    def timed(q, fn, *a):
        fn(*a)
        q.wait()
        return q.kernel_ms()

    r.configure(n, n, shadows=True, light=rt.DEFAULT_LIGHT, counters=False)
    r.relight_capture()
    rec = r.aov_records()
    rays = ((rec["depth_flags"] & np.uint32(rt.RT_AOV_GEOM)) != 0) & (rec["t"] > 0) & np.isfinite(rec["t"])
    out["ray_pixels"] = int(rays.sum())
    out["ray_pixel_share"] = round(float(rays.mean()), 4)
    blocks = rays.reshape(n // 8, 8, n // 8, 8).any(axis=(1, 3)) if n % 8 == 0 else None
    out["blocks_with_rays_share"] = round(float(blocks.mean()), 4) if blocks is not None else None
    for rb in rbs.values():
        rb.configure(n, n, shadows=True, light=rt.DEFAULT_LIGHT, counters=False)
        rb.aov()
    rp.configure(n, n, path=True, bounces=1, seed=rt.AO_SEED, counters=False)
    rp.accum_begin()

    def ao_launch(q, k):
        q.ao_reset()
        q.ao(k, wait=False)

    def accum_launch(k):
        rp.accum_reset()
        rp.accumulate(k, wait=False)

    series = {}
    for radius in (INF, 8.0):
        tag = "inf" if radius == INF else f"{radius:g}"
        r.ao_begin(radius=radius, seed=rt.AO_SEED)
        for rb in rbs.values():
            rb.ao_begin(radius=radius, seed=rt.AO_SEED)
        ks = (1, 8, 64)
        for k in ks:
            for _ in range(args.warmup):
                timed(r, ao_launch, r, k)
                for rb in rbs.values():
                    timed(rb, ao_launch, rb, k)
        for k in (1, 8):
            for _ in range(args.warmup):
                timed(rp, accum_launch, k)
        t = {f"ao_{k}": [] for k in ks}
        t.update({f"{name}_{k}": [] for k in ks for name in rbs})
        t.update({f"accumulate_{k}": [] for k in (1, 8)})
        for _ in range(args.steps):
            for k in ks:
                t[f"ao_{k}"].append(timed(r, ao_launch, r, k))
                for name, rb in rbs.items():
                    t[f"{name}_{k}"].append(timed(rb, ao_launch, rb, k))
            for k in (1, 8):
                t[f"accumulate_{k}"].append(timed(rp, accum_launch, k))
        sp = {key: spread(v) for key, v in t.items()}
        counts = r.ao_records()               # the last launch: 64 samples
        entry = dict(sp)
        entry["occluded_share_64"] = round(float(counts.sum()) / max(64 * int(rays.sum()), 1), 4)
        entry["mrays_per_s"] = {k: round(k * int(rays.sum()) / (sp[f"ao_{k}"]["median_ms"] * 1e-3) * 1e-6, 1) for k in ks}
        for k in (1, 8):
            entry[f"ao_{k}_over_accumulate_{k}"] = round(sp[f"ao_{k}"]["median_ms"] / sp[f"accumulate_{k}"]["median_ms"], 4)
            entry[f"ao_{k}_below_accumulate_{k}_quartiles_apart"] = apart_below(sp[f"ao_{k}"], sp[f"accumulate_{k}"])
        for name, rb in rbs.items():
            entry[f"{name}_counts_equal"] = bool(np.array_equal(rb.ao_records(), counts))
            for k in ks:
                entry[f"ao_{k}_over_{name}_{k}"] = round(sp[f"ao_{k}"]["median_ms"] / sp[f"{name}_{k}"]["median_ms"], 4)
                entry[f"ao_{k}_below_{name}_{k}_quartiles_apart"] = apart_below(sp[f"ao_{k}"], sp[f"{name}_{k}"])
        series[f"radius_{tag}"] = entry
    out["trace"] = series

    # the resolves next to the relight launch (the counts: 64 samples at radius 8)
    fns = {"relight": (r.relight, ([1], False)), "grey": (r.ao_resolve, ("grey", None, False)),
           "modulate": (r.ao_resolve, ("modulate", [1], False))}
    for fn, a in fns.values():
        for _ in range(args.warmup):
            timed(r, fn, *a)
    t = {key: [] for key in fns}
    for _ in range(args.steps):
        for key, (fn, a) in fns.items():
            t[key].append(timed(r, fn, *a))
    sp = {key: spread(v) for key, v in t.items()}
    res = dict(sp)
    for key in fns:
        res[f"{key}_TBps"] = round(BYTES[key] * n * n / (sp[key]["median_ms"] * 1e-3) * 1e-12, 3)
    res["grey_over_relight"] = round(sp["grey"]["median_ms"] / sp["relight"]["median_ms"], 4)
    res["modulate_over_relight"] = round(sp["modulate"]["median_ms"] / sp["relight"]["median_ms"], 4)
    res["grey_below_relight_quartiles_apart"] = apart_below(sp["grey"], sp["relight"])
    counts, base = r.ao_records(), r.relight_base()
    r.ao_resolve("grey")
    res["grey_equals_host_resolve"] = bool(np.array_equal(r.framebuffer(), rt.ao_resolve(np.full((n, n), 0xFFFFFFFF, np.uint32), counts, 64)))
    r.ao_resolve("modulate", [1])
    lit = rt.relight_resolve(base, rec["depth_flags"], rec["light_mask"], [1])
    res["modulate_equals_host_resolve"] = bool(np.array_equal(r.framebuffer(), rt.ao_resolve(lit, counts, 64)))
    out["resolve"] = res
    for q in [r, rp] + list(rbs.values()):
        q.close()
    s.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
