#!/usr/bin/env python3
"""Kernel time of caller-supplied ray queries (image rt_query), in one process,
on three ray sets of one scene at one size:
  eye     the eye rays through every pixel centre,
  ao      the ambient-occlusion rays of the frame's ray pixels x 8 samples,
          regenerated on the host by tests/ao_reference.py's formulas from the
          device's visibility records (pixel-major: a pixel's 8 rays adjacent),
  random  2^20 rays between uniformly random points of the scene box;
each traced closest and any, in the input order, in a random shuffle, and in the
shuffle restored by the key sort (the key launch, a device sort of the keys and
the trace under RT_QUERY_PERM, timed separately and summed).  The yardstick of
ao / any is ao(8) on the same scene in the same process: the same rays, made in
registers.  --ab DIRS (kernel directories under lib/variants, default
query_w2,query_w4: RT_QUERY_WAVES 2 and 4 in place of the shipped 1) run the ao
set in the same rounds; their hits must equal the shipped image's.

Every launch is an ordinary launch started on an idle queue and timed by the
driver's events (Renderer.kernel_ms); after --warmup rounds, --steps rounds run
every series in turn, so drift hits all alike.  Median and quartiles of each; two
count as apart where their quartile ranges do not overlap.  One JSON line, also
written to --out."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_lights import spread  # noqa: E402

INF = float("inf")
BYTES_PER_RAY = {"trace": 40, "trace_skip": 44, "trace_perm": 44, "trace_skip_perm": 48, "keys": 36}


def apart_below(a, b):
    return bool(a["q3_ms"] < b["q1_ms"])


def eye_rays(n):
    pix = np.arange(n * n)
    x, y = (pix % n).astype(np.float32), (pix // n).astype(np.float32)
    s = np.float32(2.0) / np.float32(n)
    rays = np.zeros((n * n, 8), np.float32)
    rays[:, 3] = ((x + np.float32(0.5)).astype(np.float64) * np.float64(s) - 1.0).astype(np.float32)
    rays[:, 4] = ((y + np.float32(0.5)).astype(np.float64) * np.float64(s) - 1.0).astype(np.float32)
    rays[:, 5], rays[:, 7] = 1.0, INF
    return rays, None


def ao_rays(sc, rec, n, seed, S):
    import ao_reference as ar
    fv = ar.first_vertex(sc, n, n, rec["pid"], rec["t"])
    gid, _, _ = ar.geometry(sc)
    m = len(fv["idx"])
    rays = np.zeros((m, S, 8), np.float32)
    for j in range(S):
        rays[:, j, 0:3], rays[:, j, 3:6] = fv["P"], ar.sample_rays(fv, seed + j)
    rays[:, :, 7] = INF
    skip = np.repeat(gid[fv["tri"]].astype(np.int32), S)
    return rays.reshape(m * S, 8), skip, fv


def random_rays(box, n, seed=77):
    rng = np.random.default_rng(seed)
    lo, hi = box[:3].astype(np.float64), box[3:].astype(np.float64)
    a, b = lo + rng.random((n, 3)) * (hi - lo), lo + rng.random((n, 3)) * (hi - lo)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 7] = a, b - a, 1.0
    return rays, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tekkaman")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--ab", default="query_w2,query_w4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "query_1024.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_query needs a GPU"
    from conftest import scene_path
    from oracle import py_oracle as po
    from skybox_rt_amd import _lib, rt
    h = rt.lib()
    n = args.size
    path = scene_path(args.scene)
    sc = po.cgltrace.load(path)
    s = rt.Scene.load(path)
    vdir = os.path.join(ROOT, "skybox_rt_amd", "lib", "variants")
    img = os.path.join(_lib.LIB_DIR, "rt_query.vxbin")
    out = {"bench": "query", "scene": args.scene, "size": n, "steps": args.steps, "warmup": args.warmup,
           "timer": "the driver's event time of each launch (an ordinary launch started on an idle queue), in rounds",
           "kernel_md5": hashlib.md5(open(img, "rb").read()).hexdigest(), "bytes_per_ray": BYTES_PER_RAY,
           "ab_kernel_dirs": [os.path.relpath(os.path.join(vdir, v), ROOT) for v in args.ab.split(",") if v]}

    # the yardstick's renderer, and the records the ao set starts from
    r0 = rt.Renderer(s)
    r0.configure(n, n, shadows=True, light=rt.DEFAULT_LIGHT, counters=False)
    rec = r0.aov()
    r0.ao_begin(radius=INF, seed=rt.AO_SEED)
    r0.query_reserve(64)
    box = r0.query_buffers()["box"]
    sets = {"eye": eye_rays(n), "random": random_rays(box, 1 << 20)}
    ar_rays, ar_skip, fv = ao_rays(sc, rec, n, rt.AO_SEED, 8)
    sets["ao"] = (ar_rays, ar_skip)
    out["rays"] = {k: len(v[0]) for k, v in sets.items()}
    out["ray_pixels"] = len(fv["idx"])

    def renderer(rays, skip, kdir=None):
        q = rt.Renderer(s, kernel_dir=kdir)
        q.configure(64, 64, shadows=False, counters=False)
        q.query_reserve(len(rays))
        q._query_upload("bench", rays, skip)
        q.wait()
        return q

    def launch(q, m, mode, flags):
        rt._check(h.rt_query_trace(q._h, m, rt.QUERY_MODES[mode], flags), "rt_query_trace")
        return q.kernel_ms()

    def keys_launch(q, m):
        rt._check(h.rt_query_keys(q._h, m), "rt_query_keys")
        return q.kernel_ms()

    def device_sort(q, m, write):
        """the keys' stable sort on the device, by torch's events -> ms; write: the permutation into the reserve"""
        keys, ext = q._query_keys_device(m)
        ext.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(ext):
            e0.record(ext)
            perm = torch.sort(keys, stable=True).indices.to(torch.int32)
            e1.record(ext)
            if write:
                rt._hip_copy(q.query_buffers()["perm"], perm.data_ptr(), 4 * m, ext.cuda_stream)
        ext.synchronize()
        return e0.elapsed_time(e1)

    rng = np.random.default_rng(3)
    series = {}   # name -> (callable -> ms)
    checks = {}
    qs = [r0]
    for name, (rays, skip) in sets.items():
        m = len(rays)
        sh = rng.permutation(m)
        f = rt.RT_QUERY_SKIP if skip is not None else 0
        qi = renderer(rays, skip)
        qsh = renderer(rays[sh], None if skip is None else skip[sh])
        qs += [qi, qsh]
        keys_launch(qsh, m)
        device_sort(qsh, m, True)
        for mode in ("closest", "any"):
            base = f"{name}_{mode}"
            series[f"{base}_input"] = lambda q=qi, m=m, mode=mode, f=f: launch(q, m, mode, f)
            series[f"{base}_shuffled"] = lambda q=qsh, m=m, mode=mode, f=f: launch(q, m, mode, f)
            series[f"{base}_sorted_trace"] = lambda q=qsh, m=m, mode=mode, f=f: launch(q, m, mode, f | rt.RT_QUERY_PERM)
            # the three orders give the same hits, at the rays' own indices
            launch(qi, m, mode, f)
            a = qi.query_hits(m)
            launch(qsh, m, mode, f)
            b = qsh.query_hits(m)
            launch(qsh, m, mode, f | rt.RT_QUERY_PERM)
            c = qsh.query_hits(m)
            hit = a[0] >= 0
            checks[base] = {"hit_share": round(float(hit.mean()), 4),
                            "shuffled_equals_input": bool(np.array_equal(hit[sh], b[0] >= 0) if mode == "any" else
                                                          np.array_equal(a[0][sh], b[0]) and np.array_equal(a[1][sh], b[1])),
                            "sorted_equals_shuffled": bool(np.array_equal(b[0], c[0]) and np.array_equal(b[1], c[1]))}
        series[f"{name}_keys"] = lambda q=qsh, m=m: keys_launch(q, m)
        series[f"{name}_sort"] = lambda q=qsh, m=m: device_sort(q, m, False)
        if name == "ao":
            # the any-hit verdicts, summed per pixel, are ao(8)'s counts
            launch(qi, m, "any", f)
            got = np.zeros(n * n, np.uint32)
            got[fv["idx"]] = (qi.query_hits(m)[0] >= 0).reshape(-1, 8).sum(1)
            r0.ao_reset()
            r0.ao(8)
            checks["ao_any_counts_equal_ao8"] = bool(np.array_equal(got.reshape(n, n), r0.ao_records()))
            for v in [v for v in args.ab.split(",") if v]:
                qv = renderer(rays, skip, os.path.join(vdir, v))
                qvs = renderer(rays[sh], skip[sh], os.path.join(vdir, v))
                qs += [qv, qvs]
                for mode in ("closest", "any"):
                    series[f"ao_{mode}_input_{v}"] = lambda q=qv, m=m, mode=mode, f=f: launch(q, m, mode, f)
                    series[f"ao_{mode}_shuffled_{v}"] = lambda q=qvs, m=m, mode=mode, f=f: launch(q, m, mode, f)
                    launch(qv, m, mode, f)
                    launch(qi, m, mode, f)
                    checks[f"ao_{mode}_{v}_equals_shipped"] = bool(np.array_equal(qv.query_hits(m)[0], qi.query_hits(m)[0]))

    def ao8():
        r0.ao_reset()
        r0.ao(8, wait=False)
        r0.wait()
        return r0.kernel_ms()

    series["ao8_yardstick"] = ao8
    for _ in range(args.warmup):
        for fn in series.values():
            fn()
    t = {k: [] for k in series}
    for _ in range(args.steps):
        for k, fn in series.items():
            t[k].append(fn())
    sp = {k: spread(v) for k, v in t.items()}
    out["series"] = sp
    out["checks"] = checks
    summary = {}
    for name, (rays, _) in sets.items():
        m = len(rays)
        for mode in ("closest", "any"):
            base = f"{name}_{mode}"
            tot = [a + b + c for a, b, c in zip(t[f"{name}_keys"], t[f"{name}_sort"], t[f"{base}_sorted_trace"])]
            ssum = spread(tot)
            summary[base] = {
                "grays_per_s": {o: round(m / (sp[f"{base}_{o}"]["median_ms"] * 1e-3) * 1e-9, 3)
                                for o in ("input", "shuffled", "sorted_trace")},
                "sorted_sum": ssum,
                "sorted_sum_below_shuffled_quartiles_apart": apart_below(ssum, sp[f"{base}_shuffled"]),
                "sorted_sum_below_input_quartiles_apart": apart_below(ssum, sp[f"{base}_input"]),
                "sorted_trace_over_shuffled": round(sp[f"{base}_sorted_trace"]["median_ms"] / sp[f"{base}_shuffled"]["median_ms"], 4)}
    a, y = sp["ao_any_input"], sp["ao8_yardstick"]
    summary["ao_any_input_over_ao8"] = round(a["median_ms"] / y["median_ms"], 4)
    summary["ao_any_input_above_ao8_quartiles_apart"] = apart_below(y, a)
    m = len(sets["ao"][0])
    summary["ao_any_extra_ms"] = round(a["median_ms"] - y["median_ms"], 5)
    summary["ao_any_bytes_moved_MB"] = round(BYTES_PER_RAY["trace_skip"] * m * 1e-6, 2)
    summary["ao_any_bytes_at_6TBps_ms"] = round(BYTES_PER_RAY["trace_skip"] * m / 6.0e12 * 1e3, 5)
    out["summary"] = summary
    for q in qs:
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
