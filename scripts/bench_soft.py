#!/usr/bin/env python3
"""Kernel time of soft shadows from the visibility records, in one process: the
tracing launch soft(S) (image rt_soft) for S = 1, 8, 64 under n = 1 and 4 lights
at radius 0 and at a radius with a visible penumbra, next to three yardsticks --

  (a) rt_query_trace any-hit with RT_QUERY_SKIP over the same segments, supplied
      as a device tensor in the kernel's own order (block, pixel, light, sample);
      generating them is not timed.  They are restated here with torch's
      binary32 operations, which fuse nothing: a target may differ from the
      kernel's in its last bit, so the verdict sums are compared and the
      differing (light, pixel) counts reported, not required to be none.  A
      reserve holds 2^24 rays: n = 4 at S = 64 has more, so its segments go to two
      renderers' reserves, half each, and a round's time is the two launches' sum;
  (b) one record launch (rt_render_aov) under the same lights, times S: the hard
      shadow's cost on the light-space lists;
  (c) ao(S): the same structure with incoherent, unbounded rays

-- and the resolve launch (image rt_soft_resolve: lit 2 n + 8 B a pixel, grey
2 n + 4 B) next to the relight launch (image rt_relight, 24 B a pixel).

All are ordinary launches on their image's own grid, each started on an idle
queue and timed by the driver as bench_ao.py's are.  After `--warmup` launches of
each, `--steps` rounds run them in turn, so drift hits all alike.  Median and
quartiles of each; two count as apart where their quartile ranges do not
overlap.  Every tracing launch of a series resets, so each traces the same
samples.

--ab DIRS (comma-separated kernel directories under lib/variants; default the
seven A/B images beside the shipped one, which is the packet walk dealt
light-major on four waves: soft_w1 / _w2 / _w4 the per-lane walk dealt
pixel-major on 1, 2 and 4 waves, soft_lmajor the same walk dealt light-major on
2, soft_packet the packet walk dealt pixel-major on 2, soft_packet_lmajor_w1 /
_w2 the shipped choices on 1 and 2 waves): one more renderer per directory runs
the same tracing launches in the same rounds; its counts must equal the first
renderer's.

One JSON line for the whole run, also written to --out."""
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
LIGHTS = [(0.0, 60.0, 80.0), (40.0, 10.0, 60.0), (-30.0, -20.0, 90.0), (30.0, -20.0, 95.0)]
KS = (1, 8, 64)
QUERY_CAP = 1 << 24


def apart_below(a, b):
    """a measures below b with quartile ranges apart"""
    return bool(a["q3_ms"] < b["q1_ms"])


def not_above(a, b):
    """a is no slower than b beyond the quartile ranges"""
    return bool(a["q1_ms"] <= b["q3_ms"])


def segments(torch, rec, n, lights, radii, seed, S, dev="cuda"):
    """the launch's segments as a CUDA tensor float32 [m, 8] (o, d, tmin, tmax) and their skip int32 [m],
    in block / pixel / light / sample order, and the (light, pixel index) of each as int64 tensors"""
    rays = ((rec["depth_flags"] & np.uint32(0x01000000)) != 0) & (rec["t"] > 0) & np.isfinite(rec["t"])
    ys, xs = np.nonzero(rays)
    order = np.lexsort((xs & 7, ys & 7, xs >> 3, ys >> 3))
    ys, xs = ys[order], xs[order]
    p = torch.tensor(ys * n + xs, dtype=torch.int64, device=dev)
    t = torch.tensor(rec["t"][ys, xs], dtype=torch.float32, device=dev)
    pid = torch.tensor(rec["pid"][ys, xs].astype(np.int32), dtype=torch.int32, device=dev)
    sx = torch.tensor(2.0 / n, dtype=torch.float32, device=dev)
    d = torch.stack([(torch.tensor(xs, dtype=torch.float32, device=dev) + 0.5) * sx - 1.0,
                     (torch.tensor(ys, dtype=torch.float32, device=dev) + 0.5) * sx - 1.0,
                     torch.ones(len(xs), dtype=torch.float32, device=dev)], 1)
    P = d * (t * np.float32(0.999755859375))[:, None]
    M = 0xFFFFFFFF

    def pcg(v):
        state = (v * 747796405 + 2891336453) & M
        word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M
        return ((word >> 22) ^ word) & M

    def u11(h):
        return (h >> 8).to(torch.float32) * np.float32(2.0 ** -23) - 1.0

    nl = len(lights)
    k = p[:, None, None].expand(-1, nl, S)
    li = torch.arange(nl, device=dev)[None, :, None].expand(len(p), -1, S)
    j = torch.arange(S, device=dev)[None, None, :].expand(len(p), nl, -1)
    key = pcg(k ^ pcg(((seed + j) & M) ^ ((0x9E3779B9 * (64 + li + 1)) & M)))
    L = torch.tensor(lights, dtype=torch.float32, device=dev)[None, :, None, :]
    R = torch.tensor(radii, dtype=torch.float32, device=dev)[None, :, None, None]
    Pb = P[:, None, None, :].expand(-1, nl, S, -1)
    m = Pb - L
    m = m / torch.sqrt((m * m).sum(-1, keepdim=True))
    x = torch.zeros(key.shape, dtype=torch.float32, device=dev)
    y = torch.zeros_like(x)
    found = torch.zeros(key.shape, dtype=torch.bool, device=dev)
    for i in range(8):
        a, b = u11(pcg((key + 2 * i) & M)), u11(pcg((key + 2 * i + 1) & M))
        ok = (a * a + b * b < 1.0) & ~found
        x, y, found = torch.where(ok, a, x), torch.where(ok, b, y), found | ok
    z = torch.sqrt(1.0 - (x * x + y * y))
    n0, n1, n2 = m[..., 0], m[..., 1], m[..., 2]
    sgn = torch.where(n2 >= 0, 1.0, -1.0).to(torch.float32)
    A = -1.0 / (sgn + n2)
    B = n0 * n1 * A
    t1 = torch.stack([1.0 + sgn * n0 * n0 * A, sgn * B, -sgn * n0], -1)
    t2 = torch.stack([B, sgn + n1 * n1 * A, -n1], -1)
    u = x[..., None] * t1 + y[..., None] * t2 + z[..., None] * m
    D = (R * u + L) - Pb
    out = torch.zeros((len(p) * nl * S, 8), dtype=torch.float32, device=dev)
    out[:, 0:3], out[:, 3:6], out[:, 7] = Pb.reshape(-1, 3), D.reshape(-1, 3), 1.0
    skip = pid[:, None, None].expand(-1, nl, S).reshape(-1).contiguous()
    return out, skip, li.reshape(-1), k.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tekkaman")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radius", type=float, default=4.0)
    ap.add_argument("--ab", default="soft_w1,soft_w2,soft_w4,soft_lmajor,soft_packet,soft_packet_lmajor_w1,"
                                     "soft_packet_lmajor_w2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23", "soft_1024.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_soft needs a GPU"
    from conftest import scene_path
    from skybox_rt_amd import rt
    h = rt.lib()
    s = rt.Scene.load(scene_path(args.scene))
    vdir = os.path.join(ROOT, "skybox_rt_amd", "lib", "variants")
    names = [v for v in args.ab.split(",") if v]
    r = rt.Renderer(s)
    rqs = [rt.Renderer(s), rt.Renderer(s)]    # yardstick (a)'s renderers: a reserve of 2^24 rays each
    rbs = {name: rt.Renderer(s, kernel_dir=os.path.join(vdir, name)) for name in names}
    n, seed = args.size, rt.RT_SOFT_DEFAULT_SEED
    out = {"bench": "soft", "scene": args.scene, "size": n, "steps": args.steps, "warmup": args.warmup,
           "timer": "the driver's time of each launch (an ordinary launch started on an idle queue), in rounds",
           "seed": seed, "radius": args.radius, "lights": LIGHTS, "peak_TBps": PEAK_TBS,
           "ab_kernel_dirs": [os.path.relpath(os.path.join(vdir, v), ROOT) for v in names]}

    def timed(q, fn, *a):
        fn(*a)
        q.wait()
        return q.kernel_ms()

    def soft_launch(q, k):
        q.soft_reset()
        q.soft(k, wait=False)

    def ao_launch(q, k):
        q.ao_reset()
        q.ao(k, wait=False)

    def query_launch(parts):
        """one any-hit launch per part [(renderer, rays)] -> the launches' times, summed"""
        ms = 0.0
        for q, m in parts:
            rt._check(h.rt_query_trace(q._h, m, rt.QUERY_MODES["any"], rt.RT_QUERY_SKIP), "rt_query_trace")
            ms += q.kernel_ms()
        return ms

    for q in rqs:
        q.configure(64, 64, shadows=False, counters=False)
        q.query_reserve(QUERY_CAP)
    trace = {}
    for nl in (1, 4):
        lights = LIGHTS[:nl]
        for q in [r] + list(rbs.values()):
            q.configure(n, n, shadows=True, light=lights[0], counters=False)
            if nl > 1:
                q.set_lights(lights)
        r.relight_capture()
        rec = r.aov_records()
        for rb in rbs.values():
            rb.aov()
        rays = ((rec["depth_flags"] & np.uint32(rt.RT_AOV_GEOM)) != 0) & (rec["t"] > 0) & np.isfinite(rec["t"])
        out["ray_pixels"] = int(rays.sum())
        r.ao_begin(radius=float("inf"), seed=rt.AO_SEED)
        for radius in (0.0, args.radius):
            radii = [radius] * nl
            for q in [r] + list(rbs.values()):
                q.soft_begin(radii, seed=seed)
            t = {}
            for k in KS:
                m = int(rays.sum()) * nl * k
                runs = {f"soft_{k}": lambda k=k: timed(r, soft_launch, r, k), f"ao_{k}": lambda k=k: timed(r, ao_launch, r, k)}
                runs.update({f"{name}_{k}": lambda rb=rb, k=k: timed(rb, soft_launch, rb, k) for name, rb in rbs.items()})
                if k == 1:
                    runs["aov"] = lambda: timed(r, r.aov, False)
                entry_q = None
                if m <= QUERY_CAP * len(rqs):
                    seg, skip, li, pix = segments(torch, rec, n, lights, radii, seed, k)
                    cuts = [0, m] if m <= QUERY_CAP else [0, m // 2, m]
                    parts = []
                    for q, a, b in zip(rqs, cuts[:-1], cuts[1:]):
                        q._query_upload("bench", seg[a:b], skip[a:b].contiguous())
                        q.wait()
                        parts.append((q, b - a))
                    runs[f"query_{k}"] = lambda parts=parts: query_launch(parts)
                    # the verdicts, summed per (light, pixel), against the launch's counts
                    query_launch(parts)
                    hit = torch.tensor(np.concatenate([q.query_hits(mm)[0] >= 0 for q, mm in parts]),
                                       device="cuda").to(torch.int64)
                    got = torch.zeros(nl * n * n, dtype=torch.int64, device="cuda").index_add_(0, li * (n * n) + pix, hit)
                    soft_launch(r, k)
                    r.wait()
                    cnt = r.soft_records()
                    entry_q = int((got.cpu().numpy().reshape(nl, n, n) != cnt).sum())
                    del seg, skip, li, pix, got, hit
                for _ in range(args.warmup):
                    for fn in runs.values():
                        fn()
                tk = {key: [] for key in runs}
                for _ in range(args.steps):
                    for key, fn in runs.items():
                        tk[key].append(fn())
                t.update({key: spread(v) for key, v in tk.items()})
                if entry_q is not None:
                    t[f"query_{k}_counts_differing"] = entry_q
                    t[f"query_{k}_launches"] = len(parts)
                soft_launch(r, k)
                r.wait()
                cnt = r.soft_records()
                t[f"occluded_share_{k}"] = round(float(cnt.sum(dtype=np.int64)) / max(m, 1), 4)
                t[f"partial_pixels_{k}"] = int(((cnt > 0) & (cnt < k)).any(0).sum())
                t[f"mrays_per_s_{k}"] = round(m / (t[f"soft_{k}"]["median_ms"] * 1e-3) * 1e-6, 1)
                for name, rb in rbs.items():
                    soft_launch(rb, k)
                    rb.wait()
                    t[f"{name}_{k}_counts_equal"] = bool(np.array_equal(rb.soft_records(), cnt))
                    t[f"soft_{k}_over_{name}_{k}"] = round(t[f"soft_{k}"]["median_ms"] / t[f"{name}_{k}"]["median_ms"], 4)
                if f"query_{k}" in t:
                    t[f"soft_{k}_over_query_{k}"] = round(t[f"soft_{k}"]["median_ms"] / t[f"query_{k}"]["median_ms"], 4)
                    t[f"soft_{k}_not_above_query_{k}"] = not_above(t[f"soft_{k}"], t[f"query_{k}"])
                t[f"soft_{k}_over_ao_{k}"] = round(t[f"soft_{k}"]["median_ms"] / t[f"ao_{k}"]["median_ms"], 4)
                t[f"soft_{k}_over_{k}_aov"] = round(t[f"soft_{k}"]["median_ms"] / (k * t["aov"]["median_ms"]), 4)
            trace[f"n{nl}_radius_{radius:g}"] = t
            print(f"n={nl} radius {radius:g} done", file=sys.stderr, flush=True)

        # the resolves next to the relight launch (the counts: 64 samples at the radius)
        w = [1] * nl
        fns = {"relight": (r.relight, (w, False)), "lit": (r.soft_resolve, ("lit", w, False)),
               "grey": (r.soft_resolve, ("grey", None, False))}
        bpp = {"relight": 24, "lit": 2 * nl + 8, "grey": 2 * nl + 4}
        for fn, a in fns.values():
            for _ in range(args.warmup):
                timed(r, fn, *a)
        tr = {key: [] for key in fns}
        for _ in range(args.steps):
            for key, (fn, a) in fns.items():
                tr[key].append(timed(r, fn, *a))
        res = {key: spread(v) for key, v in tr.items()}
        for key in fns:
            res[f"{key}_bytes_per_pixel"] = bpp[key]
            res[f"{key}_TBps"] = round(bpp[key] * n * n / (res[key]["median_ms"] * 1e-3) * 1e-12, 3)
        res["lit_over_relight"] = round(res["lit"]["median_ms"] / res["relight"]["median_ms"], 4)
        res["grey_over_relight"] = round(res["grey"]["median_ms"] / res["relight"]["median_ms"], 4)
        cnt, base = r.soft_records(), r.relight_base()
        r.soft_resolve("lit", w)
        sub = (slice(None, None, 7), slice(None, None, 5))     # (the host's restatement on a lattice of pixels)
        want = rt.soft_resolve(base[sub], rec["depth_flags"][sub], cnt[(slice(None),) + sub], 64, w)
        res["lit_equals_host_resolve"] = bool(np.array_equal(r.framebuffer()[sub], want))
        out[f"resolve_n{nl}"] = res
    out["trace"] = trace
    for q in [r] + rqs + list(rbs.values()):
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
