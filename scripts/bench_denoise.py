#!/usr/bin/env python3
"""Kernel time of the denoiser next to the launches it sits beside, in one
process on one renderer: the guide capture (image rt_aov_guide) against the
relight capture of the primary+shadow configuration (image rt_aov_base: the same
source tracing one shadow ray per pixel), and denoise(passes=1..5) -- the prepare
launch (rt_denoise_prep) and the passes (rt_denoise_pass) -- against
accumulate(1) of the same path frame.

All are ordinary launches on their image's own grid, timed by the driver.  A
denoise() call is 1 + passes launches queued back to back, and the driver puts
events on one queued launch in VX_HIP_TIME_EVERY (4): this script runs under
VX_HIP_TIME_EVERY=1 (unless the variable is set), so every launch is timed.  A
call's time is the growth of the driver's sum over the timed launches across the
call (every launch of the call must have been timed, or the round is dropped and
counted), and the driver's time of the last launch is the time of pass `passes`
alone (stride 2^(passes-1), with the remodulating store).  The prepare launch is
the call's first, started on an idle queue: the driver times such a launch with
its launch boundary, so prepare_ms = denoise_1 - pass_1 is an upper bound.  After
`--warmup` rounds, `--steps` rounds run capture, sample and the five filters in
turn, so drift hits all alike.  Median and quartiles of each.

--ab DIR: a second renderer on kernel directory DIR (lib/variants/dn_lds: the pass
image that stages its tile with halo in LDS at strides 1 and 2) runs the same
filters in the same rounds on the same records; its pass times are reported
beside the first renderer's (the shipped images, or --kernel-dir's) and its
frames must equal them.

Bytes.  The prepare pass moves 52 B a pixel (16-B record, 16-B guide, 4-B base
colour in, two 8-B tap records out).  A pass gathers 25 taps of 16 B: 400 B a
pixel requested from the caches, of which 16 B are new to the chip when every
tap is served on chip; it stores 8 B (the last pass 4 B and reads the 4-B base
colour).  Both figures are given over each pass's time against the 8 TB/s peak
of the memory: the compulsory 24 B a pixel as the share of peak a perfect cache
would leave, the 408 B as what the cache hierarchy delivered.  At the size timed
one denoised frame is checked against the numpy model when --check is given.
One JSON line for the whole run, also written to --out."""
import argparse
import json
import os
import sys

import numpy as np

os.environ.setdefault("VX_HIP_TIME_EVERY", "1")  # read when the device opens: events on every queued launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_lights import spread  # noqa: E402

PEAK_TBS = 8.0
PREP_BYTES = 52
PASS_COMPULSORY = 24
PASS_REQUESTED = 408


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="tekkaman")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--check", action="store_true", help="compare one frame with tests/denoise_reference.py")
    ap.add_argument("--kernel-dir", default=None, help="kernel directory of the first renderer (default: the library's)")
    ap.add_argument("--ab", default=None, help="kernel directory of a pass-image variant to time beside the shipped one")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20", "denoise_1024.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_denoise needs a GPU"
    from conftest import scene_path
    from skybox_rt_amd import rt
    s = rt.Scene.load(scene_path(args.scene))
    r = rt.Renderer(s, kernel_dir=args.kernel_dir)
    n = args.size
    npix = n * n
    out = {"bench": "denoise", "scene": args.scene, "size": n, "bounces": args.bounces, "steps": args.steps,
           "warmup": args.warmup, "peak_TBps": PEAK_TBS,
           "kernel_dir": os.path.relpath(args.kernel_dir, ROOT) if args.kernel_dir else None, "VX_HIP_TIME_EVERY": os.environ["VX_HIP_TIME_EVERY"],
           "defaults": [rt.DENOISE_PASSES, rt.DENOISE_DEPTH_SHIFT, rt.DENOISE_COLOR_SHIFT],
           "timer": "the driver's time of each launch; a denoise call: the growth of the driver's sum over its "
                    "1 + passes launches; rounds of capture / accumulate(1) / denoise(passes=1..5)"}

    def timed(fn, *a, **kw):
        fn(*a, **kw)
        r.wait()
        return r.kernel_ms()

    # the relight capture of the primary+shadow configuration: the yardstick for the guide capture
    r.configure(n, n, shadows=True, counters=False)
    for _ in range(args.warmup):
        timed(r.relight_capture, False)
    out["relight_capture"] = spread([timed(r.relight_capture, False) for _ in range(args.steps)])

    r.configure(n, n, path=True, bounces=args.bounces, counters=False)
    r.accum_begin()
    r.denoise_capture()
    r.accumulate(8)
    g = r.denoise_guide()[0]
    out["geometry_pixel_share"] = round(float(((g["depth_flags"] & np.uint32(rt.RT_AOV_GEOM)) != 0).mean()), 4)
    rb = None
    if args.ab:
        rb = rt.Renderer(s, kernel_dir=args.ab)
        rb.configure(n, n, path=True, bounces=args.bounces, counters=False)
        rb.accum_begin()
        rb.denoise_capture()
        rb.write_accum(r.accum())
        out["ab"] = {"kernel_dir": os.path.relpath(args.ab, ROOT), "frames_equal": True}
        tb = {f"pass_{p}": [] for p in range(1, 6)}
    t = {"capture": [], "accumulate_1": []}
    for p in range(1, 6):
        t[f"denoise_{p}"] = []
        t[f"pass_{p}"] = []
    dropped = 0
    for i in range(args.warmup + args.steps):
        row = {"capture": timed(r.denoise_capture, False), "accumulate_1": timed(r.accumulate, 1, False)}
        ok = True
        for p in range(1, 6):
            ms0, nt0, _ = r.run_totals()
            row[f"pass_{p}"] = timed(r.denoise, passes=p, wait=False)
            ms1, nt1, _ = r.run_totals()
            ok = ok and nt1 - nt0 == p + 1
            row[f"denoise_{p}"] = ms1 - ms0
            if rb is not None:
                rb.denoise(passes=p, wait=False)
                rb.wait()
                if i >= args.warmup:
                    tb[f"pass_{p}"].append(rb.kernel_ms())
        if i < args.warmup:
            continue
        if not ok:
            dropped += 1
            continue
        for k, v in row.items():
            t[k].append(v)
    sp = {k: spread(v) for k, v in t.items() if v}
    out["rounds_dropped_untimed"] = dropped
    out.update(sp)
    if "denoise_1" in sp:
        prep = sp["denoise_1"]["median_ms"] - sp["pass_1"]["median_ms"]
        out["prepare_ms"] = round(prep, 5)
        out["prepare_TBps"] = round(PREP_BYTES * npix / (prep * 1e-3) * 1e-12, 3) if prep > 0 else None
        out["capture_over_relight_capture"] = round(sp["capture"]["median_ms"] / out["relight_capture"]["median_ms"], 4)
        for p in range(1, 6):
            sec = sp[f"pass_{p}"]["median_ms"] * 1e-3
            out[f"pass_{p}_stride"] = 1 << (p - 1)
            out[f"pass_{p}_compulsory_share_of_peak"] = round(PASS_COMPULSORY * npix / sec * 1e-12 / PEAK_TBS, 4)
            out[f"pass_{p}_requested_TBps"] = round(PASS_REQUESTED * npix / sec * 1e-12, 3)
            out[f"denoise_{p}_over_accumulate_1"] = round(sp[f"denoise_{p}"]["median_ms"] /
                                                          sp["accumulate_1"]["median_ms"], 4)
    if rb is not None:
        rb.write_accum(r.accum())
        for p in range(1, 6):
            r.denoise(passes=p)
            rb.denoise(passes=p)
            out["ab"]["frames_equal"] = out["ab"]["frames_equal"] and bool(np.array_equal(r.framebuffer(),
                                                                                          rb.framebuffer()))
        for p in range(1, 6):
            v = spread(tb[f"pass_{p}"])
            out["ab"][f"pass_{p}"] = v
            if f"pass_{p}" in sp:
                out["ab"][f"pass_{p}_over_shipped"] = round(v["median_ms"] / sp[f"pass_{p}"]["median_ms"], 4)
                out["ab"][f"pass_{p}_quartiles_apart"] = bool(v["q3_ms"] < sp[f"pass_{p}"]["q1_ms"] or
                                                              sp[f"pass_{p}"]["q3_ms"] < v["q1_ms"])
        rb.close()
    if args.check:
        import denoise_reference as dr
        r.denoise(passes=5, depth_shift=8, color_shift=6)
        fb = r.framebuffer()
        g, base = r.denoise_guide()
        want = dr.denoise(r.accum(), g["pid"], g["depth_flags"] & np.uint32(0xFFFFFF),
                          (g["depth_flags"] & np.uint32(rt.RT_AOV_GEOM)) != 0, base, dr.unpack_normal(g["normal"]),
                          5, 8, 6)
        out["frame_equals_model"] = bool(np.array_equal(fb, want))
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
