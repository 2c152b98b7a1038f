"""The soft-shadow definition of include/vx_rt.h composed from the oracle's
exported primitives (oracle.py_oracle pt_key, pt_bounce_dir, trace_rays by brute
force) on tests/ao_reference.py's first vertex.  TEST INFRASTRUCTURE ONLY.

A ray pixel's sample of seed s for light i (centre L, radius R) is the segment
from P = d * (t * 0.999755859375f) to fmaf(R, u, L), u = pt_bounce_dir((P - L) /
|P - L|, pt_key(s, y * W + x, 64 + i)); it is occluded iff some geometry
triangle other than the pixel's own meets it at 0 < t < 1.  The six operations
this adds to the primitives -- subtract, dot3, sqrtf, divide, fmaf, subtract --
are restated in binary32: the plain ones are numpy float32 operations (one
IEEE rounding each), the fused ones exact rationals rounded once
(ray_reference.round_f32 over Fraction: fmaf).  Arrays go through fmaf_vec, the
same single rounding without a rational per element -- an exact float64 product,
the sum's exact error term, and the one case where rounding the float64 sum
again would differ settled by that term -- which tests/test_soft_cpu.py holds to
fmaf, ties included.
"""
from __future__ import annotations

import numpy as np

import ao_reference as ar
from ray_reference import frac, round_f32

VERTEX = 64   # light i's samples are keyed at path vertex 64 + i

_cache = {}


def fmaf(a, b, c) -> np.float32:
    """a * b + c rounded once"""
    return round_f32(frac(a) * frac(b) + frac(c))


def fmaf_vec(a, b, c) -> np.ndarray:
    """fmaf over float32 arrays (finite), rounded once.  Where the result is not well inside the normal
    range -- below 2^-120 in magnitude and not an exact zero -- the element goes through the rational fmaf.
    p = a * b is exact in float64 (48 bits).  s = fl64(p + c) with Knuth's error term e: p + c = s + e
    exactly.  Rounding s to float32 is rounding p + c unless s lies exactly midway between two float32
    values -- a float32 midpoint is a float64, so s = RN64(p + c) is never on the other side of one --
    and there e, when it is not 0, says which neighbour is nearer."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in np.broadcast_arrays(a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    f = s.astype(np.float32)
    assert np.isfinite(f).all()
    for other in (np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))):
        mid = (f.astype(np.float64) + other.astype(np.float64)) * 0.5
        toward = np.sign(other.astype(np.float64) - f.astype(np.float64))
        f = np.where((s == mid) & (e != 0) & (np.sign(e) == toward), other, f)
    f = f.astype(np.float32)
    small = (np.abs(s) < 2.0 ** -120) & ((s != 0) | (e != 0))
    for i in np.flatnonzero(small.reshape(-1)):
        f.reshape(-1)[i] = fmaf(a.reshape(-1)[i], b.reshape(-1)[i], c.reshape(-1)[i])
    return f


def dot3(a) -> np.ndarray:
    """rt_trace.h dot3(a, a) over rows: fmaf(a2, a2, fmaf(a1, a1, a0 * a0))"""
    a = np.asarray(a, np.float32)
    return fmaf_vec(a[..., 2], a[..., 2], fmaf_vec(a[..., 1], a[..., 1], a[..., 0] * a[..., 0]))


def light_frames(fv, light):
    """steps 2-5 per ray pixel -> (m float32[n, 3] unit, ok bool[n]: len is finite and not 0)"""
    L = np.asarray(light, np.float32)
    m = (fv["P"] - L[None, :]).astype(np.float32)
    with np.errstate(all="ignore"):
        ln = np.sqrt(dot3(m)).astype(np.float32)
    ok = np.isfinite(ln) & (ln != 0)
    return (m / np.where(ok, ln, np.float32(1.0))[:, None]).astype(np.float32), ok


def targets(u, light, radius):
    """step 7 -> float32[n, 3]"""
    L, R = np.asarray(light, np.float32), np.float32(radius)
    if R == 0:
        # fmaf(0, u, L) is L for every finite u: the product is an exact zero
        assert np.isfinite(u).all()
        return np.broadcast_to(L, u.shape).astype(np.float32)
    return fmaf_vec(R, np.asarray(u, np.float32), L[None, :])


def verdicts(sc, W, H, lights, radii, seed, S, pid, t, with_rays=False):
    """Per-sample verdicts uint8[n, S, H, W] of samples seed .. seed + S - 1 under each of the n lights
    (0 off the ray pixels): the composition by brute force.  with_rays: also (fv, dirs[i][j] float32[rays,
    3]: target - P of light i, sample j)."""
    from oracle import py_oracle as po
    assert len(lights) == len(radii)
    fv = ar.first_vertex(sc, W, H, pid, t)
    nr = len(fv["idx"])
    out = np.zeros((len(lights), S, H * W), np.uint8)
    dirs = []
    for i, (light, radius) in enumerate(zip(lights, radii)):
        dirs.append([])
        if nr == 0:
            dirs[i] = [np.zeros((0, 3), np.float32)] * S
            continue
        m, ok = light_frames(fv, light)
        for j in range(S):
            key = po.pt_key(np.full(nr, (seed + j) & 0xFFFFFFFF, np.uint32), fv["idx"].astype(np.uint32),
                            np.full(nr, VERTEX + i, np.uint32))
            u = po.pt_bounce_dir(m, key)
            D = (targets(u, light, radius) - fv["P"]).astype(np.float32)
            dirs[i].append(D)
            rays = np.zeros((nr, 8), np.float32)
            rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = fv["P"], D, 0.0, 1.0
            _, _, occ = po.trace_rays(fv["tri9"], rays, fv["tri"].astype(np.int32), np.zeros(nr, np.uint8))
            out[i, j, fv["idx"]] = np.where(ok, occ, 0)
    out = out.reshape(len(lights), S, H, W)
    return (out, fv, dirs) if with_rays else out


def cached_verdicts(name, sc, W, H, lights, radii, seed, S, pid, t):
    """verdicts() once per process and case (the tests share it and leave it unchanged)"""
    key = (name, W, H, tuple(map(tuple, lights)), tuple(float(r) for r in radii), seed, S)
    if key not in _cache:
        _cache[key] = verdicts(sc, W, H, lights, radii, seed, S, pid, t, with_rays=True)
    return _cache[key]
