"""The ambient-occlusion definition of include/vx_rt.h composed from the
oracle's exported primitives (oracle.py_oracle pt_key, pt_normal, pt_bounce_dir,
trace_rays by brute force), and a float64 verdict with a margin for the same
rays from tests/rt_reference.py's Model.  TEST INFRASTRUCTURE ONLY.

A ray pixel is a geometry pixel whose plane t is finite and > 0; its sample of
seed s starts at P = d * (t * 0.999755859375f) along pt_bounce_dir(pt_normal(e1,
e2, d), pt_key(s, y * W + x, 0)) and is occluded iff some geometry triangle
other than the pixel's own meets it at 0 < t < radius.
"""
from __future__ import annotations

import numpy as np

PULL32 = np.float32(0.999755859375)
EPS = 1e-4   # slack below which the float64 model does not decide (rt_reference.EPS)

_cache = {}


def geometry(sc):
    """-> (gid int[T]: geometry index -> pid, of_pid int[P], tri9 float32[T, 9]: v0, e1, e2 in
    clip (x, y, w)) of a cgltrace scene, as rt_reference.Model lists them"""
    pv = np.asarray(sc.prim_verts, np.float32)
    geom = np.zeros(max(len(pv), 1), bool)
    for dc in sc.drawcalls:
        geom[dc.prim_offset:dc.prim_offset + dc.prim_count] = bool(dc.states["depth_test"])
    gid = np.flatnonzero(geom[:len(pv)])
    of_pid = np.full(max(len(pv), 1), -1)
    of_pid[gid] = np.arange(len(gid))
    c = pv[gid][:, :, (0, 1, 3)]
    v0 = c[:, 0]
    e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    return gid, of_pid, np.ascontiguousarray(np.concatenate([v0, e1, e2], 1), np.float32)


def ray_pixels(pid, t, of_pid):
    """the ray pixels of the oracle's pid / t [H, W] -> (mask bool[H, W], tri int[H, W])"""
    pid = np.asarray(pid)
    t = np.asarray(t, np.float32)
    tri = np.where(pid >= 0, of_pid[np.maximum(pid, 0)], -1)
    return (tri >= 0) & (t > 0) & np.isfinite(t), tri


def first_vertex(sc, W, H, pid, t):
    """-> dict(rays bool[H, W], idx int[n]: the ray pixels' y * W + x, tri int[n], P float32[n, 3],
    n float32[n, 3], tri9)"""
    from oracle import py_oracle as po
    _, of_pid, tri9 = geometry(sc)
    rays, tri = ray_pixels(pid, t, of_pid)
    idx = np.flatnonzero(rays.reshape(-1))
    x, y = (idx % W).astype(np.float32), (idx // W).astype(np.float32)
    sx, sy = np.float32(2.0) / np.float32(W), np.float32(2.0) / np.float32(H)
    # primary_dir: fmaf((x + 0.5), sx, -1); the product is formed in float64 (exact: two binary32
    # factors) and rounded once with the addend, which is the fused operation
    d = np.empty((len(idx), 3), np.float32)
    d[:, 0] = ((x + np.float32(0.5)).astype(np.float64) * np.float64(sx) - 1.0).astype(np.float32)
    d[:, 1] = ((y + np.float32(0.5)).astype(np.float64) * np.float64(sy) - 1.0).astype(np.float32)
    d[:, 2] = 1.0
    tt = np.asarray(t, np.float32).reshape(-1)[idx] * PULL32
    P = (d * tt[:, None]).astype(np.float32)
    g = tri.reshape(-1)[idx]
    n = po.pt_normal(tri9[g, 3:6], tri9[g, 6:9], d) if len(idx) else np.zeros((0, 3), np.float32)
    return dict(rays=rays, idx=idx, tri=g, P=P, n=n, tri9=tri9)


def sample_rays(fv, seed):
    """the rays of sample seed `seed` -> float32[n, 3] directions"""
    from oracle import py_oracle as po
    n = len(fv["idx"])
    if n == 0:
        return np.zeros((0, 3), np.float32)
    key = po.pt_key(np.full(n, seed & 0xFFFFFFFF, np.uint32), fv["idx"].astype(np.uint32), np.zeros(n, np.uint32))
    return po.pt_bounce_dir(fv["n"], key)


def verdicts(sc, W, H, seed, radius, S, pid, t, with_rays=False):
    """Per-sample verdicts uint8[S, H, W] of samples seed .. seed + S - 1 (0 off the ray pixels):
    the composition by brute force.  with_rays: also (fv, [directions per sample])."""
    from oracle import py_oracle as po
    fv = first_vertex(sc, W, H, pid, t)
    out = np.zeros((S, H * W), np.uint8)
    dirs = []
    n = len(fv["idx"])
    for j in range(S):
        D = sample_rays(fv, seed + j)
        dirs.append(D)
        if n == 0:
            continue
        rays = np.zeros((n, 8), np.float32)
        rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = fv["P"], D, 0.0, np.float32(radius)
        _, _, occ = po.trace_rays(fv["tri9"], rays, fv["tri"].astype(np.int32), np.zeros(n, np.uint8))
        out[j, fv["idx"]] = occ
    out = out.reshape(S, H, W)
    return (out, fv, dirs) if with_rays else out


def cached_verdicts(name, sc, W, H, seed, radius, S, pid, t):
    """verdicts() once per process and case (the tests share it and leave it unchanged)"""
    key = (name, W, H, seed, float(radius), S)
    if key not in _cache:
        _cache[key] = verdicts(sc, W, H, seed, radius, S, pid, t, with_rays=True)
    return _cache[key]


def model_verdict(model, A, D, own, radius, eps=EPS):
    """The float64 verdict of rays A + s D (float[n, 3] each; own int[n]: the origin's triangle,
    skipped) against every triangle of rt_reference.Model `model`, 0 < s < radius
    -> (occluded bool[n], robust bool[n]).
    Occluded is robust when some other triangle has every one of s, radius - s, b0, b1, b2 above
    eps; clear is robust when every other triangle misses by more than eps and none is within eps
    of edge-on."""
    A, D = np.asarray(A, np.float64), np.asarray(D, np.float64)
    nd, s, b1, b2 = model._cross(A, D)
    with np.errstate(all="ignore"):
        cosv = nd / np.linalg.norm(D, axis=1)[:, None]
        b0 = 1.0 - b1 - b2
        hi = np.full_like(s, np.inf) if np.isinf(radius) else float(radius) - s
        slack = np.minimum(np.minimum(np.minimum(b0, b1), b2), np.minimum(s, hi))
    slack = np.where(np.isfinite(slack) | (slack == np.inf), slack, -np.inf)
    other = model.ok[None, :] & (nd != 0)
    r = np.arange(len(A))
    mine = np.zeros_like(other)
    mine[r, own] = True
    other &= ~mine
    hit = other & (slack >= 0)
    occ = hit.any(1)
    sure_hit = (other & (slack > eps)).any(1)
    # a triangle that counts for nothing: the ray's own, a degenerate one
    ignore = mine | ~model.ok[None, :]
    sure_miss = (ignore | ((slack < -eps) & (np.abs(cosv) > eps))).all(1)
    return occ, np.where(occ, sure_hit, sure_miss)
