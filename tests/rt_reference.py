"""An independent float64 model of what the RT path computes behind primary
visibility: the secondary-ray origin, the shadow verdict and the diffuse path
estimator of DESIGN 2.1 / 2.6.  TEST INFRASTRUCTURE ONLY.

Written from the meaning of the operations, in numpy float64.  Nothing here is
shared with oracle/ or the kernels: a triangle is met by crossing its plane
(s = n.(v0 - A) / n.D) and solving the 2x2 Gram system of its edges for the
crossing point's coordinates (no Moeller-Trumbore, no cross products of ray and
edge); bounce directions come from numpy.random.Generator (r = sqrt(u1), phi =
2 pi u2) in a basis made of the triangle's own first edge (no PCG, no disk
rejection, no Duff basis).

Space: a corner is its clip (x, y, w); the eye is the origin; pixel (x, y) looks
along d = ((x + 1/2) 2/W - 1, (y + 1/2) 2/H - 1, 1).  Which primitive a pixel
shows (`pid`) and its unlit colour (`plain`) are inputs: primary visibility and
shading are the raster's, pinned by the reference's goldens.
"""
from __future__ import annotations

import numpy as np

PULL = 2.0 ** -12          # P = o + d t (1 - 2^-12)
SKY = 0.25                 # an escaped bounce ray adds T * 0.25
EPS = 1e-4                 # slack below which a verdict is not compared
T_BOUND = 2.0 ** -14       # |t - t_model| <= 2^-14 |t_model|: a quarter of the pull-back

# the estimator's documented parts, each of which a variant can take out
# (check_sensitivity in rt_model_checks.py shows the tests notice)
TRUE = dict(uniform_hemisphere=False, face_normal=True, bounce_shadows=True, sky=True,
            pull=PULL, self_skip=True, segment_end=True, fixed_light=None,
            shared_draws=None)     # "pixels": one draw per sample for every pixel; "seeds": samples 2j, 2j + 1 share theirs


def variant(**kw):
    assert set(kw) <= set(TRUE), kw
    return dict(TRUE, **kw)


class Model:
    def __init__(self, prim_verts, drawcalls, width, height):
        """prim_verts float[P, 3, 10] (x, y, z, w, r, g, b, a, u, v per corner);
        drawcalls: objects with .states["depth_test"], .prim_offset, .prim_count"""
        pv = np.asarray(prim_verts, np.float64)
        self.W, self.H = int(width), int(height)
        geom = np.zeros(max(len(pv), 1), bool)
        for dc in drawcalls:
            geom[dc.prim_offset:dc.prim_offset + dc.prim_count] = bool(dc.states["depth_test"])
        self.is_geom = geom
        self.gid = np.flatnonzero(geom[:len(pv)])            # geometry index -> pid
        self.of_pid = np.full(max(len(pv), 1), -1)
        self.of_pid[self.gid] = np.arange(len(self.gid))
        c = pv[self.gid][:, :, (0, 1, 3)]                    # [T, 3 corners, 3]
        self.v0 = c[:, 0]
        self.e1, self.e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
        self.n = np.cross(self.e1, self.e2)                  # not unit; 0 for a degenerate triangle
        self.nlen = np.linalg.norm(self.n, axis=1)
        self.ok = self.nlen > 0
        with np.errstate(all="ignore"):
            self.nu = self.n / self.nlen[:, None]
            # dual basis of (e1, e2) in the triangle's plane from the 2x2 Gram system:
            # X - v0 = b1 e1 + b2 e2  <=>  b1 = (X - v0).g1, b2 = (X - v0).g2
            a, b, d = (self.e1 * self.e1).sum(1), (self.e1 * self.e2).sum(1), (self.e2 * self.e2).sum(1)
            det = a * d - b * b
            self.g1 = (d[:, None] * self.e1 - b[:, None] * self.e2) / det[:, None]
            self.g2 = (a[:, None] * self.e2 - b[:, None] * self.e1) / det[:, None]
        for arr in (self.nu, self.g1, self.g2):
            arr[~self.ok] = 0.0
        self.k0 = (self.v0 * self.nu).sum(1)                 # plane offsets
        self.k1, self.k2 = (self.v0 * self.g1).sum(1), (self.v0 * self.g2).sum(1)
        # one flat colour per triangle: floor(c * 255) / 255 per channel, what the
        # raster shows of an untextured triangle whose corners share a colour
        self.albedo = np.floor(pv[self.gid][:, 0, 4:7].astype(np.float32) * np.float32(255.0)) / 255.0
        e1u = self.e1 / np.maximum(np.linalg.norm(self.e1, axis=1), 1e-300)[:, None]
        self.tan1 = e1u                                      # in the plane, so orthogonal to nu
        self.tan2 = np.cross(self.nu, e1u)

    # ---- eye rays -----------------------------------------------------------
    def eye_dirs(self):
        x = (np.arange(self.W) + 0.5) * 2.0 / self.W - 1.0
        y = (np.arange(self.H) + 0.5) * 2.0 / self.H - 1.0
        d = np.empty((self.H, self.W, 3))
        d[..., 0], d[..., 1], d[..., 2] = x[None, :], y[:, None], 1.0
        return d

    def primary(self, pid):
        """pid int[H, W] (the raster's winner, -1 none) -> (rays bool[H, W]: a geometry
        pixel whose plane parameter is finite and > 0, t float64[H, W], tri int[H, W])"""
        pid = np.asarray(pid)
        tri = np.where(pid >= 0, self.of_pid[np.maximum(pid, 0)], -1)
        g = np.maximum(tri, 0)
        d = self.eye_dirs()
        with np.errstate(all="ignore"):
            t = self.k0[g] / (self.nu[g] * d).sum(-1)
        t = np.where(tri >= 0, t, 0.0)
        return (tri >= 0) & np.isfinite(t) & (t > 0), t, tri

    # ---- triangles met by A + s D ----------------------------------------------
    def _cross(self, A, D):
        """plane parameter s and edge coordinates b1, b2 of every ray on every
        triangle's plane, [R, T] each"""
        with np.errstate(all="ignore"):
            nd = D @ self.nu.T
            s = (self.k0[None, :] - A @ self.nu.T) / nd
            b1 = A @ self.g1.T - self.k1[None, :] + s * (D @ self.g1.T)
            b2 = A @ self.g2.T - self.k2[None, :] + s * (D @ self.g2.T)
        return nd, s, b1, b2

    def occluded(self, A, D, skip, smax=1.0):
        """some triangle other than `skip` meets the open segment A + s D, 0 < s < smax"""
        nd, s, b1, b2 = self._cross(A, D)
        hit = (nd != 0) & self.ok[None, :] & (s > 0) & (s < smax) & (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1)
        if skip is not None:
            hit[np.arange(len(A)), skip] = False
        return hit.any(1)

    def closest(self, A, D, skip):
        """-> (tri int[R] or -1, s float[R]): the nearest triangle other than `skip` along s > 0"""
        nd, s, b1, b2 = self._cross(A, D)
        hit = (nd != 0) & self.ok[None, :] & (s > 0) & (b1 >= 0) & (b2 >= 0) & (b1 + b2 <= 1)
        if skip is not None:
            hit[np.arange(len(A)), skip] = False
        s = np.where(hit, s, np.inf)
        k = s.argmin(1)
        sk = s[np.arange(len(A)), k]
        return np.where(np.isfinite(sk), k, -1), sk

    # ---- the shadow verdict with its margin ---------------------------------------
    def shadow_verdict(self, pid, light, eps=EPS, v=TRUE):
        """-> dict(rays, t, P, occluded, robust, margin), [H, W] each (P [H, W, 3]).
        occluded: some geometry triangle other than the pixel's own meets the open
        segment P -> light.  margin: the least slack of the deciding inequalities --
        for an occluded pixel the best occluder's least slack over its three
        coordinates, s against 0 and 1 and |cos(n, D)| against 0; for a lit pixel the
        least amount by which any triangle misses.  robust: margin > eps."""
        rays, t, tri = self.primary(pid)
        d = self.eye_dirs()
        P = d * (t * (1.0 - v["pull"]))[..., None]
        L = np.asarray(light if v["fixed_light"] is None else v["fixed_light"], np.float64)
        idx = np.flatnonzero(rays.reshape(-1))
        A = P.reshape(-1, 3)[idx]
        own = tri.reshape(-1)[idx]
        D = L[None, :] - A
        nd, s, b1, b2 = self._cross(A, D)
        with np.errstate(all="ignore"):
            cosv = nd / np.linalg.norm(D, axis=1)[:, None]            # n^ . D^
            b0 = 1.0 - b1 - b2
            hi = (1.0 - s) if v["segment_end"] else np.full_like(s, np.inf)
            inside = np.minimum(np.minimum(b0, b1), b2)
            slack = np.minimum(np.minimum(inside, np.minimum(s, hi)), np.abs(cosv))
            # a miss that needs no division by cos: the coordinates scaled by cos are
            # finite for an edge-on triangle too, and they sum to cos, so one above eps
            # and one below -eps means the line passes outside whatever the sign of cos
            q = (self.k0[None, :] - A @ self.nu.T) / np.linalg.norm(D, axis=1)[:, None]
            w1 = (A @ self.g1.T - self.k1[None, :]) * cosv + q * (D @ self.g1.T)
            w2 = (A @ self.g2.T - self.k2[None, :]) * cosv + q * (D @ self.g2.T)
            w0 = cosv - w1 - w2
            wmax = np.maximum(np.maximum(w0, w1), w2)
            wmin = np.minimum(np.minimum(w0, w1), w2)
            straddle = np.minimum(wmax, -wmin)
        slack = np.where(np.isfinite(slack), slack, -np.inf)
        hit = self.ok[None, :] & (nd != 0) & (inside >= 0) & (s > 0) & ((s < 1) | (not v["segment_end"]))
        # by how much a triangle misses: outside by a coordinate, or off the segment's
        # ends (either needs a plane that is not edge-on), or the straddle above
        clear = np.abs(cosv) > eps
        miss = np.where(clear, -np.minimum(inside, np.minimum(s, hi)), -np.inf)
        miss = np.maximum(miss, np.where(np.isfinite(straddle), straddle, -np.inf))
        miss = np.where(self.ok[None, :], miss, np.inf)
        r = np.arange(len(A))
        if v["self_skip"]:
            hit[r, own] = False
            slack[r, own] = -np.inf
            miss[r, own] = np.inf
        occ = hit.any(1)
        margin = np.where(occ, np.where(hit, slack, -np.inf).max(1), miss.min(1))
        out = dict(rays=rays, t=t, P=P)
        for name, val, fill in (("occluded", occ, False), ("margin", margin, np.inf)):
            full = np.full(self.W * self.H, fill, dtype=np.asarray(val).dtype)
            full[idx] = val
            out[name] = full.reshape(self.H, self.W)
        out["robust"] = out["margin"] > eps
        return out

    # ---- the path estimator ---------------------------------------------------------
    def path_samples(self, pid, plain, lights, bounces, samples, rng, v=TRUE, chunk=1 << 14, unrounded=False):
        """-> (idx int[n]: the flat indices of the path pixels, uint8[samples, n, 3]:
        independent 8-bit samples of every path pixel's colour).  plain uint32[H, W]:
        the unlit frame (ARGB), whose RGB / 255 is a path's first albedo.  lights: one
        (x, y, w) or several; with K lights a sample is the rounded mean
        (2 sum + K) // 2K of the K single-light 8-bit samples along the same path.
        unrounded (one light): float64 clamp(L) * 255 instead, before the rounding."""
        lights = np.atleast_2d(np.asarray(lights, np.float64))
        K = len(lights)
        rays, t, tri = self.primary(pid)
        idx = np.flatnonzero(rays.reshape(-1))
        n = len(idx)
        plain = np.asarray(plain, np.uint32).reshape(-1)[idx]
        alb0 = np.stack([(plain >> 16) & 0xFF, (plain >> 8) & 0xFF, plain & 0xFF], 1) / 255.0
        d0, t0, tri0 = self.eye_dirs().reshape(-1, 3)[idx], t.reshape(-1)[idx], tri.reshape(-1)[idx]
        out = np.empty((samples, n, 3), np.float64 if unrounded else np.uint8)
        per = max(1, chunk // max(n, 1))
        for s0 in range(0, samples, per):
            m = min(per, samples - s0)
            rep = lambda a: np.broadcast_to(a, (m,) + a.shape).reshape((m * n,) + a.shape[1:])
            val = self._paths(rep(d0), rep(t0), rep(tri0), rep(alb0), lights, bounces, rng, v, n)
            if unrounded:
                assert K == 1
                out[s0:s0 + m] = (np.clip(val[0], 0.0, 1.0) * 255.0).reshape(m, n, 3)
                continue
            s8 = np.floor(np.clip(val, 0.0, 1.0) * 255.0 + 0.5).astype(np.int64)   # [K, R, 3]
            out[s0:s0 + m] = ((2 * s8.sum(0) + K) // (2 * K)).reshape(m, n, 3)
        return idx, out

    def _paths(self, D, th, tri, T, lights, bounces, rng, v, n):
        """rays in blocks of n: every block holds the same n first vertices"""
        R = len(D)
        K = len(lights)
        Lsum = np.zeros((K, R, 3))
        live = np.arange(R)
        O = np.zeros((R, 3))
        D, th, tri, T = D.copy(), th.copy(), tri.copy(), T.copy()
        for vert in range(bounces + 1):
            if not len(live):
                break
            P = O + D * (th * (1.0 - v["pull"]))[:, None]
            nrm = self.nu[tri]
            if v["face_normal"]:                              # facing against the incoming ray
                nrm = np.where(((nrm * D).sum(1) > 0)[:, None], -nrm, nrm)
            skip = tri if v["self_skip"] else None
            for k, Lk in enumerate(lights if v["fixed_light"] is None else [v["fixed_light"]] * K):
                sd = np.asarray(Lk, np.float64)[None, :] - P
                if vert == 0:                                 # the same in every block: once
                    occ = np.tile(self.occluded(P[:n], sd[:n], None if skip is None else skip[:n],
                                                1.0 if v["segment_end"] else np.inf), R // n)
                elif v["bounce_shadows"]:
                    occ = self.occluded(P, sd, skip, 1.0 if v["segment_end"] else np.inf)
                else:
                    occ = np.zeros(len(P), bool)
                cosl = np.maximum(0.0, (nrm * sd).sum(1) / np.linalg.norm(sd, axis=1))
                Lsum[k, live] += T * np.where(occ, 0.0, cosl)[:, None]
            if vert == bounces:
                break
            if v["shared_draws"] == "pixels":
                u1, u2 = (rng.random(R // n)[live // n] for _ in range(2))
            elif v["shared_draws"] == "seeds":
                u1, u2 = (rng.random(((R // n + 1) // 2, n))[(live // n) // 2, live % n] for _ in range(2))
            else:
                u1, u2 = rng.random(len(live)), rng.random(len(live))
            phi = 2.0 * np.pi * u2
            if v["uniform_hemisphere"]:
                z = u1
                r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
            else:
                r = np.sqrt(u1)
                z = np.sqrt(np.maximum(0.0, 1.0 - u1))
            nd = (r * np.cos(phi))[:, None] * self.tan1[tri] + (r * np.sin(phi))[:, None] * self.tan2[tri] \
                + z[:, None] * nrm
            hit, s = self.closest(P, nd, skip)
            esc = hit < 0
            if v["sky"]:
                Lsum[:, live[esc]] += (T[esc] * SKY)[None]
            keep = ~esc
            live, O, D, th, tri = live[keep], P[keep], nd[keep], s[keep], hit[keep]
            T = T[keep] * self.albedo[tri]
        return Lsum


def moments(samples):
    """uint8[M, n, 3] -> (mean, variance) float64[n, 3] (variance unbiased)"""
    x = samples.astype(np.float64)
    return x.mean(0), x.var(0, ddof=1) if len(x) > 1 else np.zeros(x.shape[1:])
