"""An exact model of the ray routines (kernels/rt_trace.h, kernels/rt_path.h;
oracle/rt.c restates them), written from their definitions and sharing no
code with either: Möller-Trumbore and the ray / box interval in rationals
(fractions.Fraction of the float32 bit patterns, and the same in int64 for
whole tables of lattice inputs), the closest hit of a ray over a triangle
list under the kernels' order, PCG and the bounce key in Python integers
(DESIGN.md 2.1, O'Neill's published constants), the hash -> [-1, 1) map, the
disk rejection sampler and the lifted direction in float64.

Ray / triangle: with pvec = d x e2, det = e1 . pvec, tvec = o - v0,
u = tvec . pvec / det, qvec = tvec x e1, v = d . qvec / det,
t = e2 . qvec / det, the ray o + t d meets the triangle (v0, v0 + e1,
v0 + e2) iff det != 0, u >= 0, v >= 0, u + v <= 1 (edges and vertices
included), and counts iff t > tmin; the reported t is the rational rounded to
the nearest float32, ties to even.  Where t is compared with a limit that is
not a tie of rationals (closer(), tmax) the rounded value is what is compared:
that is the only value a float32 routine can hand to the comparison.
"""
from fractions import Fraction

import numpy as np

PT_TRIES = 8


# ---- float32 <-> rationals --------------------------------------------------
def frac(x) -> Fraction:
    """the exact value of a float32"""
    return Fraction(float(np.float32(x)))


def round_f32(q: Fraction) -> np.float32:
    """q rounded to the nearest float32, ties to even (|q| below the float32
    range's end; subnormals included)"""
    if q == 0:
        return np.float32(0.0)
    s, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    qe = max(e - 23, -149)                       # the quantum's exponent
    m = a / Fraction(2) ** qe
    n, r = divmod(m.numerator, m.denominator)
    twice = 2 * r
    if twice > m.denominator or (twice == m.denominator and (n & 1)):
        n += 1
    v = float(s * n * Fraction(2) ** qe)         # exact: n <= 2^24, a float32 value
    assert v == np.float32(v)
    return np.float32(v)


def next_f32(x, up=True) -> np.float32:
    return np.nextafter(np.float32(x), np.float32(np.inf if up else -np.inf), dtype=np.float32)


# ---- ray / triangle ---------------------------------------------------------
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def mt_exact(o, d, v0, e1, e2, tmin, inclusive=True, strict_tmin=True):
    """(verdict, t rounded to float32 or None, (u, v, t) rationals or None);
    `inclusive` / `strict_tmin` False are the mutants check_sensitivity uses."""
    o, d, v0, e1, e2 = ([frac(x) for x in a] for a in (o, d, v0, e1, e2))
    pvec = _cross(d, e2)
    det = _dot(e1, pvec)
    if det == 0:
        return False, None, None
    tvec = [o[k] - v0[k] for k in range(3)]
    u = _dot(tvec, pvec) / det
    qvec = _cross(tvec, e1)
    v = _dot(d, qvec) / det
    t = _dot(e2, qvec) / det
    tm = frac(tmin)
    if inclusive:
        inside = u >= 0 and v >= 0 and u + v <= 1
    else:
        inside = u > 0 and v > 0 and u + v < 1
    ok = inside and (t > tm if strict_tmin else t >= tm)
    return ok, round_f32(t), (u, v, t)


def on_boundary(uvt) -> bool:
    """the hit point lies on an edge or a vertex of the triangle"""
    u, v, _ = uvt
    return u == 0 or v == 0 or u + v == 1


def mt_lattice(o, d, v0, e1, e2):
    """The same quantities for whole tables of integer inputs, in int64 (the
    caller keeps every product below 2^62): o, d [R, 3]; v0, e1, e2 [T, 3] ->
    det, un, vn, tn int64[R, T] with u = un / det, v = vn / det, t = tn / det."""
    o, d = (np.asarray(a, np.int64)[:, None, :] for a in (o, d))
    v0, e1, e2 = (np.asarray(a, np.int64)[None, :, :] for a in (v0, e1, e2))
    cr = lambda a, b: np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                                a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)
    dt = lambda a, b: (a * b).sum(-1)
    pvec = cr(d, e2)
    det = dt(e1, pvec)
    tvec = o - v0
    un = dt(tvec, pvec)
    qvec = cr(tvec, e1)
    vn = dt(d, qvec)
    tn = dt(e2, qvec)
    return det, un, vn, tn


def lattice_hits(o, d, v0, e1, e2, inclusive=True):
    """-> (inside bool[R, T], t float32[R, T] correctly rounded, boundary bool[R, T]).
    |tn|, |det| < 2^53 are exact in float64, and a float64 quotient rounded
    again to float32 is the correctly rounded quotient (53 >= 2 * 24 + 2)."""
    det, un, vn, tn = mt_lattice(o, d, v0, e1, e2)
    sg = np.sign(det)
    un, vn, ad = un * sg, vn * sg, det * sg
    if inclusive:
        inside = (det != 0) & (un >= 0) & (vn >= 0) & (un + vn <= ad)
    else:
        inside = (det != 0) & (un > 0) & (vn > 0) & (un + vn < ad)
    assert np.abs(tn).max(initial=0) < 2 ** 53 and np.abs(det).max(initial=0) < 2 ** 53
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (tn.astype(np.float64) / det.astype(np.float64)).astype(np.float32)
    boundary = inside & ((un == 0) | (vn == 0) | (un + vn == ad))
    return inside, t, boundary


def closer(t, pid, bt, bpid, tie_high):
    """the kernels' closest-hit order: t, then pid by the depth-compare tie rule"""
    return t < bt or (t == bt and (pid > bpid if tie_high else pid < bpid))


def closest_hits(inside, t, tmin, tmax, skip, tie_high, strict_tmin=True, use_skip=True,
                 flip_tie=False):
    """Per ray the closest hit over the list in ascending pid order: starts at
    (tmax, -1), a hit counts iff t > tmin and replaces the best iff closer().
    -> (pid int32[R] or -1, t float32[R] (0 on a miss), occluded bool[R]: some
    hit with tmin < t < tmax)."""
    R, T = inside.shape
    tmin, tmax = np.asarray(tmin, np.float32), np.asarray(tmax, np.float32)
    skip = np.asarray(skip, np.int64)
    tie = np.asarray(tie_high, bool) ^ flip_tie
    pids = np.arange(T)[None, :]
    ok = inside & ((t > tmin[:, None]) if strict_tmin else (t >= tmin[:, None]))
    if use_skip:
        ok &= pids != skip[:, None]
    occ = (ok & (t < tmax[:, None])).any(1)
    bt = tmax.copy()
    bp = np.full(R, -1, np.int64)
    for p in range(T):          # ascending pid: closer() as the routines apply it
        tp, okp = t[:, p], ok[:, p]
        better = okp & ((tp < bt) | ((tp == bt) & np.where(tie, p > bp, p < bp)))
        bt = np.where(better, tp, bt)
        bp = np.where(better, p, bp)
    return bp.astype(np.int32), np.where(bp >= 0, bt, np.float32(0)).astype(np.float32), occ


# ---- ray / box ----------------------------------------------------------------
def box_interval(o, d, lo, hi):
    """The interval of t with o + t d inside the closed box [lo, hi], in
    rationals: (t0, t1), either None where unbounded, empty where t0 > t1; a
    zero direction component puts a side condition on the origin (lo <= o <=
    hi) in place of an interval, and None is returned where it fails.
    Infinite planes bound nothing."""
    pl = lambda x: float(x) if np.isinf(x) else frac(x)
    return _interval_frac(o, d, [pl(x) for x in lo], [pl(x) for x in hi])


def box_meets(o, d, lo, hi, tmin, tmax, shrink=Fraction(0)):
    """whether the ray meets the box within [tmin, tmax]; `shrink` > 0 first
    moves every plane inward by shrink * max(|lo|, |hi|, |o|) of its axis (a
    box that turns inside out meets nothing)"""
    lo2, hi2 = [], []
    for k in range(3):
        if np.isinf(lo[k]) or np.isinf(hi[k]):
            lo2.append(lo[k]); hi2.append(hi[k])
            continue
        s = shrink * max(abs(frac(lo[k])), abs(frac(hi[k])), abs(frac(o[k])))
        l, h = frac(lo[k]) + s, frac(hi[k]) - s
        if l > h:
            return False
        lo2.append(l); hi2.append(h)
    iv = _interval_frac(o, d, lo2, hi2)
    if iv is None:
        return False
    t0, t1 = iv
    a = frac(tmin) if t0 is None else max(t0, frac(tmin))
    tm = None if np.isinf(tmax) else frac(tmax)
    b = tm if t1 is None else (t1 if tm is None else min(t1, tm))
    return b is None or a <= b


def _interval_frac(o, d, lo, hi):
    """box_interval over planes already rational (or +-inf floats)"""
    t0 = t1 = None
    for k in range(3):
        ok, dk = frac(o[k]), frac(d[k])
        linf = isinstance(lo[k], (float, np.floating)) and np.isinf(lo[k])
        hinf = isinstance(hi[k], (float, np.floating)) and np.isinf(hi[k])
        if (linf and lo[k] > 0) or (hinf and hi[k] < 0):
            return None
        lk, hk = (None if linf else Fraction(lo[k])), (None if hinf else Fraction(hi[k]))
        if dk == 0:
            if (lk is not None and ok < lk) or (hk is not None and ok > hk):
                return None
            continue
        a = None if lk is None else (lk - ok) / dk
        b = None if hk is None else (hk - ok) / dk
        if dk < 0:
            a, b = b, a
        if a is not None and (t0 is None or a > t0):
            t0 = a
        if b is not None and (t1 is None or b < t1):
            t1 = b
    return t0, t1


# ---- PCG and the sampler ------------------------------------------------------
M32 = 0xFFFFFFFF


def pcg_hash(v: int) -> int:
    """PCG-RXS-M-XS 32 as a hash of v: one LCG step
    (multiplier 747796405, increment 2891336453), a random xorshift by the top
    four bits + 4, the multiplier 277803737, a last xorshift by 22"""
    state = (v * 747796405 + 2891336453) & M32
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & M32
    return ((word >> 22) ^ word) & M32


def pt_key(seed: int, px: int, v: int) -> int:
    """the bounce stream's key of (seed, pixel, vertex): the vertex spread by
    the golden-ratio constant, hashed with the seed, then with the pixel"""
    return pcg_hash(px ^ pcg_hash((seed ^ (0x9E3779B9 * (v + 1))) & M32))


def pt_u11(h: int) -> float:
    """the top 24 bits of h as a point of [-1, 1): (h >> 8) / 2^23 - 1 (exact in float64)"""
    return (h >> 8) / 8388608.0 - 1.0


def disk_tries(key: int, pair_stride: int = 2):
    """the sampler's PT_TRIES candidate points (a, b) in float64 with their
    a^2 + b^2: try i reads the stream at key + 2 i and key + 2 i + 1
    (pair_stride 1: the mutant reading key + i, key + i + 1)"""
    out = []
    for i in range(PT_TRIES):
        a = pt_u11(pcg_hash((key + pair_stride * i) & M32))
        b = pt_u11(pcg_hash((key + pair_stride * i + 1) & M32))
        out.append((a, b, a * a + b * b))
    return out


def disk_class(key: int, margin: float = 1e-6):
    """0: every try is rejected by more than `margin` (the fall-back); k in
    1..8: tries 1..k-1 rejected and try k accepted, each by more than
    `margin`; None: some decisive try lies within the margin"""
    for i, (_, _, r2) in enumerate(disk_tries(key)):
        if abs(r2 - 1.0) <= margin:
            return None
        if r2 < 1.0:
            return i + 1
    return 0


def duff_basis(n):
    """The orthonormal basis (t1, t2) about unit n of Duff et al. 2017, in
    float64 from its definition: s = sign(n.z) (+1 at +-0 with the sign bit
    clear ... n.z >= 0), a = -1 / (s + n.z), b = n.x n.y a,
    t1 = (1 + s n.x^2 a, s b, -s n.x), t2 = (b, s + n.y^2 a, -n.y)."""
    x, y, z = (float(c) for c in n)
    s = 1.0 if z >= 0.0 else -1.0
    a = -1.0 / (s + z)
    b = x * y * a
    return np.array([1.0 + s * x * x * a, s * b, -s * x]), np.array([b, s + y * y * a, -y])


def gram_schmidt_basis(n):
    """an orthonormal pair about n by Gram-Schmidt from the axis least aligned with n"""
    n = np.asarray(n, np.float64)
    e = np.zeros(3)
    e[int(np.argmin(np.abs(n)))] = 1.0
    t1 = e - n * (e @ n)
    t1 /= np.linalg.norm(t1)
    return t1, np.cross(n, t1)


def bounce_model(n, key, pair_stride=2, fallback="pole"):
    """The bounce direction in float64: the first try inside the unit disk
    gives (x, y), none gives (0, 0) -- the pole (fallback "last": the mutant
    keeping the last rejected pair, clamped onto the disk's rim); z = sqrt(1 -
    x^2 - y^2); dir = x t1 + y t2 + z n.  -> (dir, x, y, z)"""
    x = y = 0.0
    tries = disk_tries(key, pair_stride)
    for a, b, r2 in tries:
        if r2 < 1.0:
            x, y = a, b
            break
    else:
        if fallback == "last":
            a, b, r2 = tries[-1]
            x, y = a / np.sqrt(r2), b / np.sqrt(r2)
    z = float(np.sqrt(max(0.0, 1.0 - x * x - y * y)))
    t1, t2 = duff_basis(n)
    return x * t1 + y * t2 + z * np.asarray(n, np.float64), x, y, z
