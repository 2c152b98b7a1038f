"""Known answers and input tables for the ray routines (tests/
test_ray_kat_cpu.py holds the oracle to them, tests/test_gpu_ray_kat.py the
rt_kat image).  The known answers are worked by hand below; the tables are
inputs only -- expected values come from tests/ray_reference.py."""
import numpy as np

import ray_reference as rr

INF = float("inf")

# ---- PCG (ray_reference.pcg_hash's steps, by hand) --------------------------
# pcg_hash(0): state = 0 * 747796405 + 2891336453 = 0xAC564B05; its top four
#   bits are 0xA = 10, so the xorshift is by 14: state >> 14 = 0x2B159,
#   0xAC564B05 ^ 0x0002B159 = 0xAC54FA5C; times 277803737 mod 2^32 = 0x07BB2FFC;
#   0x07BB2FFC >> 22 = 0x1E, 0x07BB2FFC ^ 0x1E = 0x07BB2FE2.
# pcg_hash(1): state = 747796405 + 2891336453 = 3639132858 = 0xD8E8C2BA; top
#   bits 0xD = 13, shift 17: >> 17 = 0x6C74, xor = 0xD8E8AECE; times 277803737
#   = 0xA8BEE89E; >> 22 = 0x2A2, xor = 0xA8BEEA3C.
# pcg_hash(0xFFFFFFFF): state = 2891336453 - 747796405 = 2143540048 =
#   0x7FC3D350; top bits 7, shift 11: >> 11 = 0xFF87A, xor = 0x7FCC2B2A; times
#   277803737 = 0xE62A4A9A; >> 22 = 0x398, xor = 0xE62A4902.
PCG_KAT = [(0, 0x07BB2FE2), (1, 0xA8BEEA3C), (0xFFFFFFFF, 0xE62A4902)]
# pt_key(seed 0x5EED, pixel 7, vertex 2): 0x9E3779B9 * (2 + 1) = 0x1DAA66D2B,
#   low word 0xDAA66D2B; ^ 0x5EED = 0xDAA633C6; pcg_hash of that = 0x90BFCE49;
#   ^ 7 = 0x90BFCE4E; pcg_hash of that = 0xFF5DA5DA.
PT_KEY_KAT = [((0x5EED, 7, 2), 0xFF5DA5DA)]
# pt_u11: (h >> 8) * 2^-23 - 1: 0 -> -1; 0x80000000 -> 0x800000 * 2^-23 - 1 = 0;
#   0xFFFFFFFF -> (2^24 - 1) * 2^-23 - 1 = 1 - 2^-23.
PT_U11_KAT = [(0, -1.0), (0x80000000, 0.0), (0xFFFFFFFF, 1.0 - 2.0 ** -23)]

# ---- ray / triangle -----------------------------------------------------------
# The triangle A = (0, 0, 0), B = (4, 0, 0), C = (0, 4, 0): v0 = A, e1 = (4, 0, 0),
# e2 = (0, 4, 0).  A ray from (x, y, -2) along d = (0, 0, 4) meets its plane at
# t = 1/2 in the point (x, y) = (4 u, 4 v): pvec = d x e2 = (-16, 0, 0),
# det = e1 . pvec = -64; tvec = (x, y, -2), u = tvec . pvec / det = x / 4;
# qvec = tvec x e1 = (0, -8, -4 y), v = d . qvec / det = -16 y / -64 = y / 4,
# t = e2 . qvec / det = -32 / -64 = 1/2.
_T = ((0, 0, 0), (4, 0, 0), (0, 4, 0))
_HALF_BELOW = float(np.nextafter(np.float32(0.5), np.float32(0)))  # 0.5 - 2^-25
#            o            d           tri  tmin        verdict  t
MT_KAT = [
    ((1, 1, -2), (0, 0, 4), _T, 0.0, True, 0.5),     # interior: u = v = 1/4
    ((2, 0, -2), (0, 0, 4), _T, 0.0, True, 0.5),     # on edge AB: v = 0
    ((0, 2, -2), (0, 0, 4), _T, 0.0, True, 0.5),     # on edge AC: u = 0
    ((2, 2, -2), (0, 0, 4), _T, 0.0, True, 0.5),     # on edge BC: u + v = 1
    ((0, 0, -2), (0, 0, 4), _T, 0.0, True, 0.5),     # vertex A: u = v = 0
    ((4, 0, -2), (0, 0, 4), _T, 0.0, True, 0.5),     # vertex B: u = 1
    ((0, 4, -2), (0, 0, 4), _T, 0.0, True, 0.5),     # vertex C: v = 1
    ((2, -1, -2), (0, 0, 4), _T, 0.0, False, None),  # one unit outside AB: v = -1/4
    ((3, 2, -2), (0, 0, 4), _T, 0.0, False, None),   # outside BC: u + v = 5/4
    ((1, 1, -2), (1, 0, 0), _T, 0.0, False, None),   # parallel to the plane: det = 0
    ((1, 1, 0), (1, 1, 0), _T, 0.0, False, None),    # inside the plane: det = 0
    # back face: from above, d = (0, 0, -4): pvec = (16, 0, 0), det = 64,
    # tvec = (1, 1, 2): u = 16 / 64, qvec = (0, 8, -4), v = 16 / 64, t = 32 / 64
    ((1, 1, 2), (0, 0, -4), _T, 0.0, True, 0.5),
    ((1, 1, -2), (0, 0, 4), _T, 0.5, False, None),   # t == tmin: the comparison is strict
    ((1, 1, -2), (0, 0, 4), _T, _HALF_BELOW, True, 0.5),  # t the next float above tmin
    ((1, 1, 2), (0, 0, 4), _T, 0.0, False, None),    # the plane behind the origin: t = -1/2
    ((1, 1, 2), (0, 0, 4), _T, -1.0, True, -0.5),    # ... which a negative tmin admits
    # zero area: e2 = 2 e1, and a point triangle: det = 0
    ((1, 1, -2), (0, 0, 4), ((0, 0, 0), (4, 0, 0), (8, 0, 0)), 0.0, False, None),
    ((0, 0, -2), (0, 0, 4), ((0, 0, 0), (0, 0, 0), (0, 0, 0)), 0.0, False, None),
]


def mt_kat_arrays():
    o = np.array([r[0] for r in MT_KAT], np.float32)
    d = np.array([r[1] for r in MT_KAT], np.float32)
    tri = np.array([r[2] for r in MT_KAT], np.float32)
    tmin = np.array([r[3] for r in MT_KAT], np.float32)
    return o, d, tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], tmin


# ---- ray / box --------------------------------------------------------------
# Directions are powers of two, so inv = 1 / d, o * inv and plane * inv - o * inv
# are exact and the routine's tnear / tfar are the interval's ends themselves.
# From o = (0, 0, 0) along d = (2, 1/2, -1): x in [2, 4] gives t in [1, 2],
# y in [1, 2] gives [2, 4], z in [-4, -2] gives [2, 4] (d.z < 0: the planes swap).
F16_MAX, F16_INF = 0x7BFF, 0x7C00
#   o, d, (lo.x, hi.x, lo.y, hi.y, lo.z, hi.z), tmin, tmax, verdict, tnear, tfar
SLAB_KAT = [
    ((0, 0, 0), (2, .5, -1), (2, 4, 1, 2, -4, -2), 0, INF, True, 2.0, 2.0),     # touches at t = 2
    ((0, 0, 0), (2, .5, -1), (2, 3, 1, 2, -4, -2), 0, INF, False, 2.0, 1.5),    # x leaves at 3/2
    ((0, 0, 0), (2, .5, -1), (2, 8, 1, 2, -4, -2), 0, INF, True, 2.0, 4.0),
    ((0, 0, 0), (2, .5, -1), (2, 8, 1, 2, -4, -2), 3, INF, True, 3.0, 4.0),     # tmin inside
    ((0, 0, 0), (2, .5, -1), (2, 8, 1, 2, -4, -2), 0, 2, True, 2.0, 2.0),       # tmax at tnear
    ((0, 0, 0), (2, .5, -1), (2, 8, 1, 2, -4, -2), 0, 1.5, False, 2.0, 1.5),    # tmax before
    ((0, 0, 0), (2, .5, -1), (2, 8, 1, 2, -4, -2), 4.5, INF, False, 4.5, 4.0),  # tmin behind
    ((1, 1, 1), (-1, -1, -1), (-2, 0, -2, 0, -2, 0), 0, INF, True, 1.0, 3.0),   # all negative
    ((3, 0, 0), (4, 4, 4), (1, 5, -1, 1, -1, 1), 0, INF, True, 0.0, 0.25),      # starts inside
    # a plane at binary16's largest value: x in [0, 65504], d.x = 32768: t <= 65504 / 32768
    ((0, 0, 0), (32768, 1, 1), (0, 65504, -1, 4, -1, 4), 0, INF, True, 0.0, 1.9990234375),
]
# rows over binary16 planes as a rt_node4h_t holds them: (o, d, halves (lo.x,
# hi.x, ...), tmin, tmax, verdict, tnear, tfar).  65504 = 0x7BFF is the last
# finite one; a plane past it rounds outward to +-inf = 0x7C00 / 0xFC00 and then
# bounds nothing: inf * inv - oi = +-inf, which min / max drop.
SLAB_HALF_KAT = [
    # x in [1, 65504] with d.x = 32768: t in [2^-15, 65504 / 32768]; y, z in [-1, 1], d = 1
    ((0, 0, 0), (32768, 1, 1), (0x3C00, F16_MAX, 0xBC00, 0x3C00, 0xBC00, 0x3C00), 0, INF,
     True, 2.0 ** -15, 1.0),
    # hi.x = +inf, lo.x = -inf: only y and z bound: [-1, 1] each from o = 0: tfar = 1
    ((0, 0, 0), (32768, 1, 1), (0xFC00, F16_INF, 0xBC00, 0x3C00, 0xBC00, 0x3C00), 0, INF,
     True, 0.0, 1.0),
    # the same box met from outside in y: o.y = -3: y enters at 2, leaves at 4; z leaves at 1
    ((0, -3, 0), (32768, 1, 1), (0xFC00, F16_INF, 0xBC00, 0x3C00, 0xBC00, 0x3C00), 0, INF,
     False, 2.0, 1.0),
]


def half_to_f32(h):
    return np.array(h, np.uint16).view(np.float16).astype(np.float32)


# ---- closer at a tie ----------------------------------------------------------
# Two copies of _T as pids 0 and 1, the ray ((1, 1, -2), (0, 0, 4)): both at
# t = 1/2.  Ascending pid order: pid 0 becomes the best (1/2 < tmax); pid 1
# ties it and replaces it only under tie_high (1 > 0).  With tmax = 1/2 the
# first candidate ties the start (tmax, -1): 0 > -1 holds, 0 < -1 does not, so
# tie_high reports pid 1 at t = 1/2 and the low rule reports a miss.
#   tmax, tie_high -> pid, t
CLOSER_KAT = [(INF, False, 0, 0.5), (INF, True, 1, 0.5), (0.5, True, 1, 0.5), (0.5, False, -1, 0.0)]


# ---- tables: Möller-Trumbore ---------------------------------------------------
def mt_lattice_table(n=20000, seed=7):
    """Integer records: vertices and origins in [-16, 16] (the centroid
    quarter in [-10, 10] so that |d| <= 60), |d| <= 64; a quarter each aimed
    at a random lattice point, the midpoint of an edge (t = 1/2), a vertex
    (t = 1), the centroid (t = 1/3).  tmin cycles 0, 1/2, 1.
    -> o, d, v0, e1, e2 int64[n, 3], tmin float32[n]"""
    rng = np.random.default_rng(seed)
    q = n // 4
    r = lambda lim, m: rng.integers(-lim, lim + 1, size=(m, 3))
    a, b, c, o = r(16, n), r(16, n), r(16, n), r(16, n)
    for x in (a, b, c, o):
        x[3 * q:] = r(10, n - 3 * q)
    d = np.empty_like(o)
    d[:q] = r(16, q) - o[:q]
    e = rng.integers(0, 3, q)                                   # which edge
    p0 = np.where((e == 2)[:, None], b[q:2 * q], a[q:2 * q])    # AB, AC, BC
    p1 = np.where((e == 0)[:, None], b[q:2 * q], c[q:2 * q])
    d[q:2 * q] = p0 + p1 - 2 * o[q:2 * q]
    w = rng.integers(0, 3, q)
    vtx = np.where((w == 0)[:, None], a[2 * q:3 * q], np.where((w == 1)[:, None], b[2 * q:3 * q], c[2 * q:3 * q]))
    d[2 * q:3 * q] = vtx - o[2 * q:3 * q]
    d[3 * q:] = a[3 * q:] + b[3 * q:] + c[3 * q:] - 3 * o[3 * q:]
    assert np.abs(d).max() <= 64
    tmin = np.array([0.0, 0.5, 1.0], np.float32)[np.arange(n) % 3]
    return o, d, a, b - a, c - a, tmin


def mt_general_table(n=4096, seed=8):
    """Random float rays and triangles, then records holding inf, NaN, a
    denormal and 1e30 in every position in turn.  float32 arrays."""
    rng = np.random.default_rng(seed)
    m = n - 4 * 16
    rec = rng.normal(0.0, 1.0, (n, 16)).astype(np.float32) * np.float32(4.0)
    rec[: m // 2] = np.round(rec[: m // 2] * 4) / 4        # dyadic: many exact zeros of det, u, v
    rec[:, 15] = np.abs(rec[:, 15]) * np.float32(0.1)
    k = m
    for val in (np.inf, np.nan, 1e-40, 1e30):
        for pos in range(16):
            rec[k, pos] = np.float32(val)
            k += 1
    return rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12], rec[:, 12:15], rec[:, 15]


# ---- tables: slab ------------------------------------------------------------
def slab_table(n=4096, seed=9):
    """-> o, d, planes float32[n, 6], tmin, tmax, exact bool[n]: the exact rows
    (power-of-two directions, quarter-integer origins and planes) first, then
    general rows: random boxes and rays, with zero, tiny and axis-parallel
    direction components, origins on a face, planes that overflow binary16."""
    rng = np.random.default_rng(seed)
    ne = n // 2
    o = np.zeros((n, 3), np.float32); d = np.zeros((n, 3), np.float32)
    pl = np.zeros((n, 6), np.float32)
    o[:ne] = rng.integers(-64, 65, (ne, 3)) / 4.0
    d[:ne] = np.ldexp(rng.choice([-1.0, 1.0], (ne, 3)), rng.integers(-3, 4, (ne, 3)))
    c = rng.integers(-64, 65, (ne, 3)) / 4.0
    h = rng.integers(0, 33, (ne, 3)) / 4.0
    pl[:ne, 0::2], pl[:ne, 1::2] = c - h, c + h
    g = n - ne
    o[ne:] = rng.uniform(-20, 20, (g, 3))
    d[ne:] = rng.normal(0, 1, (g, 3))
    c = rng.uniform(-20, 20, (g, 3)); h = rng.uniform(0, 8, (g, 3))
    pl[ne:, 0::2], pl[ne:, 1::2] = c - h, c + h
    i = np.arange(ne, n)
    ax = rng.integers(0, 3, g)
    z1 = i[(i % 8) == 0]; d[z1, ax[z1 - ne]] = 0.0                      # one zero component
    z2 = i[(i % 8) == 1]                                                # two zero components
    keep = d[z2, ax[z2 - ne]].copy(); d[z2] = 0.0; d[z2, ax[z2 - ne]] = keep
    tiny = i[(i % 8) == 2]; d[tiny, ax[tiny - ne]] = 1e-30              # below safe_dir's bound
    face = i[(i % 8) == 3]; o[face, ax[face - ne]] = pl[face, 2 * ax[face - ne]]  # origin on a lo face
    aim = i[(i % 8) >= 4]                                               # aimed at a point of the box
    tgt = (pl[aim, 0::2] + (pl[aim, 1::2] - pl[aim, 0::2]) * rng.uniform(0, 1, (aim.size, 3))).astype(np.float32)
    nz = d[aim] != 0
    d[aim] = np.where(nz, tgt - o[aim], 0.0)
    big = i[(i % 16) == 7]; pl[big] *= np.float32(8192.0); o[big] *= np.float32(8192.0); d[big] *= np.float32(8192.0)
    tmin = np.where(rng.random(n) < 0.5, 0.0, rng.integers(0, 9, n) / 4.0).astype(np.float32)
    tmax = np.where(rng.random(n) < 0.5, np.inf, tmin + rng.integers(0, 17, n) / 4.0).astype(np.float32)
    exact = np.arange(n) < ne
    return o, d, pl, tmin, tmax, exact


def half_planes_outward(pl):
    """binary16 bits of fp32 planes rounded outward (lo down, hi up; past
    65504: -inf / +inf), as lo | hi << 16 per axis -> (uint32[n, 3], the
    planes these decode to float32[n, 6])"""
    pl = np.asarray(pl, np.float32)
    with np.errstate(over="ignore"):
        h = pl.astype(np.float16)
    back = h.astype(np.float32)
    lo_bad = back[:, 0::2] > pl[:, 0::2]
    hi_bad = back[:, 1::2] < pl[:, 1::2]
    with np.errstate(over="ignore"):
        h[:, 0::2] = np.where(lo_bad, np.nextafter(h[:, 0::2], np.float16(-np.inf)), h[:, 0::2])
        h[:, 1::2] = np.where(hi_bad, np.nextafter(h[:, 1::2], np.float16(np.inf)), h[:, 1::2])
    bits = h.view(np.uint16).astype(np.uint32)
    return bits[:, 0::2] | (bits[:, 1::2] << 16), h.astype(np.float32)


# ---- tables: PCG and the sampler ------------------------------------------------
def pcg_inputs(n=4096, seed=10):
    edge = []
    for v in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        edge += [(v - 1) & rr.M32, v, (v + 1) & rr.M32]
    rng = np.random.default_rng(seed)
    rest = rng.integers(0, 2 ** 32, n - len(edge), dtype=np.uint64)
    return np.concatenate([np.array(edge, np.uint64), rest]).astype(np.uint32)


def pt_key_inputs():
    seeds = [0, 1, 2, 0x5EED, 0xFFFFFFFE, 0xFFFFFFFF]
    pxs = [0, 1, 2 ** 24 - 1]
    return np.array([(s, p, v) for s in seeds for p in pxs for v in range(5)], np.uint32)


_KEY_CACHE = {}


def bounce_keys():
    """-> (fall-back keys: every key below 2^24 whose 8 tries the float64 model
    rejects by more than 1e-6; accepted: {k: the first 8 keys accepted first on
    try k by the same margin}).  A vectorised scan of the 2^24 keys (numpy
    uint64), a try's hashes computed only for the keys still undecided."""
    if _KEY_CACHE:
        return _KEY_CACHE["fb"], _KEY_CACHE["acc"]
    m32 = np.uint64(rr.M32)

    def h(v):
        st = (v * np.uint64(747796405) + np.uint64(2891336453)) & m32
        w = (((st >> ((st >> np.uint64(28)) + np.uint64(4))) ^ st) * np.uint64(277803737)) & m32
        return ((w >> np.uint64(22)) ^ w) & m32

    def u11(x):
        return (x >> np.uint64(8)).astype(np.float64) / 8388608.0 - 1.0
    key = np.arange(1 << 24, dtype=np.uint64)   # the keys whose tries so far were all rejected
    acc = {}
    for i in range(rr.PT_TRIES):
        a = u11(h((key + np.uint64(2 * i)) & m32))
        b = u11(h((key + np.uint64(2 * i + 1)) & m32))
        r2 = a * a + b * b
        acc[i + 1] = key[r2 < 1.0 - 1e-6][:8].astype(np.uint32)
        key = key[r2 > 1.0 + 1e-6]
    fb = key.astype(np.uint32)
    # the scalar model agrees with the vectorised scan
    assert all(rr.disk_class(int(k)) == 0 for k in fb[:8])
    assert all(rr.disk_class(int(k)) == t for t, ks in acc.items() for k in ks[:2])
    _KEY_CACHE["fb"], _KEY_CACHE["acc"] = fb, acc
    return fb, acc


def bounce_table():
    """4096 (normal, key) records: normal r % 64 of bounce_normals() with key
    r % len(keys) of the key list -- every fall-back key, then 8 keys accepted
    first on each try 1 .. 8 (an odd count, so the pairs do not repeat)
    -> (normals float32[4096, 3], keys uint32[4096], class int[4096]: 0
    fall-back, k accepted on try k)"""
    fb, acc = bounce_keys()
    keys = np.concatenate([fb] + [acc[k] for k in range(1, rr.PT_TRIES + 1)])
    cls = np.concatenate([np.zeros(len(fb), int)] + [np.full(len(acc[k]), k) for k in range(1, rr.PT_TRIES + 1)])
    if len(keys) % 2 == 0:
        keys, cls = np.append(keys, acc[1][0]), np.append(cls, 1)
    r = np.arange(4096)
    return bounce_normals()[r % 64], keys[r % len(keys)].astype(np.uint32), cls[r % len(keys)]


def bounce_normals(seed=11):
    rng = np.random.default_rng(seed)
    fixed = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0.0, 0.0, -0.0)]
    zc = -1.0 + 2.0 ** -24
    for z in (zc, 2.0 ** -20, -(2.0 ** -20)):
        s = np.sqrt(1.0 - z * z)
        fixed.append((s * 0.6, s * 0.8, z))
    v = rng.normal(0, 1, (64 - len(fixed), 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return np.concatenate([np.array(fixed, np.float64), v]).astype(np.float32)


# ---- walk scenes -------------------------------------------------------------
def _soup(seed=21):
    """64 lattice triangles in [-16, 16]^3: pids 60, 61 coplanar with and
    overlapping pids 3, 4 (the same corner, both edges doubled), pids 62, 63
    exact duplicates of pids 5 and 9"""
    rng = np.random.default_rng(seed)
    tri = np.zeros((64, 3, 3), np.int64)
    k = 0
    while k < 60:
        lim = 8 if k in (3, 4) else 16
        a = rng.integers(-lim, lim + 1, 3)
        e1, e2 = rng.integers(-8, 9, 3), rng.integers(-8, 9, 3)
        if not np.any(np.cross(e1, e2)) or np.abs(a + 2 * e1).max() > 16 or np.abs(a + 2 * e2).max() > 16:
            continue
        tri[k] = (a, a + e1, a + e2)
        k += 1
    for dst, src in ((60, 3), (61, 4)):
        a, b, c = tri[src]
        tri[dst] = (a, a + 2 * (b - a), a + 2 * (c - a))
    tri[62], tri[63] = tri[5], tri[9]
    return tri


def _quads():
    """axis-aligned quads (two triangles each) in planes x = c, y = c, w = c:
    every triangle's box is flat before the builders pad it"""
    tri = []
    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for c, (u0, v0, s) in zip((-12, -3, 5, 14), ((-14, -10, 9), (-6, -8, 14), (0, -2, 7), (-16, -16, 32))):
            p = np.zeros((4, 3), np.int64)
            p[:, axis] = c
            p[:, u] = (u0, u0 + s, u0 + s, u0)
            p[:, v] = (v0, v0, v0 + s, v0 + s)
            tri += [(p[0], p[1], p[2]), (p[0], p[2], p[3])]
    return np.array(tri, np.int64)


def _fan():
    """32 triangles round the vertex (0, 0, 4), their far edges the 32 lattice
    points on the rim of the square [-4, 4]^2 at w = -4"""
    rim = [(x, -4) for x in range(-4, 4)] + [(4, y) for y in range(-4, 4)] + \
          [(x, 4) for x in range(4, -4, -1)] + [(-4, y) for y in range(4, -4, -1)]
    apex = (0, 0, 4)
    return np.array([(apex, (*rim[i], -4), (*rim[(i + 1) % 32], -4)) for i in range(32)], np.int64)


LATTICE_SCENES = {"soup": (_soup, 0), "quads": (_quads, 0), "fan": (_fan, 0),
                  "soup_big": (_soup, 12), "soup_small": (_soup, -12)}


def lattice_scene(name):
    """-> (integer corners int64[T, 3, 3], the power of two that scales them)"""
    f, e = LATTICE_SCENES[name]
    return f(), e


def write_scene(path, corners_f):
    """corners float[T, 3, 3] clip (x, y, w) -> a trace through synth_scene._write"""
    import synth_scene
    c = np.asarray(corners_f, np.float64)
    verts = [(c[:, k, 0], c[:, k, 1], np.zeros(len(c)), c[:, k, 2]) for k in range(3)]
    return synth_scene._write(path, verts, np.full((len(c), 3), 0.5))


def tri9_of(corners_f32):
    """float32 corners [T, 3, 3] -> the v0, e1, e2 records by pid (float32[T, 9])"""
    c = np.asarray(corners_f32, np.float32)
    return np.concatenate([c[:, 0], c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]], 1).astype(np.float32)


# ---- walk rays ------------------------------------------------------------------
N_RAYS = 4096
PATTERNS = ("all", "odd_off", "lane63", "pair_half")


def activity(pattern, n=N_RAYS):
    lane = np.arange(n) % 64
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "odd_off":
        return (lane & 1) == 0
    if pattern == "lane63":
        return lane == 63
    if pattern == "pair_half":          # pair p = lanes 2p, 2p + 1: lane 2p + (p & 1) off
        return lane != ((lane & ~1) | ((lane >> 1) & 1))
    raise ValueError(pattern)


def lattice_rays(tri, seed=31):
    """4096 integer rays for a lattice scene of extent 16 (tri int64[T, 3, 3]):
    -> o, d int64[n, 3], tmin float32[n], skip int32[n], tie_high bool[n], and
    `kind` int[n]; tmax and the skip of the winners are filled by finish_rays.
    The kinds are shuffled, so a wave's 64 rays are unrelated."""
    rng = np.random.default_rng(seed)
    T = len(tri)
    n = N_RAYS
    o = rng.integers(-16, 17, (n, 3))
    d = np.zeros((n, 3), np.int64)
    kind = np.repeat(np.arange(8), n // 8)
    t = rng.integers(0, T, n)
    a, b, c = tri[t, 0], tri[t, 1], tri[t, 2]
    w = rng.integers(0, 3, n)
    vtx = np.where((w == 0)[:, None], a, np.where((w == 1)[:, None], b, c))
    nxt = np.where((w == 0)[:, None], b, np.where((w == 1)[:, None], c, a))
    k = kind == 0                                   # lattice point to lattice point
    d[k] = rng.integers(-16, 17, (k.sum(), 3)) - o[k]
    k = kind == 1                                   # at a vertex (t = 1) / an edge midpoint (t = 1/2)
    d[k] = np.where((rng.random(k.sum()) < 0.5)[:, None], vtx[k] - o[k], vtx[k] + nxt[k] - 2 * o[k])
    k = kind == 2                                   # axis-parallel, one zero component, through a vertex
    d[k] = vtx[k] - o[k]
    ax = rng.integers(0, 3, n)
    idx = np.flatnonzero(k)
    o[idx, ax[idx]] = vtx[idx, ax[idx]]
    d[idx, ax[idx]] = 0
    k = kind == 3                                   # two zero components: along an axis through a point
    idx = np.flatnonzero(k)
    pt = np.where((rng.random(idx.size) < 0.5)[:, None], vtx[idx], (a[idx] + b[idx] + c[idx]) // 3)
    o[idx] = pt
    step = rng.choice([-8, -3, 2, 24], idx.size)
    o[idx, ax[idx]] -= step
    d[idx] = 0
    d[idx, ax[idx]] = np.sign(step) * rng.choice([1, 2, 16], idx.size)
    k = kind == 4                                   # starts on a vertex / runs inside a triangle's plane
    idx = np.flatnonzero(k)
    half = rng.random(idx.size) < 0.5
    o[idx] = vtx[idx]
    d[idx] = rng.integers(-16, 17, (idx.size, 3))
    inpl = idx[~half]
    i, j = rng.integers(-2, 3, inpl.size), rng.integers(-2, 3, inpl.size)
    o[inpl] = a[inpl] - (b[inpl] - a[inpl]) * i[:, None]
    d[inpl] = (b[inpl] - a[inpl]) * rng.integers(-1, 3, inpl.size)[:, None] + (c[inpl] - a[inpl]) * j[:, None]
    k = kind == 5                                   # far origins: back along the ray by 8 d
    d[k] = vtx[k] - o[k]
    o[k] = o[k] - 8 * d[k]
    k = kind >= 6                                   # tmax / skip at the winner (finish_rays)
    d[k] = np.where((rng.random(k.sum()) < 0.5)[:, None], vtx[k] - o[k], rng.integers(-16, 17, (k.sum(), 3)) - o[k])
    z = ~d.any(1)
    d[z] = (1, 2, 3)
    assert np.abs(o).max() <= 128 * 16
    tmin = np.where(rng.random(n) < 0.7, 0.0, rng.choice([0.5, 1.0], n)).astype(np.float32)
    tie = rng.random(n) < 0.5
    p = rng.permutation(n)
    return o[p], d[p], tmin[p], tie[p], kind[p]


def finish_rays(kind, tmin, win_pid, win_t, seed=32):
    """tmax and skip from the winners of the unbounded rays (win_pid, win_t:
    the closest hits with tmax = inf, skip = -1): kind 6 rays get tmax at the
    winner's t, one float below and one above it; kind 7 rays skip the winner;
    a quarter of the others get a finite random tmax."""
    rng = np.random.default_rng(seed)
    n = len(kind)
    tmax = np.full(n, np.inf, np.float32)
    skip = np.full(n, -1, np.int32)
    r = rng.random(n)
    fin = (kind < 6) & (r < 0.25)
    tmax[fin] = rng.choice([0.5, 1.0, 2.0, 8.0], fin.sum())
    k6 = np.flatnonzero((kind == 6) & (win_pid >= 0))
    t = win_t[k6].astype(np.float32)
    which = np.arange(k6.size) % 3
    tmax[k6] = np.where(which == 0, t, np.where(which == 1, np.nextafter(t, np.float32(-np.inf)),
                                                 np.nextafter(t, np.float32(np.inf))))
    k7 = (kind == 7) & (win_pid >= 0)
    skip[k7] = win_pid[k7]
    return tmax, skip


def pack_rays(o, d, tmin, tmax):
    """float32 [n, 8] rows for orc_trace_rays"""
    return np.concatenate([np.asarray(o, np.float32), np.asarray(d, np.float32),
                           np.asarray(tmin, np.float32)[:, None], np.asarray(tmax, np.float32)[:, None]], 1)


CHAIN_N = 140   # synth_scene.make_chain_scene: the host tree's BVH4 stack need is then 32


def chain_rays(corners, seed=33):
    """4096 float rays for the chain scene (corners float32[T, 3, 3]): from the
    eye and from points in front of a triangle towards its corners, edge
    midpoints and centroid, rays along the chain, rays from far behind.  No
    model answers these: the walks are compared with brute force."""
    rng = np.random.default_rng(seed)
    n, T = N_RAYS, len(corners)
    c = np.asarray(corners, np.float64)
    t = rng.integers(0, min(T, 48), n)          # the triangles float32 still resolves
    w = rng.random((n, 3))
    w /= w.sum(1)[:, None]
    kind = np.repeat(np.arange(8), n // 8)
    w[kind == 1] = np.eye(3)[rng.integers(0, 3, (kind == 1).sum())]               # a corner
    m = kind == 2
    w[m] = (np.eye(3)[rng.integers(0, 3, m.sum())] + np.eye(3)[rng.integers(0, 3, m.sum())]) / 2  # an edge midpoint
    tgt = (c[t] * w[:, :, None]).sum(1)
    o = np.zeros((n, 3))
    m = kind >= 3
    o[m] = tgt[m] + rng.normal(0, 1, (m.sum(), 3)) * (0.5, 0.5, 30.0)
    d = tgt - o
    m = kind == 5                                # along the chain, inside / next to its plane
    d[m] = (1.0, 0.0, 0.0)
    o[m] = np.stack([-rng.random(m.sum()), rng.random(m.sum()), np.where(rng.random(m.sum()) < 0.5, 100.0, 99.5)], 1)
    d[m, 2] = np.where(o[m, 2] == 100.0, 0.0, rng.random(m.sum()) * 0.5)
    m = kind == 6                                # from far behind the target
    o[m] = o[m] - 64 * d[m]
    z = ~d.any(1)
    d[z] = (0.0, 0.0, 1.0)
    tmin = np.where(rng.random(n) < 0.7, 0.0, 0.5).astype(np.float32)
    tie = rng.random(n) < 0.5
    kind = np.where(kind == 0, 6, np.where(kind == 4, 7, kind))   # finish_rays: tmax / skip at the winner
    p = rng.permutation(n)
    return o[p].astype(np.float32), d[p].astype(np.float32), tmin[p], tie[p], kind[p]


WALK_SCENES = tuple(LATTICE_SCENES) + ("chain",)
_WALK_CACHE = {}


def walk_case(name, tmpdir, po, rt):
    """One walk scene with its trees and ray table (cached per process):
    tri9 float32[T, 9]; trees {"sah": the host builder's, "lbvh": the oracle's
    restatement of the device LBVH} each (nodes, tris, nodes4 with the planes
    rounded to binary16 values, rt_node4h_t records uint8[N4, 64], BVH4 stack
    need); rays float32[n, 8], skip, tie_high; for a lattice scene the integer
    corners and rays (`lat`), else None."""
    if name in _WALK_CACHE:
        return _WALK_CACHE[name]
    import os
    import synth_scene
    path = os.path.join(str(tmpdir), name + ".cgltrace.gz")
    lat = None
    if name == "chain":
        synth_scene.make_chain_scene(path, CHAIN_N)
    else:
        tri, e = lattice_scene(name)
        write_scene(path, np.ldexp(tri.astype(np.float64), e))
    s = rt.Scene.load(path)
    info = s.info()
    corners = np.ascontiguousarray(s.prims()[:, :, [0, 1, 3]], np.float32)
    if name != "chain":
        assert np.array_equal(corners, np.ldexp(tri.astype(np.float64), e).astype(np.float32))
    tri9 = tri9_of(corners)
    T = len(tri9)
    nodes, tris = s.bvh()
    # the leaf records are the triangles by pid, bit for bit
    pid = tris[:, 3].view(np.int32)
    assert sorted(pid.tolist()) == list(range(T))
    rec = np.concatenate([tris[:, 0:3], tris[:, 4:7], tris[:, 8:11]], 1)
    assert np.array_equal(rec.view(np.uint32), tri9[pid].view(np.uint32))
    n4 = s.bvh4()
    r4, h4 = po.half4(n4)
    assert np.array_equal(r4.view(np.uint32), n4.view(np.uint32))   # the host rounded them already
    trees = {"sah": (nodes, tris, n4, h4, info["bvh4_stack"])}
    geom = np.zeros((T, 12), np.float32)
    geom[:, 0:3], geom[:, 4:7], geom[:, 8:11] = tri9[:, 0:3], tri9[:, 3:6], tri9[:, 6:9]
    geom[:, 3] = np.arange(T, dtype=np.int32).view(np.float32)
    ln, lt, depth = po.lbvh_build(corners, geom)
    l4, lstack = po.lbvh_collapse4(ln)
    l4r, lh = po.half4(l4)
    assert depth <= 32 and lstack <= 32 and info["bvh_depth"] <= 32 and info["bvh4_stack"] <= 32
    trees["lbvh"] = (ln, lt, l4r, lh, lstack)
    s.close()
    if name == "chain":
        o, d, tmin, tie, kind = chain_rays(corners)
        free = pack_rays(o, d, tmin, np.full(N_RAYS, np.inf))
        wp, wt, _ = po.trace_rays(tri9, free, np.full(N_RAYS, -1), tie)   # shapes the inputs only
    else:
        oi, di, tmin, tie, kind = lattice_rays(tri)
        o, d = np.ldexp(oi.astype(np.float64), e).astype(np.float32), np.ldexp(di.astype(np.float64), e).astype(np.float32)
        inside, t, boundary = rr.lattice_hits(oi, di, tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        wp, wt, _ = rr.closest_hits(inside, t, tmin, np.full(N_RAYS, np.inf, np.float32), np.full(N_RAYS, -1), tie)
        lat = dict(tri=tri, o=oi, d=di, inside=inside, t=t, boundary=boundary)
    tmax, skip = finish_rays(kind, tmin, wp, wt)
    case = dict(name=name, path=path, tri9=tri9, geom=geom, trees=trees, rays=pack_rays(o, d, tmin, tmax), skip=skip,
                tie=tie, kind=kind, lat=lat, geom_inf=bool(np.isinf(n4[:, :24]).any()),
                half_denormal=bool(((np.abs(n4[:, :24]) < 2.0 ** -14) & (n4[:, :24] != 0)).any()))
    _WALK_CACHE[name] = case
    return case
