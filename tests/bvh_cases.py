"""Inputs for the tree builders' invariants (tests/test_bvh_invariants_cpu.py,
tests/test_gpu_bvh_invariants.py): triangle lists that reach the builders'
boundaries -- each the smallest that does -- and 2 048 rays per list.  Inputs
only: what a tree must satisfy is tests/bvh_reference.py, what a ray hits the
oracle's brute force (and, for the lattice list, the exact model).

A case is float32 clip-space corners [T, 3, 3] written through
ray_known_answers.write_scene, so a pid is the triangle's index.

  rand<n>          uniform centres in +-16, corners +-1 around them.  n = 1 .. 6: a lone root leaf,
                   SAH_LEAF / BVHB_LEAF_MAX 4 | 5; 63 .. 65: SAH_SMALL (a wave's segment | a
                   workgroup's); 255 .. 257: SAH_BLOCK and the LBVH's 256-leaf LDS window;
                   1023 .. 1025: the sort's BVHB_ITEMS block; 2049: three sort blocks, nine windows
  lat1025          integer corners in +-16 (the exact model's domain), non-degenerate
  same<n>          one triangle n times: every Morton code equal (the index alone orders them),
                   every SAH split empty (the median fall-back at every level)
  collinear257     centres on one line: two axes of zero extent (the 16 bins, the codes)
  flatgrid1089     33 x 33 triangles in the plane w = 5: flat boxes, one axis of zero extent
  zeroarea8        4 lattice triangles and 4 collapsed to a point each
  cluster_outlier  1 024 triangles within 2^-8 and one 4 096 times larger: the padding and the
                   code range are set by the one, the tree holds the many
  ladder_b_c_m     depth: c copies of a small triangle at the origin, then m copies in each cell
                   whose 30-bit code is 1 << b for b < bits (axis 2 - b % 3, offset 1 << b // 3),
                   then one at (1023, 1023, 1023) that fixes the code range -- the radix tree
                   peels one cell per level"""
import os

import numpy as np

import bvh_reference as br
import ray_known_answers as ka

N_RAYS = 2048
STACK_DEEP = 32                  # RT_STACK_DEEP (kernels/rt_common.h): the deep images' traversal stack

RAND = (1, 2, 3, 4, 5, 6, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
SAME = (1, 2, 4, 5, 64, 65, 300, 1025)
LADDER_STACK32 = (20, 8, 8)      # the LBVH's BVH4 stack need is exactly 32: the deep images' bound
LADDER_STACK_OVER = (21, 8, 8)   # LBVH depth <= 32, stack need > 32: the BVH2 is traversed
LADDER_LBVH_DEEP = (30, 32, 1)   # LBVH depth 33: refused
LADDER_SAH_STACK = (30, 2048, 1) # the SAH tree's stack need is 33: the BVH2 is traversed
LADDERS = ((24, 64, 1), (30, 8, 1), LADDER_STACK32, LADDER_LBVH_DEEP, LADDER_SAH_STACK, LADDER_STACK_OVER)

# what each depth case exists for, from the CPU side (the host builder's info() and the oracle's
# LBVH): (host depth, host stack4, LBVH depth, LBVH stack4)
LADDER_FACTS = {(24, 64, 1): (11, 15, 29, 30), (30, 8, 1): (8, 8, 31, 31), (20, 8, 8): (8, 10, 22, 32),
                (30, 32, 1): (10, 12, 33, 34), (30, 2048, 1): (16, 33, 39, 43)}


def ladder_name(spec):
    return "ladder_%d_%d_%d" % spec


NAMES = tuple(f"rand{n}" for n in RAND) + ("lat1025",) + tuple(f"same{n}" for n in SAME) + \
    ("collinear257", "flatgrid1089", "zeroarea8", "cluster_outlier") + tuple(ladder_name(s) for s in LADDERS)
# the cases both device builders take within every limit (depth and BVH4 stack need <= 32)
BEYOND = tuple(ladder_name(s) for s in (LADDER_STACK_OVER, LADDER_LBVH_DEEP, LADDER_SAH_STACK))
WITHIN = tuple(n for n in NAMES if n not in BEYOND)


def _rand(n):
    rng = np.random.default_rng(4000 + n)
    cen = rng.uniform(-16, 16, (n, 1, 3))
    return (cen + rng.uniform(-1, 1, (n, 3, 3))).astype(np.float32)


def _lattice(n, seed=41):
    """integer triangles in [-16, 16]^3 with edges of up to 8, none of zero area (as
    ray_known_answers._soup draws them)"""
    rng = np.random.default_rng(seed)
    tri = np.zeros((n, 3, 3), np.int64)
    k = 0
    while k < n:
        a = rng.integers(-16, 17, 3)
        e1, e2 = rng.integers(-8, 9, 3), rng.integers(-8, 9, 3)
        if not np.any(np.cross(e1, e2)) or np.abs(a + e1).max() > 16 or np.abs(a + e2).max() > 16:
            continue
        tri[k] = (a, a + e1, a + e2)
        k += 1
    return tri


_ONE = np.array([[1.0, 2.0, 3.0], [4.0, 2.5, 3.5], [2.0, 5.0, 4.0]], np.float32)
# box centre = the triangle's position on every axis: corners at -h / +h on each
_CELL = np.array([[-1, -1, -1], [1, -1, 1], [-1, 1, 1]], np.float32) * np.float32(0.125)


def _ladder(bits, c, m):
    pos = [np.zeros(3)] * c
    for b in range(bits):
        p = np.zeros(3)
        p[2 - b % 3] = 1 << (b // 3)
        pos += [p] * m
    pos.append(np.full(3, 1023.0))
    return (np.array(pos)[:, None, :] + _CELL[None]).astype(np.float32)


_VIEWS = {}


def corners_of(name):
    if name in _VIEWS:
        return _VIEWS[name]
    if name.startswith("rand"):
        return _rand(int(name[4:]))
    if name.startswith("same"):
        return np.repeat(_ONE[None], int(name[4:]), 0)
    if name.startswith("ladder_"):
        return _ladder(*(int(x) for x in name.split("_")[1:]))
    if name == "lat1025":
        return _lattice(1025).astype(np.float32)
    if name == "collinear257":
        return (_ONE[None] + np.arange(257)[:, None, None] * np.array([0.37, 0.0, 0.0])).astype(np.float32)
    if name == "flatgrid1089":
        i, j = np.meshgrid(np.arange(33.0) - 16.0, np.arange(33.0) - 16.0, indexing="ij")
        o = np.stack([i.ravel(), j.ravel(), np.full(1089, 5.0)], 1)
        return (o[:, None, :] + np.array([[0, 0, 0], [0.8, 0, 0], [0, 0.8, 0]])[None]).astype(np.float32)
    if name == "zeroarea8":
        tri = _lattice(8, seed=43)
        tri[4:, 1], tri[4:, 2] = tri[4:, 0], tri[4:, 0]
        return tri.astype(np.float32)
    if name == "cluster_outlier":
        rng = np.random.default_rng(47)
        cen = rng.uniform(0.0, 2.0 ** -8, (1024, 1, 3))
        small = np.clip(cen + rng.uniform(-(2.0 ** -11), 2.0 ** -11, (1024, 3, 3)), 0.0, 2.0 ** -8)
        big = np.array([[[0.0, 0.0, 0.0], [16.0, 0.0, 16.0], [0.0, 16.0, 16.0]]])
        return np.concatenate([small, big]).astype(np.float32)
    raise KeyError(name)


# the origin box's padding, in units of the scene's largest half-extent, for a case that falls
# short of the N/8 hits or N/16 misses with the default of 0.5 (none does: 431 .. 1 665 hits)
ORIGIN_PAD = {}


def make_rays(corners, seed, pad=0.5):
    """2 048 float32 rays [n, 8] (o, d, tmin, tmax), the kinds shuffled: a quarter each from
    points of the padded scene box to random points of random triangles; to triangle corners;
    to either as segments that end exactly at the target (tmax = 1); in random directions"""
    rng = np.random.default_rng(seed)
    c = np.asarray(corners, np.float64)
    n, T = N_RAYS, len(c)
    lo, hi = c.reshape(-1, 3).min(0), c.reshape(-1, 3).max(0)
    half = (hi - lo) / 2
    r = max(half.max(), 2.0 ** -20)
    o = ((lo + hi) / 2 + rng.uniform(-1, 1, (n, 3)) * (half + pad * r)).astype(np.float32)
    kind = np.repeat(np.arange(4), n // 4)
    t = rng.integers(0, T, n)
    w = rng.random((n, 3))
    w /= w.sum(1)[:, None]
    corner = (kind == 1) | ((kind == 2) & (rng.random(n) < 0.5))
    w[corner] = np.eye(3)[rng.integers(0, 3, corner.sum())]
    tgt = (c[t] * w[:, :, None]).sum(1).astype(np.float32)
    d = (tgt - o).astype(np.float32)
    k3 = kind == 3
    d[k3] = (rng.normal(0, 1, (k3.sum(), 3)) * r).astype(np.float32)
    d[~d.any(1)] = (0.0, 0.0, 1.0)
    tmax = np.where(kind == 2, 1.0, np.inf).astype(np.float32)
    p = rng.permutation(n)
    return ka.pack_rays(o[p], d[p], np.zeros(n, np.float32), tmax[p])


_CACHE = {}


def case(name, tmpdir, po, rt):
    """One case, cached per process: corners, tri9, its trace's path, the host builder's tree
    and the oracle's LBVH (each nodes, tris, nodes4 with binary16 planes, rt_node4h_t records,
    depth, BVH4 stack need), the rays and the brute-force answers (pid, t, occluded)."""
    if name in _CACHE:
        return _CACHE[name]
    corners = corners_of(name)
    path = os.path.join(str(tmpdir), name + ".cgltrace.gz")
    ka.write_scene(path, corners)
    s = rt.Scene.load(path)
    info = s.info()
    T = len(corners)
    assert info["num_geometry"] == T == info["num_prims"]
    got = np.ascontiguousarray(s.prims()[:, :, [0, 1, 3]], np.float32)
    assert np.array_equal(got.view(np.uint32), corners.view(np.uint32))      # the trace holds the corners exactly
    tri9 = ka.tri9_of(corners)
    geom = br.records_of(corners)
    nodes, tris = s.bvh()
    n4 = s.bvh4()
    r4, h4 = po.half4(n4)
    assert np.array_equal(r4.view(np.uint32), n4.view(np.uint32))            # the host rounded them already
    trees = {"sah": (nodes, tris, n4, h4, info["bvh_depth"], info["bvh4_stack"])}
    ln, lt, ldepth = po.lbvh_build(corners, geom)
    l4, lstack = po.lbvh_collapse4(ln)
    l4r, lh = po.half4(l4)
    trees["lbvh"] = (ln, lt, l4r, lh, ldepth, lstack)
    s.close()
    rays = make_rays(corners, seed=5000 + len(name) * 131 + T, pad=ORIGIN_PAD.get(name, 0.5))
    none = np.full(N_RAYS, -1, np.int32)
    brute = po.trace_rays(tri9, rays, none, np.zeros(N_RAYS, np.uint8))
    c = dict(name=name, path=path, corners=corners, tri9=tri9, geom=geom, info=info, trees=trees, rays=rays,
             brute=brute, none=none)
    _CACHE[name] = c
    return c


def lattice_table(c):
    """lat1025's second ray table: ray_known_answers.lattice_rays over its integer corners,
    answered by the exact rational model -> (rays float32[4096, 8], skip, model pid, model t)"""
    import ray_reference as rr
    if "lat" not in c:
        tri = c["corners"].astype(np.int64)
        n = ka.N_RAYS
        oi, di, tmin, _, kind = ka.lattice_rays(tri)
        inside, t, _ = rr.lattice_hits(oi, di, tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        low = np.zeros(n, bool)
        wp, wt, _ = rr.closest_hits(inside, t, tmin, np.full(n, np.inf, np.float32), np.full(n, -1), low)
        tmax, skip = ka.finish_rays(kind, tmin, wp, wt)
        mp, mt, mo = rr.closest_hits(inside, t, tmin, tmax, skip, low)
        c["lat"] = (ka.pack_rays(oi, di, tmin, tmax), skip, mp, mt, mo)
    return c["lat"]


VIEW_W = 1.0


def in_view(corners, w0=VIEW_W):
    """A copy of a ladder in front of the eye: w + w0.  The offset that would bring every
    triangle's x / w and y / w inside (-1, 1) is above 1023, and there a 0.25-sized triangle
    spans 2^-12 of the view: it covers no pixel centre at 64 x 64 and the frame casts no shadow
    ray.  At w0 = 1 the copies at the origin and the near cells along w are in view (45 pixels
    at 64 x 64), the cells further out along x and y lie outside it and still occlude; the
    offsets are exact in float32, so the codes and the tree's shape are the case's."""
    c = np.asarray(corners, np.float32).copy()
    c[:, :, 2] += np.float32(w0)
    assert (c[:, :, 2] > 0).all()
    return c


def view_case(name, tmpdir, po, rt):
    """the case's in-view copy as a case of its own (name + "_view"): its trace, its trees"""
    key = name + "_view"
    if key not in _CACHE:
        _VIEWS[key] = in_view(corners_of(name))
        case(key, tmpdir, po, rt)
    return _CACHE[key]
