"""What a tree over a triangle list means, in numpy (tests/test_bvh_invariants_cpu.py
holds the host builder and the oracle's LBVH to it, tests/test_gpu_bvh_invariants.py
the two device builders).  Written from the record layouts alone (vx_rt.h,
kernels/rt_common.h: rt_node_t, rt_node4_t, rt_node4h_t, rt_tri_t) and from
bvh_common.h's description of the LBVH's ordering; it shares nothing with
app/bvh.cpp, oracle/lbvh.c or the kernels.

  rt_node_t   float[16]: (c0 lo, c0 hi, c1 lo, c1 hi) of x, of y, of w, then the two
              child references as int32 and two unused words
  reference   >= 0 an internal node; -1 empty; else a leaf: bits 4..30 its first
              record, bits 0..3 its record count - 1
  rt_tri_t    float[12]: v0.xyw, pid (int32), e1.xyw, 0, e2.xyw, 0
  rt_node4_t  float[32]: lo.x[4], hi.x[4], lo.y[4], hi.y[4], lo.w[4], hi.w[4],
              reference[4] (int32), 4 unused words
  rt_node4h_t 64 bytes: the 24 planes as binary16 in the same order, reference[4]

Containment is exact everywhere: lo <= corner <= hi on the float32 input corners,
child box inside the box its parent stores for it, no tolerance."""
import numpy as np

LEAF_MAX = 4


class Invalid(AssertionError):
    """a tree that breaks one of the invariants"""


def _need(cond, *what):
    if not cond:
        raise Invalid(what)


def records_of(corners):
    """float32 corners [T, 3, 3] -> the rt_tri_t records by pid (float32[T, 12]; pid = index)"""
    c = np.asarray(corners, np.float32)
    rec = np.zeros((len(c), 12), np.float32)
    rec[:, 0:3], rec[:, 4:7], rec[:, 8:11] = c[:, 0], c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    rec[:, 3] = np.arange(len(c), dtype=np.int32).view(np.float32)
    return rec


def _leaf(ref):
    u = int(ref) & 0xFFFFFFFF
    return (u >> 4) & 0x7FFFFFF, (u & 15) + 1


def _refs2(node):
    return node[12:14].view(np.int32)


def _box2(node, ch):
    return node[[2 * ch, 4 + 2 * ch, 8 + 2 * ch]], node[[1 + 2 * ch, 5 + 2 * ch, 9 + 2 * ch]]


def _leaf_checks(ref, lo, hi, tris, corners, rec, slot_used, pid_seen, where):
    """one leaf reference under the box (lo, hi): 1..4 records inside the array, no record and
    no pid met before, every record its triangle bit for bit, every corner inside the box"""
    first, count = _leaf(ref)
    _need(1 <= count <= LEAF_MAX, "leaf size", where, count)
    _need(first + count <= len(tris), "leaf past the records", where, first, count)
    for k in range(first, first + count):
        _need(not slot_used[k], "record in two leaves", where, k)
        slot_used[k] = True
        pid = int(tris[k, 3:4].view(np.int32)[0])
        _need(0 <= pid < len(corners), "pid out of range", where, pid)
        _need(not pid_seen[pid], "pid in two records", where, pid)
        pid_seen[pid] = True
        _need(np.array_equal(tris[k].view(np.uint32), rec[pid].view(np.uint32)), "record differs from its triangle", where, pid)
        c = corners[pid]
        _need(bool(np.all(lo <= c) and np.all(c <= hi)), "corner outside its leaf box", where, pid)


def _expected(pids, T):
    want = np.ones(T, bool)
    if pids is not None:
        want[:] = False
        want[np.asarray(pids, np.int64)] = True
    return want


def walk2(nodes, tris, corners, pids=None):
    """the BVH2's invariants -> dict(depth, reached, leaves): internal levels on the deepest
    path (the root is level 1), internal nodes reached, the leaf references in walk order.
    pids: the triangles the tree is over (None: every one of `corners`)"""
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 16)
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 12)
    corners = np.ascontiguousarray(corners, np.float32)
    T = len(corners)
    rec = records_of(corners)
    _need(len(nodes) >= 1 and T >= 1, "empty tree")
    want = _expected(pids, T)
    _need(len(tris) == want.sum(), "record count", len(tris), int(want.sum()))
    seen = np.zeros(len(nodes), bool)
    slot_used, pid_seen = np.zeros(len(tris), bool), np.zeros(T, bool)
    leaves, depth = [], 0
    todo = [(0, None, None, 1)]
    while todo:
        i, plo, phi, d = todo.pop()
        _need(0 <= i < len(nodes), "node reference out of range", i)
        _need(not seen[i], "node reached twice", i)
        seen[i] = True
        depth = max(depth, d)
        refs = _refs2(nodes[i])
        _need(refs[0] != -1, "empty first child", i)
        _need(refs[1] != -1 or (i == 0 and refs[0] < 0), "empty child below the root", i)
        for ch in (1, 0):
            ref = int(refs[ch])
            if ref == -1:
                continue
            lo, hi = _box2(nodes[i], ch)
            _need(bool(np.all(lo <= hi)), "lo > hi", i, ch)
            if plo is not None:
                _need(bool(np.all(plo <= lo) and np.all(hi <= phi)), "child box outside its parent's", i, ch)
            if ref >= 0:
                todo.append((ref, lo, hi, d + 1))
            else:
                leaves.append(ref)
                _leaf_checks(ref, lo, hi, tris, corners, rec, slot_used, pid_seen, (i, ch))
    _need(np.array_equal(pid_seen, want), "triangle in no leaf, or one the tree is not over",
          np.flatnonzero(pid_seen != want)[:4].tolist())
    _need(bool(slot_used.all()), "record in no leaf", np.flatnonzero(~slot_used)[:4].tolist())
    return dict(depth=depth, reached=int(seen.sum()), leaves=leaves)


def check_bvh2(nodes, tris, corners, pids=None):
    """every pid in exactly one leaf slot, leaves of 1..4, records == the input triangles, exact
    containment of corners and of child boxes, lo <= hi, no reference past the arrays, no node
    reached twice -> the depth"""
    return walk2(nodes, tris, corners, pids)["depth"]


def decode4h(half):
    """rt_node4h_t records uint8[N, 64] -> (planes float32[N, 24], references int32[N, 4])"""
    h = np.ascontiguousarray(half, np.uint8).reshape(-1, 64)
    return h[:, :48].copy().view(np.float16).astype(np.float32), h[:, 48:].copy().view(np.int32)


def is_binary16(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        return x.astype(np.float16).astype(np.float32).view(np.uint32) == x.view(np.uint32)


def check_bvh4(nodes4, nodes, tris, corners, half=None, f16=True, pids=None):
    """the BVH4's invariants: the same exact containment straight against the corners, used
    slots first, >= 2 children but for a lone root, the leaf set the BVH2's; with f16 every
    plane a binary16 value; `half` (rt_node4h_t, uint8[N4, 64]) decodes to the fp32 records
    -> (depth: BVH4 levels on the deepest path, the worst root-to-leaf sum of slots - 1)"""
    nodes4 = np.ascontiguousarray(nodes4, np.float32).reshape(-1, 32)
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1, 12)
    corners = np.ascontiguousarray(corners, np.float32)
    rec = records_of(corners)
    _need(len(nodes4) >= 1, "empty BVH4")
    if half is not None:
        planes, refs = decode4h(half)
        _need(len(planes) == len(nodes4), "half record count", len(planes), len(nodes4))
        _need(np.array_equal(planes.view(np.uint32), nodes4[:, :24].view(np.uint32)), "half planes differ")
        _need(np.array_equal(refs, nodes4[:, 24:28].view(np.int32)), "half references differ")
    seen = np.zeros(len(nodes4), bool)
    slot_used, pid_seen = np.zeros(len(tris), bool), np.zeros(len(corners), bool)
    leaves, depth, stack = [], 0, 0
    todo = [(0, None, None, 1, 0)]
    while todo:
        i, plo, phi, d, acc = todo.pop()
        _need(0 <= i < len(nodes4), "node reference out of range", i)
        _need(not seen[i], "node reached twice", i)
        seen[i] = True
        n = nodes4[i]
        refs = n[24:28].view(np.int32)
        k = int((refs != -1).sum())
        _need(bool((refs[:k] != -1).all()), "used slots not first", i)
        _need(k >= 2 or (i == 0 and k == 1), "fewer than 2 children", i, k)
        depth, stack = max(depth, d), max(stack, acc + k - 1)
        if f16:
            used = np.concatenate([np.arange(k) + 4 * g for g in range(6)])
            _need(bool(is_binary16(n[used]).all()), "plane is no binary16 value", i)
        for q in range(k):
            lo, hi = n[[q, 8 + q, 16 + q]], n[[4 + q, 12 + q, 20 + q]]
            _need(bool(np.all(lo <= hi)), "lo > hi", i, q)
            if plo is not None:
                _need(bool(np.all(plo <= lo) and np.all(hi <= phi)), "child box outside its parent's", i, q)
            ref = int(refs[q])
            if ref >= 0:
                todo.append((ref, lo, hi, d + 1, acc + k - 1))
            else:
                leaves.append(ref)
                _leaf_checks(ref, lo, hi, tris, corners, rec, slot_used, pid_seen, (i, q))
    _need(np.array_equal(pid_seen, _expected(pids, len(corners))) and bool(slot_used.all()), "triangle in no BVH4 leaf")
    leaves2 = walk2(nodes, tris, corners, pids)["leaves"]
    _need(sorted(leaves) == sorted(leaves2), "BVH4 leaf set differs from the BVH2's")
    return depth, stack


# ---- the LBVH's ordering rule ----------------------------------------------------
def morton_codes(corners):
    """30-bit codes of the box centres: per axis 10 bits over the centre bounds (clamped at
    1023, zero extent -> 0), x the highest bit of each triple; all arithmetic float32"""
    c = np.ascontiguousarray(corners, np.float32)
    half = np.float32(0.5)
    cen = ((c.min(1) + c.max(1)) * half).astype(np.float32)
    lo, hi = cen.min(0), cen.max(0)
    ext = (hi - lo).astype(np.float32)
    code = np.zeros(len(c), np.uint32)
    for axis in range(3):
        if ext[axis] > 0:
            t = ((cen[:, axis] - lo[axis]).astype(np.float32) / ext[axis]).astype(np.float32)
        else:
            t = np.zeros(len(c), np.float32)
        q = np.minimum((t * np.float32(1024.0)).astype(np.float32).astype(np.int64), 1023).astype(np.uint32)
        for bit in range(10):
            code |= ((q >> np.uint32(bit)) & np.uint32(1)) << np.uint32(3 * bit + 2 - axis)
    return code


def morton_order(corners):
    """the pids in the LBVH's leaf order: a stable sort by code (equal codes keep index order)"""
    return np.argsort(morton_codes(corners), kind="stable").astype(np.int32)


# ---- a plain builder: a quality yardstick and the validator's own test trees ------------
def pad_of(corners):
    """the builders' box padding: 2^-16 of the largest |coordinate|, at least 1e-6 (float32)"""
    ext = np.float32(np.abs(np.asarray(corners, np.float32)).max())
    return max(np.float32(ext * np.float32(1.0 / 65536.0)), np.float32(1e-6))


def range_tree(corners, order=None, pad=None):
    """order None: the object-median tree -- every range sorted (stably) by box centre along
    the longest axis of its centre bounds and halved, ranges of <= 4 leaves.  order given:
    that leaf order kept, every range halved.  Boxes padded by `pad` (None: pad_of)
    -> (nodes float32[N, 16], root first; tris float32[T, 12] in leaf order)"""
    c = np.ascontiguousarray(corners, np.float32)
    T = len(c)
    pad = pad_of(c) if pad is None else np.float32(pad)
    blo, bhi = c.min(1), c.max(1)
    cen = ((blo + bhi) * np.float32(0.5)).astype(np.float32)
    idx = np.arange(T) if order is None else np.asarray(order).copy()
    nodes, out = [], []
    rec = records_of(c)

    def box(b, e):
        return blo[idx[b:e]].min(0) - pad, bhi[idx[b:e]].max(0) + pad

    def leaf(b, e):
        first = len(out)
        out.extend(idx[b:e].tolist())
        return np.int64(0x80000000 | (first << 4) | (e - b - 1)).astype(np.int32)

    def put(node, ch, lo, hi, ref):
        nodes[node][[2 * ch, 4 + 2 * ch, 8 + 2 * ch]] = lo
        nodes[node][[1 + 2 * ch, 5 + 2 * ch, 9 + 2 * ch]] = hi
        nodes[node][12 + ch:13 + ch] = np.array([ref], np.int32).view(np.float32)

    nodes.append(np.zeros(16, np.float32))
    if T <= LEAF_MAX:
        put(0, 0, *box(0, T), leaf(0, T))
        put(0, 1, np.zeros(3, np.float32), np.zeros(3, np.float32), -1)
        return np.array(nodes, np.float32), rec[out]
    todo = [(0, 0, T)]
    while todo:
        node, b, e = todo.pop()
        if order is None:
            cc = cen[idx[b:e]]
            axis = int(np.argmax(cc.max(0) - cc.min(0)))
            idx[b:e] = idx[b:e][np.argsort(cc[:, axis], kind="stable")]
        mid = (b + e) // 2
        later = []
        for ch, (cb, ce) in enumerate(((b, mid), (mid, e))):
            if ce - cb <= LEAF_MAX:
                later.append((ch, cb, ce, None))
            else:
                nodes.append(np.zeros(16, np.float32))
                later.append((ch, cb, ce, len(nodes) - 1))
        for ch, cb, ce, child in later:
            if child is None:
                put(node, ch, *box(cb, ce), leaf(cb, ce))
            else:
                put(node, ch, *box(cb, ce), child)
        for ch, cb, ce, child in reversed(later):
            if child is not None:
                todo.append((child, cb, ce))
    return np.array(nodes, np.float32), rec[out]


def median_tree(corners):
    """the object-median tree on the longest axis, leaves of at most 4"""
    return range_tree(corners)


def sah_cost(nodes):
    """the surface-area cost of a BVH2: 1 for the root, and for every stored child box its
    area over the root's (the union of the root's two boxes), times 1 for an internal node
    and times the triangle count for a leaf; float64"""
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 16)

    def area(lo, hi):
        d = hi.astype(np.float64) - lo.astype(np.float64)
        return 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0])

    refs0 = _refs2(nodes[0])
    boxes = [_box2(nodes[0], ch) for ch in range(2) if refs0[ch] != -1]
    root = area(np.min([b[0] for b in boxes], 0), np.max([b[1] for b in boxes], 0))
    cost, todo = 1.0, [0]
    while todo:
        i = todo.pop()
        refs = _refs2(nodes[i])
        for ch in range(2):
            ref = int(refs[ch])
            if ref == -1:
                continue
            a = area(*_box2(nodes[i], ch)) / root
            if ref >= 0:
                cost += a
                todo.append(ref)
            else:
                cost += a * _leaf(ref)[1]
    return cost


def half_outward(planes, upper):
    """fp32 planes rounded outward to binary16 values (upper: bool mask of the hi planes)"""
    p = np.asarray(planes, np.float32)
    with np.errstate(over="ignore"):
        h = p.astype(np.float16)
        back = h.astype(np.float32)
        h = np.where(~upper & (back > p), np.nextafter(h, np.float16(-np.inf)), h)
        h = np.where(upper & (back < p), np.nextafter(h, np.float16(np.inf)), h)
    return h.astype(np.float16)


def collapse4(nodes):
    """a BVH4 of a BVH2: every node at an even level takes its children's children (a leaf
    child stays), nodes in walk order; planes rounded outward to binary16
    -> (nodes4 float32[N4, 32], rt_node4h_t records uint8[N4, 64], depth, stack need)"""
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 16)
    out, depth, stack = [], 0, 0
    todo = [(0, -1, 0, 1, 0)]                     # BVH2 node, parent BVH4 node and slot, level, pushes above
    while todo:
        i, pn, ps, d, acc = todo.pop()
        me = len(out)
        o = np.zeros(32, np.float32)
        o[24:28] = np.array([-1] * 4, np.int32).view(np.float32)
        out.append(o)
        if pn >= 0:
            out[pn][24 + ps:25 + ps] = np.array([me], np.int32).view(np.float32)
        slots = []
        for ch in range(2):
            ref = int(_refs2(nodes[i])[ch])
            if ref == -1:
                continue
            if ref < 0:
                slots.append((*_box2(nodes[i], ch), ref))
            else:
                slots += [(*_box2(nodes[ref], g), int(_refs2(nodes[ref])[g])) for g in range(2)]
        k = len(slots)
        depth, stack = max(depth, d), max(stack, acc + k - 1)
        for q, (lo, hi, ref) in enumerate(slots):
            o[[q, 8 + q, 16 + q]], o[[4 + q, 12 + q, 20 + q]] = lo, hi
            o[24 + q:25 + q] = np.array([ref], np.int32).view(np.float32)
            if ref >= 0:
                todo.append((ref, me, q, d + 1, acc + k - 1))
    n4 = np.array(out, np.float32)
    upper = np.tile(np.repeat([False, True], 4), 3)[None, :].repeat(len(n4), 0)
    h = half_outward(n4[:, :24], upper)
    n4[:, :24] = h.astype(np.float32)
    half = np.zeros((len(n4), 64), np.uint8)
    half[:, :48] = h.view(np.uint8).reshape(len(n4), 48)
    half[:, 48:] = n4[:, 24:28].copy().view(np.uint8).reshape(len(n4), 16)
    return n4, half, depth, stack


def check_all(nodes, tris, nodes4, half, corners, depth=None, stack4=None, morton=False):
    """both validators, the reported depth and BVH4 stack need when given, and with `morton`
    the leaf order against morton_order -> (depth, BVH4 depth, stack need)"""
    d2 = check_bvh2(nodes, tris, corners)
    d4, st = check_bvh4(nodes4, nodes, tris, corners, half=half)
    _need(depth is None or depth == d2, "reported depth", depth, d2)
    _need(stack4 is None or stack4 == st, "reported stack need", stack4, st)
    if morton:
        pids = np.ascontiguousarray(tris, np.float32).reshape(-1, 12)[:, 3].copy().view(np.int32)
        _need(np.array_equal(pids, morton_order(corners)), "leaf order is not the Morton order")
    return d2, d4, st


def _sensitivity_scene():
    """41 triangles: 32 random ones, 8 copies of one triangle (equal codes), one far away"""
    rng = np.random.default_rng(77)
    cen = rng.uniform(-8, 8, (32, 1, 3))
    c = (cen + rng.uniform(-1, 1, (32, 3, 3))).astype(np.float32)
    same = np.repeat(np.array([[[1.5, 2.0, 3.0], [2.5, 2.25, 3.5], [1.75, 3.0, 3.25]]], np.float32), 8, 0)
    far = np.array([[[30.0, 31.0, 29.0], [31.0, 30.5, 30.0], [30.5, 30.0, 31.0]]], np.float32)
    return np.concatenate([c[:16], same, c[16:], far])


def check_sensitivity():
    """The validator on trees of its own making with tight boxes (no padding: every plane
    touches a corner): the trees pass, and every one of the mutations below is rejected.
    -> the names of the rejected mutations"""
    c = _sensitivity_scene()
    order = morton_order(c)
    codes = morton_codes(c)
    nodes, tris = range_tree(c, order=order, pad=0.0)
    n4, half, d4, st = collapse4(nodes)
    d2 = check_bvh2(nodes, tris, c)
    assert check_all(nodes, tris, n4, half, c, depth=d2, stack4=st, morton=True) == (d2, d4, st)
    u32 = lambda a: a.view(np.uint32)

    def leaf_slots(arr):
        """(node, child / slot, reference) of every leaf reference of a BVH2 / BVH4 array"""
        w = arr.shape[1]
        refs = arr[:, 12:14].view(np.int32) if w == 16 else arr[:, 24:28].view(np.int32)
        return [(i, q, int(refs[i, q])) for i in range(len(arr)) for q in range(refs.shape[1])
                if refs[i, q] < -1]

    def rejected(name, **kw):
        a = dict(nodes=nodes, tris=tris, nodes4=n4, half=half, corners=c, depth=d2, stack4=st, morton=True)
        a.update(kw)
        try:
            check_all(**a)
        except Invalid:
            return name
        raise AssertionError(f"the validator accepts: {name}")

    done = []
    l2, l4 = leaf_slots(nodes), leaf_slots(n4)
    # one leaf-box plane of the BVH2 one ulp inward (lo.x of the first leaf: a corner lies on it)
    i, ch, ref = l2[0]
    m = nodes.copy()
    m[i, 2 * ch] = np.nextafter(m[i, 2 * ch], np.float32(np.inf))
    done.append(rejected("leaf plane one ulp inward (lo)", nodes=m))
    m = nodes.copy()
    m[i, 9 + 2 * ch] = np.nextafter(m[i, 9 + 2 * ch], np.float32(-np.inf))
    done.append(rejected("leaf plane one ulp inward (hi)", nodes=m))
    # one BVH4 plane one binary16 quantum inward, in both forms of the node
    i, q, ref = l4[0]
    for word, step in ((8 + q, np.inf), (20 + q, -np.inf)):
        m4, mh = n4.copy(), half.copy()
        v = np.nextafter(np.float16(m4[i, word]), np.float16(step))
        m4[i, word] = np.float32(v)
        mh[i, 2 * word:2 * word + 2] = np.array([v], np.float16).view(np.uint8)
        done.append(rejected(f"BVH4 plane one binary16 quantum inward (word {word})", nodes4=m4, half=mh))
    # an internal slot's box one quantum inward: the child's boxes stick out of it
    inner = [(i, q) for i in range(len(n4)) for q in range(4) if n4[i, 24:28].view(np.int32)[q] >= 0]
    i, q = inner[0]
    m4, mh = n4.copy(), half.copy()
    v = np.nextafter(np.float16(m4[i, q]), np.float16(np.inf))
    m4[i, q] = np.float32(v)
    mh[i, 2 * q:2 * q + 2] = np.array([v], np.float16).view(np.uint8)
    done.append(rejected("BVH4 internal box one quantum inward", nodes4=m4, half=mh))
    # a triangle dropped from a leaf count
    i, ch, ref = next(x for x in l2 if _leaf(x[2])[1] >= 2)
    m = nodes.copy()
    u32(m)[i, 12 + ch] = (ref & 0xFFFFFFFF) - 1
    done.append(rejected("triangle dropped from a leaf count", nodes=m))
    # a leaf referenced twice (in place of another leaf of the same size, so only the pids tell)
    (i, ch, ref), (j, cj, rj) = l2[0], next(x for x in l2[1:] if _leaf(x[2])[1] == _leaf(l2[0][2])[1])
    m = nodes.copy()
    u32(m)[j, 12 + cj] = ref & 0xFFFFFFFF
    m[j, [2 * cj, 4 + 2 * cj, 8 + 2 * cj]] = nodes[i, [2 * ch, 4 + 2 * ch, 8 + 2 * ch]]
    m[j, [1 + 2 * cj, 5 + 2 * cj, 9 + 2 * cj]] = nodes[i, [1 + 2 * ch, 5 + 2 * ch, 9 + 2 * ch]]
    done.append(rejected("leaf referenced twice", nodes=m))
    # two leaf records swapped across leaves (the first record and the last: far apart)
    m = tris.copy()
    m[[0, len(m) - 1]] = m[[len(m) - 1, 0]]
    done.append(rejected("leaf records swapped across leaves", tris=m))
    # the reported stack bound off by one, either way; the reported depth too
    done.append(rejected("stack bound one too high", stack4=st + 1))
    done.append(rejected("stack bound one too low", stack4=st - 1))
    done.append(rejected("depth one too high", depth=d2 + 1))
    # a fp32 plane that is no binary16 value: one fp32 ulp outward, still containing
    i, q, ref = l4[0]
    m4 = n4.copy()
    m4[i, q] = np.nextafter(m4[i, q], np.float32(-np.inf))
    assert not is_binary16(m4[i, q])
    done.append(rejected("fp32 plane that is no binary16 value", nodes4=m4, half=None))
    done.append(rejected("half record that decodes to another plane", nodes4=m4))
    # two equal-code triangles swapped in the leaf order: records and tree stay consistent
    # (the copies are one triangle), only the order tells
    pids = tris[:, 3].copy().view(np.int32)
    k = next(k for k in range(len(pids) - 1) if codes[pids[k]] == codes[pids[k + 1]]
             and np.array_equal(c[pids[k]], c[pids[k + 1]]))
    m = tris.copy()
    m[[k, k + 1], 3] = m[[k + 1, k], 3]
    check_all(nodes, m, n4, half, c, depth=d2, stack4=st)          # still a valid tree
    done.append(rejected("equal-code triangles swapped in the leaf order", tris=m))
    # used slots not packed first, a node reached twice, a child past the array
    i = next(i for i in range(len(n4)) if (n4[i, 24:28].view(np.int32) != -1).sum() >= 3)
    m4 = n4.copy()
    u32(m4)[i, 24] = 0xFFFFFFFF
    done.append(rejected("used slots not packed first", nodes4=m4, half=None))
    if len(nodes) > 2:
        m = nodes.copy()
        j, cj = next((j, cj) for j in range(len(nodes)) for cj in range(2) if _refs2(nodes[j])[cj] > 0)
        u32(m)[j, 12 + cj] = 0
        done.append(rejected("node reached twice", nodes=m))
        m = nodes.copy()
        u32(m)[j, 12 + cj] = len(nodes)
        done.append(rejected("child past the array", nodes=m))
    return done
