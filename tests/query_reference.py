"""What the ray-query tests share: the coherence key of include/vx_rt.h restated
in numpy (float32 operation by operation), a hand-worked key table, the
malformed rays, and the per-scene references of the walk scenes (tests/
ray_known_answers.py), computed once per process and never modified."""
import numpy as np

INF = float("inf")
NAN = float("nan")
MISS_KEY = 0xFFFFFFFF


def malformed(rays):
    """rays float32 [n, 8] (o, d, tmin, tmax) -> bool [n]: any word NaN, an
    infinite origin or direction component, or an all-zero direction"""
    w = np.ascontiguousarray(rays, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    nan = (w > 0x7F800000).any(1)
    inf = (w[:, :6] == 0x7F800000).any(1)
    zero = (w[:, 3:6] == 0).all(1)
    return nan | inf | zero


def _part3(c):
    out = np.zeros(c.shape, np.uint32)
    for b in range(7):
        out |= ((c >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
    return out


def key_numpy(rays, box):
    """the key definition of vx_rt.h, every operation in float32 -> uint32 [n]"""
    r = np.ascontiguousarray(rays, np.float32)
    box = np.asarray(box, np.float32).reshape(6)
    lo, hi = box[:3], box[3:]
    bad = malformed(r)
    with np.errstate(all="ignore"):
        ext = (hi - lo).astype(np.float32)
        inv = np.where(hi > lo, np.float32(128.0) / np.where(hi > lo, ext, np.float32(1.0)), np.float32(0.0))
        inv = inv.astype(np.float32)
        key = np.zeros(len(r), np.uint32)
        w = r.view(np.uint32)
        for a in range(3):
            key |= (w[:, 3 + a] >> np.uint32(31)) << np.uint32(31 - a)
            g = ((r[:, a] - lo[a]).astype(np.float32) * inv[a]).astype(np.float32)
            c = np.fmin(np.fmax(g, np.float32(0.0)), np.float32(127.0)).astype(np.uint32)
            key |= _part3(c) << np.uint32(8 + a)
        m = np.abs(r[:, 3:6]).astype(np.float32)
        s = ((m[:, 0] + m[:, 1]).astype(np.float32) + m[:, 2]).astype(np.float32)
        s = np.where(bad, np.float32(1.0), s)
        for a, sh in ((0, 0), (1, 4)):
            q = ((m[:, a] / s).astype(np.float32) * np.float32(16.0)).astype(np.float32)
            cell = np.fmin(np.where(bad, np.float32(0.0), q), np.float32(15.0)).astype(np.uint32)
            key |= cell << np.uint32(sh)
    return np.where(bad, np.uint32(MISS_KEY), key).astype(np.uint32)


# ---- the hand-worked table --------------------------------------------------------------
# (o, d, tmin, tmax, box, key).  Box U = [0, 128]^3: inv = 1 per axis, a cell is floor(o) clamped to
# 0..127.  Morton: bit i of x at 3 i, of y at 3 i + 1, of z at 3 i + 2; the code sits at key bits 8..28.
# The direction cells are floor(16 |d.x| / s) and floor(16 |d.y| / s), each capped at 15, s = |d.x| +
# |d.y| + |d.z|; y's cell at bits 4..7, x's at bits 0..3.  Signs of d.x, d.y, d.z at bits 31, 30, 29.
U = (0.0, 0.0, 0.0, 128.0, 128.0, 128.0)
BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
HAND_ROWS = [
    # on the three low faces, d along +x: cells 0; 16 * 1 = 16 capped to 15, y's cell 0
    ((0, 0, 0), (1, 0, 0), 0.0, INF, U, 0x0000000F),
    # on the three high faces: 128 clamps to 127 on every axis = all 21 Morton bits; d along -y: bit 30,
    # y's cell 15 (-0.0 components carry their sign bit: none here)
    ((128, 128, 128), (0, -1, 0), 0.0, 1.0, U, 0x5FFFFFF0),
    # outside: x below (cell 0), y above (cell 127: bits 1, 4, .., 19 = 0x92492), z = 64 (bit 6 of z = Morton
    # bit 20 = 0x100000); d along -z: bit 29, both cells 0
    ((-5, 200, 64), (0, 0, -2), 0.0, INF, U, 0x39249200),
    # on the high x face only: x cell 127 (bits 0, 3, .., 18 = 0x49249), y = 5 (bits 1, 7 = 130), z = 5
    # (bits 2, 8 = 260): 0x49249 + 390 = 0x493CF; d = (1, 1, 2): s = 4, both quotients 1/4 -> cell 4
    ((128, 5, 5), (1, 1, 2), 0.0, INF, U, 0x0493CF44),
    # on the high y face and the high z face, one each
    ((0, 128, 0), (1, 1, 2), 0.0, INF, U, 0x09249244),   # y cell 127 = 0x92492
    ((0, 0, 128), (1, 1, 2), 0.0, INF, U, 0x12492444),   # z cell 127 = 0x124924
    # the eight octants from the origin cell, |d| = (1, 1, 2): cells 4, 4
    ((0, 0, 0), (1, 1, 2), 0.0, INF, U, 0x00000044),
    ((0, 0, 0), (1, 1, -2), 0.0, INF, U, 0x20000044),
    ((0, 0, 0), (1, -1, 2), 0.0, INF, U, 0x40000044),
    ((0, 0, 0), (1, -1, -2), 0.0, INF, U, 0x60000044),
    ((0, 0, 0), (-1, 1, 2), 0.0, INF, U, 0x80000044),
    ((0, 0, 0), (-1, 1, -2), 0.0, INF, U, 0xA0000044),
    ((0, 0, 0), (-1, -1, 2), 0.0, INF, U, 0xC0000044),
    ((0, 0, 0), (-1, -1, -2), 0.0, INF, U, 0xE0000044),
    # o = (1, 2, 3): x bit 0 -> 1; y bit 1 -> Morton bit 4 = 16; z bits 0, 1 -> Morton bits 2, 5 = 36: 53 = 0x35
    ((1, 2, 3), (-1, -1, -2), 0.0, INF, U, 0xE0003544),
    # x = 64: bit 6 -> Morton bit 18; d = (2, -1, 1): s = 4, x quotient 1/2 -> 8, y 1/4 -> 4
    ((64, 0, 0), (2, -1, 1), 0.0, INF, U, 0x44000048),
    # the direction cells' boundary 15 / 16: 15/16 * 16 = 15 exactly -> 15, 1/16 * 16 = 1 -> 1 ...
    ((0, 0, 0), (15, 1, 0), 0.0, INF, U, 0x0000001F),
    # ... and 239/256 * 16 = 14.9375 -> 14, 17/256 * 16 = 1.0625 -> 1
    ((0, 0, 0), (239, 17, 0), 0.0, INF, U, 0x0000001E),
    # d along y and along z
    ((0, 0, 0), (0, 3, 0), 0.0, INF, U, 0x000000F0),
    ((0, 0, 0), (0, 0, 3), 0.0, INF, U, 0x00000000),
    # the origin cells' boundary: the float below 1 is cell 0, 1 is cell 1 (y: Morton bit 1)
    ((BELOW_ONE, 1, 0), (0, 0, 1), 0.0, INF, U, 0x00000200),
    # a flat axis: inv.z = 0, z's cell 0 wherever the origin is; x = 2: bit 1 -> Morton bit 3
    ((2, 0, 77), (0, 0, 1), 0.0, INF, (0, 0, 5, 128, 128, 5), 0x00000800),
    # box [-16, 16]^3: inv = 128 / 32 = 4; the centre is cell 64 on every axis: Morton bits 18, 19, 20
    ((0, 0, 0), (0, 1, 0), 0.0, INF, (-16, -16, -16, 16, 16, 16), 0x1C0000F0),
    # tmin = -inf and tmax = +inf are admitted
    ((0, 0, 0), (1, 1, 2), -INF, INF, U, 0x00000044),
    # malformed, one of each kind: an all-zero direction (of either sign), a NaN in each group of words,
    # an infinite origin component, an infinite direction component
    ((1, 2, 3), (0, -0.0, 0), 0.0, INF, U, MISS_KEY),
    ((NAN, 2, 3), (1, 1, 2), 0.0, INF, U, MISS_KEY),
    ((1, 2, 3), (1, NAN, 2), 0.0, INF, U, MISS_KEY),
    ((1, 2, 3), (1, 1, 2), NAN, INF, U, MISS_KEY),
    ((1, 2, 3), (1, 1, 2), 0.0, NAN, U, MISS_KEY),
    ((1, INF, 3), (1, 1, 2), 0.0, INF, U, MISS_KEY),
    ((1, 2, 3), (1, 1, -INF), 0.0, INF, U, MISS_KEY),
]


def hand_rays():
    """-> rays float32 [n, 8], boxes float32 [n, 6], keys uint32 [n]"""
    rays = np.array([list(o) + list(d) + [tmin, tmax] for o, d, tmin, tmax, _, _ in HAND_ROWS], np.float32)
    boxes = np.array([b for *_, b, _ in HAND_ROWS], np.float32)
    keys = np.array([k for *_, k in HAND_ROWS], np.uint32)
    return rays, boxes, keys


# one malformed ray of each kind, as (column, value) edits of a valid ray; "zero" clears the direction
MALFORMED_KINDS = {
    "zero_direction": [(3, 0.0), (4, -0.0), (5, 0.0)],
    "nan_origin": [(1, NAN)],
    "nan_direction": [(5, NAN)],
    "nan_tmin": [(6, NAN)],
    "nan_tmax": [(7, NAN)],
    "inf_origin": [(0, INF)],
    "inf_direction": [(4, -INF)],
}


def with_malformed(rays, kind, lanes=(0, 31, 63)):
    out = np.array(rays, np.float32, copy=True)
    for ln in lanes:
        for col, v in MALFORMED_KINDS[kind]:
            out[ln, col] = v
    return out


def corner_box(corners):
    """the bounds of corners float32 [T, 3, 3] -> float32 [6] (lo.xyz, hi.xyz); zeros when T = 0"""
    c = np.asarray(corners, np.float32).reshape(-1, 3)
    if len(c) == 0:
        return np.zeros(6, np.float32)
    return np.concatenate([c.min(0), c.max(0)]).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
