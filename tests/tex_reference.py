"""Independent model of the texture sampler, written from the meaning of the
operations in plain per-channel arithmetic (numpy int64): no packed
two-channels-per-word lerp, no sign-smear wrap tricks, no pre-shifted
fractions.  The oracle (oracle/gfx.c orc_tex_read, oracle/tex.c), the RT
path's sampler (gfx_device.h) and the texture kernel (tex_kernel.hip) are
three transcriptions of one bit-trick source; this module is the second
opinion they are all held to (tests/test_tex_unit_cpu.py,
tests/test_gpu_tex_unit.py).  Test infrastructure only.

Coordinates are signed fixed point with F = 23 fraction bits: ONE = 2^23 is
the texture's width (height).  A colour is the word a<<24 | r<<16 | g<<8 | b.
"""
from __future__ import annotations

import numpy as np

F = 23
ONE = 1 << F
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
LOD_MAX = 15

A8R8G8B8, R5G6B5, A1R5G5B5, A4R4G4B4, A8L8, L8, A8 = range(7)
FORMATS = ("A8R8G8B8", "R5G6B5", "A1R5G5B5", "A4R4G4B4", "A8L8", "L8", "A8")
STRIDE = (4, 2, 2, 2, 2, 1, 1)
CLAMP, REPEAT, MIRROR = 0, 1, 2
POINT, BILINEAR, TRILINEAR = 0, 1, 2

# texel layout: channel -> (lowest bit, width); "l" is luminance (r = g = b).
# A channel that a format does not store reads as 255.
FIELDS = (
    {"a": (24, 8), "r": (16, 8), "g": (8, 8), "b": (0, 8)},
    {"r": (11, 5), "g": (5, 6), "b": (0, 5)},
    {"a": (15, 1), "r": (10, 5), "g": (5, 5), "b": (0, 5)},
    {"a": (12, 4), "r": (8, 4), "g": (4, 4), "b": (0, 4)},
    {"a": (8, 8), "l": (0, 8)},
    {"l": (0, 8)},
    {"a": (0, 8)},
)


def _i64(x):
    return np.asarray(x, dtype=np.int64)


def int32(x):
    """two's-complement wrap into [-2^31, 2^31)"""
    return (_i64(x) + (1 << 31)) % (1 << 32) - (1 << 31)


# ---- addressing -------------------------------------------------------------
def wrap(d, mode):
    """coordinate -> [0, ONE)"""
    d = _i64(d)
    if mode == CLAMP:
        return np.minimum(np.maximum(d, 0), ONE - 1)
    if mode == REPEAT:
        return d % ONE
    if mode == MIRROR:
        per, fr = np.divmod(d, ONE)
        return np.where(per % 2 == 1, ONE - 1 - fr, fr)
    raise ValueError(mode)


# ---- texel formats ------------------------------------------------------------
def expand(field, bits):
    """n-bit field -> 8 bits by bit replication (the field's bits repeated
    from the top until 8 are filled; 1 bit -> 0 or 255)"""
    field = _i64(field)
    rep, n = np.zeros_like(field), 0
    while n < 8:
        rep = rep * (1 << bits) + field
        n += bits
    return rep // (1 << (n - 8))


def decode(texel, fmt):
    """stored texel -> (a, r, g, b), each 0..255"""
    texel = _i64(texel)
    ch = {}
    for name, (lo, bits) in FIELDS[fmt].items():
        ch[name] = expand((texel // (1 << lo)) % (1 << bits), bits)
    full = np.full_like(texel, 255)
    if "l" in ch:
        ch["r"] = ch["g"] = ch["b"] = ch["l"]
    return tuple(ch.get(k, full) for k in "argb")


def encode(a, r, g, b, fmt):
    """8-bit channels -> stored texel: truncation to the channel width,
    luminance = the red channel, 1-bit alpha = (a != 0)"""
    src = {"a": _i64(a), "r": _i64(r), "g": _i64(g), "b": _i64(b), "l": _i64(r)}
    t = np.zeros_like(src["a"])
    for name, (lo, bits) in FIELDS[fmt].items():
        v = src[name]
        f = (v != 0).astype(np.int64) if bits == 1 else v // (1 << (8 - bits))
        t = t + f * (1 << lo)
    return t


def split(argb):
    c = _i64(argb)
    return (c // (1 << 24)) % 256, (c // (1 << 16)) % 256, (c // (1 << 8)) % 256, c % 256


def pack(a, r, g, b):
    return (_i64(a) * (1 << 24) + _i64(r) * (1 << 16) + _i64(g) * (1 << 8) + _i64(b)).astype(np.uint32)


def fetch(tex, base, idx, fmt):
    """little-endian texel `idx` of the level at byte offset `base`"""
    tex = np.asarray(tex, np.uint8)
    s = STRIDE[fmt]
    off = base + _i64(idx) * s
    t = np.zeros_like(off)
    for i in range(s):
        t = t + tex[off + i].astype(np.int64) * (1 << (8 * i))
    return t


# ---- filtering ------------------------------------------------------------------
def lerp(a, b, f):
    """a..b by f/255-ish, the sampler's rounding: p = a(255-f) + bf + 128,
    then (p + p/256) / 256"""
    p = _i64(a) * (255 - _i64(f)) + _i64(b) * _i64(f) + 128
    return (p + p // 256) // 256


def sample_level(tex, base, logw, logh, fmt, filt, wrapu, wrapv, u, v):
    """(a, r, g, b) of one level: `filt` POINT or BILINEAR"""
    W, H = 1 << logw, 1 << logh
    u, v = _i64(u), _i64(v)

    def texel(x, y):
        return decode(fetch(tex, base, x + y * W, fmt), fmt)

    if filt == POINT:
        x = wrap(u, wrapu) * W // ONE
        y = wrap(v, wrapv) * H // ONE
        return texel(x, y)
    du, dv = (ONE // 2) // W, (ONE // 2) // H     # half a texel
    u0, u1 = wrap(int32(u - du), wrapu), wrap(int32(u + du), wrapu)
    v0, v1 = wrap(int32(v - dv), wrapv), wrap(int32(v + dv), wrapv)
    x0, x1 = u0 * W // ONE, u1 * W // ONE
    y0, y1 = v0 * H // ONE, v1 * H // ONE
    alpha = (u0 * W * 256 // ONE) % 256          # position of u0 inside its texel
    beta = (v0 * H * 256 // ONE) % 256
    c00, c01, c10, c11 = texel(x0, y0), texel(x1, y0), texel(x0, y1), texel(x1, y1)
    return tuple(lerp(lerp(c00[k], c01[k], alpha), lerp(c10[k], c11[k], alpha), beta)
                 for k in range(4))


def level(mipoff, logw, logh, lod):
    """(byte offset, logw, logh) of level `lod`; an offset past the chain is
    0 (an unwritten register), so such a level reads the base image's bytes"""
    return int(mipoff[lod]), max(logw - lod, 0), max(logh - lod, 0)


def read(tex, mipoff, logw, logh, fmt, filt, wrapu, wrapv, u, v, lod=0):
    """the sampler: colour words at level `lod`, `filt` POINT or BILINEAR"""
    base, lw, lh = level(mipoff, logw, logh, lod)
    return pack(*sample_level(tex, base, lw, lh, fmt, filt, wrapu, wrapv, u, v))


def read_trilinear(tex, mipoff, logw, logh, fmt, wrapu, wrapv, u, v, lod, frac):
    """bilinear samples at `lod` and the next level, each channel lerped by frac"""
    c0 = sample_level(tex, *level(mipoff, logw, logh, lod), fmt, BILINEAR, wrapu, wrapv, u, v)
    c1 = sample_level(tex, *level(mipoff, logw, logh, min(lod + 1, LOD_MAX)), fmt, BILINEAR,
                      wrapu, wrapv, u, v)
    return pack(*(lerp(c0[k], c1[k], frac) for k in range(4)))


NO_MIPS = np.zeros(16, np.int64)


# ---- level of detail ------------------------------------------------------------
def lod_frac(logw, logh, dw, dh):
    """level and blend fraction of a dw x dh destination.  The minification
    is computed in float32 and converted to a signed 32-bit fixed point with
    16 fraction bits by a saturating conversion (known-answer row "lod_sat":
    at a ratio of 2^15 and above j is 2^31 - 1, so lod stops at 14)"""
    f32 = np.float32
    m = max(f32(1 << logw) / f32(dw), f32(1 << logh) / f32(dh), f32(1.0))
    j = min(int(f32(m) * f32(65536.0)), INT32_MAX)
    lod = min(j.bit_length() - 1 - 16, LOD_MAX)
    return lod, (j - (1 << (lod + 16))) >> (lod + 8)


# ---- images and mip chains ------------------------------------------------------
def texel_bytes(t, fmt):
    t = _i64(t).reshape(-1)
    s = STRIDE[fmt]
    out = np.zeros((t.size, s), np.uint8)
    for i in range(s):
        out[:, i] = (t // (1 << (8 * i))) % 256
    return out.reshape(-1)


def build_chain(argb, fmt):
    """ARGB8888 image [h, w] -> (bytes uint8[], mipoff int64[16], levels): the
    encoded image and every smaller level down to 1x1, each a 2x2 box of the
    decoded level above (sum / 4 per channel, truncating) encoded again; a
    side of length 1 stays at index 0"""
    argb = np.asarray(argb, np.uint32)
    h, w = argb.shape
    cur = encode(*split(argb), fmt)                       # [h, w] texels
    blobs, mipoff, off = [], np.zeros(16, np.int64), 0
    n = 0
    while True:
        if n < 16:
            mipoff[n] = off
        blobs.append(texel_bytes(cur, fmt))
        off += blobs[-1].size
        n += 1
        h, w = cur.shape
        if h == 1 and w == 1:
            break
        nh, nw = max(h // 2, 1), max(w // 2, 1)
        ys, xs = np.mgrid[0:nh, 0:nw]
        acc = [np.zeros((nh, nw), np.int64) for _ in range(4)]
        for ky in (0, 1):
            for kx in (0, 1):
                sy = 2 * ys + ky if h > 1 else 0 * ys
                sx = 2 * xs + kx if w > 1 else 0 * xs
                for k, c in enumerate(decode(cur[sy, sx], fmt)):
                    acc[k] += c
        cur = encode(*(c // 4 for c in acc), fmt)
    return np.concatenate(blobs), mipoff, n


# ---- whole images -----------------------------------------------------------------
def render_tab(tex, mipoff, logw, logh, fmt, wrapm, filt, lod, frac, utab, vtab):
    """destination image [len(vtab), len(utab)]: pixel (y, x) samples (utab[x],
    vtab[y]) with both axes under wrap mode `wrapm`; filt POINT / BILINEAR at
    `lod`, TRILINEAR blending `lod` and the next level by `frac`"""
    u, v = np.meshgrid(_i64(utab), _i64(vtab))
    if filt == TRILINEAR:
        return read_trilinear(tex, mipoff, logw, logh, fmt, wrapm, wrapm, u, v, lod, frac)
    return read(tex, mipoff, logw, logh, fmt, filt, wrapm, wrapm, u, v, lod)


def fx23(f):
    """float32 -> fixed point, truncating (values here are far from the int32 range)"""
    return int(np.float32(f) * np.float32(ONE))


def app_tables(dw, dh, num_tasks):
    """the regression app's coordinates: u accumulated in float32 per column
    from 0.5/dw in steps of 1/dw; v likewise per row, restarted at
    (y0 + 0.5)/dh at the first row y0 of every task's tile of rows"""
    f32 = np.float32
    dx, dy = f32(1.0) / f32(dw), f32(1.0) / f32(dh)
    utab, fu = [], f32(0.5) * dx
    for _ in range(dw):
        utab.append(fx23(fu))
        fu = f32(fu + dx)
    tile = (dh + num_tasks - 1) // num_tasks
    vtab = []
    for y0 in range(0, dh, tile):
        fv = f32(f32(y0) + f32(0.5)) * dy
        for _ in range(y0, min(y0 + tile, dh)):
            vtab.append(fx23(fv))
            fv = f32(fv + dy)
    return np.array(utab, np.int64), np.array(vtab, np.int64)


def render_app(argb, fmt=0, wrapm=0, filt=0, scale=1.0, num_tasks=0, chain=None):
    """the whole regression app: the image scaled by `scale` (float32,
    truncated per side), one task per row unless num_tasks is given; `chain`
    = build_chain(argb, fmt) when the caller already has it"""
    argb = np.asarray(argb, np.uint32)
    h, w = argb.shape
    logw, logh = w.bit_length() - 1, h.bit_length() - 1
    tex, mipoff, _ = chain or build_chain(argb, fmt)
    dw, dh = int(np.float32(w) * np.float32(scale)), int(np.float32(h) * np.float32(scale))
    lod, frac = lod_frac(logw, logh, dw, dh)
    utab, vtab = app_tables(dw, dh, min(num_tasks or dh, dh))
    return render_tab(tex, mipoff, logw, logh, fmt, wrapm, filt, lod, frac, utab, vtab)
