"""The texture sampler's state-space sweeps, shared by the CPU tests
(tests/test_tex_unit_cpu.py: oracle against the model) and the GPU tests
(tests/test_gpu_tex_unit.py: gfx::tex_read / tex_read_any and the texture
kernel against the model).  Everything is seeded; the expected values come
from tests/tex_reference.py alone.

Unit sweep: 7 texture shapes x 7 formats x {point, bilinear} x 9 (wrapu,
wrapv) pairs = 882 sampler states, each sampled at UNIT_PER_STATE coordinate
pairs (edge values around 0, one texel, the texture's far edge, whole periods
on both sides and the int32 extremes, plus random ones) -- UNIT_SAMPLES in all.

Image sweep, for the texture kernel: 7 formats x 3 wraps x 3 textures (with
the model's mip chain) x 8 destination widths x 3 lods x (point, bilinear,
trilinear at 4 blend fractions) = IMAGE_CASES destination images of height 3.
"""
from __future__ import annotations

import functools
import itertools

import numpy as np

import tex_reference as tr

ONE = tr.ONE
SEED = 20240607

# ---- coordinates --------------------------------------------------------------
N_RANDOM = 12


def edge_set(log):
    """per-axis edge coordinates of a 2^log-texel side (T = one texel)"""
    T = ONE >> log
    h = T // 2
    return [0, 1, -1,
            T - 1, T,
            h, h + 1, h - 1,
            ONE - 1, ONE, ONE + 1,
            ONE - h, ONE - h - 1,
            2 * ONE - 1, 2 * ONE,
            -ONE, -ONE - 1, -ONE + h,
            3 * ONE + 5,
            tr.INT32_MIN, tr.INT32_MAX,
            tr.INT32_MAX - h + 1,      # u + half a texel wraps to INT32_MIN
            tr.INT32_MIN + h - 1]      # u - half a texel wraps to INT32_MAX


V_PER_U = 3   # v-edges every u-edge meets


def unit_coords(logw, logh, rng):
    """(u, v) int64 arrays: every u-edge paired with V_PER_U v-edges by a fixed
    stride (5 and 7 are coprime to the 23 edges, so the pairs spread over the
    whole v set), then N_RANDOM random pairs in [-4 ONE, 4 ONE)"""
    eu, ev = edge_set(logw), edge_set(logh)
    u, v = [], []
    for i, x in enumerate(eu):
        for k in range(V_PER_U):
            u.append(x)
            v.append(ev[(5 * i + 7 * k + 3) % len(ev)])
    u += rng.integers(-4 * ONE, 4 * ONE, N_RANDOM).tolist()
    v += rng.integers(-4 * ONE, 4 * ONE, N_RANDOM).tolist()
    return np.array(u, np.int64), np.array(v, np.int64)


# ---- unit sweep -----------------------------------------------------------------
SHAPES = ((0, 0), (1, 0), (0, 2), (2, 2), (3, 1), (1, 4), (5, 3))   # (logw, logh)
WRAP_PAIRS = tuple(itertools.product(range(3), range(3)))
UNIT_PER_STATE = 23 * V_PER_U + N_RANDOM
UNIT_STATES = len(SHAPES) * 7 * 2 * len(WRAP_PAIRS)
UNIT_SAMPLES = UNIT_STATES * UNIT_PER_STATE


class UnitState:
    """one sampler state of the unit sweep and its coordinates"""
    __slots__ = ("shape", "logw", "logh", "fmt", "filt", "wrapu", "wrapv", "tex", "u", "v")

    def key(self):
        return (self.logw, self.logh, self.fmt, self.filt, self.wrapu, self.wrapv)


@functools.lru_cache(maxsize=None)
def unit_textures():
    """{(shape index, fmt): seeded random texel bytes uint8[]}"""
    rng = np.random.default_rng(SEED)
    out = {}
    for si, (logw, logh) in enumerate(SHAPES):
        for fmt in range(7):
            out[si, fmt] = rng.integers(0, 256, (1 << (logw + logh)) * tr.STRIDE[fmt], dtype=np.uint8)
    return out


@functools.lru_cache(maxsize=None)
def unit_states():
    """the unit sweep, in a fixed order"""
    texs = unit_textures()
    rng = np.random.default_rng(SEED + 1)
    states = []
    for si, (logw, logh) in enumerate(SHAPES):
        u, v = unit_coords(logw, logh, rng)   # one coordinate table per shape
        for fmt in range(7):
            for filt in (tr.POINT, tr.BILINEAR):
                for wrapu, wrapv in WRAP_PAIRS:
                    s = UnitState()
                    s.shape, s.logw, s.logh, s.fmt, s.filt = si, logw, logh, fmt, filt
                    s.wrapu, s.wrapv, s.tex, s.u, s.v = wrapu, wrapv, texs[si, fmt], u, v
                    states.append(s)
    assert len(states) == UNIT_STATES and sum(s.u.size for s in states) == UNIT_SAMPLES
    return tuple(states)


def model_unit(s, model=tr):
    """the model's colour words of one unit state"""
    return model.read(s.tex, tr.NO_MIPS, s.logw, s.logh, s.fmt, s.filt, s.wrapu, s.wrapv, s.u, s.v)


@functools.lru_cache(maxsize=None)
def unit_expected():
    """the model over the whole unit sweep, computed once: tuple of uint32 arrays"""
    out = []
    for s in unit_states():
        e = model_unit(s)
        e.setflags(write=False)
        out.append(e)
    return tuple(out)


# ---- image sweep ----------------------------------------------------------------
IMAGE_TEXTURES = ((4, 4), (8, 2), (2, 16))     # (width, height)
IMAGE_WIDTHS = (1, 63, 64, 65, 255, 256, 257, 513)
IMAGE_HEIGHT = 3
IMAGE_WMAX = max(IMAGE_WIDTHS)
FILTER_FRACS = ((tr.POINT, 0), (tr.BILINEAR, 0), (tr.TRILINEAR, 0), (tr.TRILINEAR, 1),
                (tr.TRILINEAR, 128), (tr.TRILINEAR, 255))
IMAGE_CASES = 7 * 3 * len(IMAGE_TEXTURES) * len(IMAGE_WIDTHS) * 3 * len(FILTER_FRACS)


class ImageTexture:
    """one texture of the image sweep in one format: the model's chain and
    the coordinate tables (the edge set cycled: column x takes edge x, row y
    edge 7 y + 4, so the 3 rows sit in different places of the set)"""
    __slots__ = ("index", "w", "h", "logw", "logh", "fmt", "tex", "mipoff", "levels", "utab", "vtab")

    def lods(self):
        return (0, 1, self.levels - 1)


@functools.lru_cache(maxsize=None)
def image_textures():
    """{(texture index, fmt): ImageTexture}"""
    rng = np.random.default_rng(SEED + 2)
    out = {}
    for ti, (w, h) in enumerate(IMAGE_TEXTURES):
        argb = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
        for fmt in range(7):
            t = ImageTexture()
            t.index, t.w, t.h, t.fmt = ti, w, h, fmt
            t.logw, t.logh = w.bit_length() - 1, h.bit_length() - 1
            t.tex, t.mipoff, t.levels = tr.build_chain(argb, fmt)
            eu, ev = edge_set(t.logw), edge_set(t.logh)
            t.utab = np.array([eu[x % len(eu)] for x in range(IMAGE_WMAX)], np.int64)
            t.vtab = np.array([ev[(7 * y + 4) % len(ev)] for y in range(IMAGE_HEIGHT)], np.int64)
            out[ti, fmt] = t
    return out


def image_cases(filt=None):
    """(texture, wrap, filter, frac, lod, dst_width) of every case, in a fixed
    order; `filt` keeps one filter's cases (the texture kernel has one image
    per filter)"""
    texs = image_textures()
    for (ti, fmt), t in sorted(texs.items()):
        for wrapm in range(3):
            for f, frac in FILTER_FRACS:
                if filt is not None and f != filt:
                    continue
                for lod in t.lods():
                    for dw in IMAGE_WIDTHS:
                        yield t, wrapm, f, frac, lod, dw


@functools.lru_cache(maxsize=None)
def image_expected_full(ti, fmt, wrapm, filt, frac, lod):
    """the model's image at the widest destination; column x depends on
    utab[x] alone, so a narrower destination is its first columns"""
    t = image_textures()[ti, fmt]
    e = tr.render_tab(t.tex, t.mipoff, t.logw, t.logh, fmt, wrapm, filt, lod, frac, t.utab, t.vtab)
    e.setflags(write=False)
    return e


def image_expected(t, wrapm, filt, frac, lod, dw):
    return image_expected_full(t.index, t.fmt, wrapm, filt, frac, lod)[:, :dw]


# ---- sensitivity ----------------------------------------------------------------
def check_sensitivity():
    """The sweeps tell the sampler's states apart on the model alone: were two
    states confused by an implementation, some sample would show it.  Raises
    AssertionError naming the first pair the sweep cannot separate."""
    exp = {s.key(): e for s, e in zip(unit_states(), unit_expected())}
    differs = lambda a, b: bool(np.any(exp[a] != exp[b]))
    # every pair of wrap modes, on u and on v, for each filter and format
    for fmt, filt in itertools.product(range(7), (0, 1)):
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert any(differs((lw, lh, fmt, filt, a, 0), (lw, lh, fmt, filt, b, 0))
                       for lw, lh in SHAPES), f"wrapu {a} vs {b}: fmt {fmt} filter {filt}"
            assert any(differs((lw, lh, fmt, filt, 0, a), (lw, lh, fmt, filt, 0, b))
                       for lw, lh in SHAPES), f"wrapv {a} vs {b}: fmt {fmt} filter {filt}"
        # wrapu swapped with wrapv
        for a, b in ((0, 1), (0, 2), (1, 2)):
            assert any(differs((lw, lh, fmt, filt, a, b), (lw, lh, fmt, filt, b, a))
                       for lw, lh in SHAPES), f"wrap swap {a},{b}: fmt {fmt} filter {filt}"
    # point and bilinear
    for fmt, (wu, wv) in itertools.product(range(7), WRAP_PAIRS):
        assert any(differs((lw, lh, fmt, 0, wu, wv), (lw, lh, fmt, 1, wu, wv))
                   for lw, lh in SHAPES), f"point vs bilinear: fmt {fmt} wrap {wu},{wv}"
    # every two formats of equal stride, decoding the same bytes
    for s in unit_states():
        for other in range(7):
            if other <= s.fmt or tr.STRIDE[other] != tr.STRIDE[s.fmt] or s.shape != 3:
                continue
            if (s.wrapu, s.wrapv) != (1, 1):
                continue
            a = tr.read(s.tex, tr.NO_MIPS, s.logw, s.logh, s.fmt, s.filt, 1, 1, s.u, s.v)
            b = tr.read(s.tex, tr.NO_MIPS, s.logw, s.logh, other, s.filt, 1, 1, s.u, s.v)
            assert np.any(a != b), f"formats {s.fmt} vs {other}: filter {s.filt}"
    # image sweep: the blend fraction and the level
    for (ti, fmt), t in sorted(image_textures().items()):
        for wrapm in range(3):
            f0 = image_expected_full(ti, fmt, wrapm, tr.TRILINEAR, 0, 0)
            f255 = image_expected_full(ti, fmt, wrapm, tr.TRILINEAR, 255, 0)
            assert np.any(f0 != f255), f"frac 0 vs 255: texture {ti} fmt {fmt} wrap {wrapm}"
            for filt in (tr.POINT, tr.BILINEAR, tr.TRILINEAR):
                l0 = image_expected_full(ti, fmt, wrapm, filt, 0, 0)
                l1 = image_expected_full(ti, fmt, wrapm, filt, 0, 1)
                assert np.any(l0 != l1), f"lod 0 vs 1: texture {ti} fmt {fmt} wrap {wrapm} filter {filt}"
