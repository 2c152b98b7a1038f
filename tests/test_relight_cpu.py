"""Relighting from the visibility records (vx_rt.h rt_relight_capture_start /
rt_render_relight_start): the exported entry points, the shipped images, and
rt_relight_resolve -- the relit pixel from its base colour, its record's
depth_flags and light_mask and per-light weights -- against a numpy restatement
of the definition: with RT_AOV_SHADOW_RAY, per channel (2 * ((W - O) * c + O *
(c >> 1)) + W) // (2 * W), W the sum of the n weights and O the sum of those
whose mask bit is set, under the base colour's alpha; else the base colour.
True integer division here; the library multiplies and shifts.  No GPU."""
import ctypes as C
import os

import numpy as np

from skybox_rt_amd import _lib, rt

SRAY = rt.RT_AOV_SHADOW_RAY
# every channel value 0..255 in each of the three channels, under two alphas: pixel i has
# R = i, G = 255 - i, B = (i * 7) & 255
_I = np.arange(256, dtype=np.uint32)
COLOURS = np.concatenate([(np.uint32(a) << np.uint32(24)) | (_I << np.uint32(16)) | ((np.uint32(255) - _I) << np.uint32(8))
                          | ((_I * np.uint32(7)) & np.uint32(0xFF)) for a in (0xFF, 0x01)])
# the same 256 values in 86 pixels: R = j, G = j + 85, B = j + 170 (for the drawn weight vectors)
_J = np.arange(86, dtype=np.uint32)
PACKED = np.uint32(0x80000000) | (_J << np.uint32(16)) | ((_J + np.uint32(85)) << np.uint32(8)) | (_J + np.uint32(170))


def model(base, sray, mask, weights):
    """the definition on a uint32 array of base colours, one mask and one shadow-ray flag"""
    base = np.asarray(base, np.uint64)
    n = len(weights)
    W = int(sum(weights))
    if not sray or W == 0 or not 1 <= n <= 16:
        return base.astype(np.uint32)
    O = sum(int(w) for i, w in enumerate(weights) if (mask >> i) & 1)
    out = base & np.uint64(0xFF000000)
    for sh in (16, 8, 0):
        c = (base >> np.uint64(sh)) & np.uint64(0xFF)
        s = np.uint64(W - O) * c + np.uint64(O) * (c >> np.uint64(1))
        out = out | (((np.uint64(2) * s + np.uint64(W)) // np.uint64(2 * W)) << np.uint64(sh))
    return out.astype(np.uint32)


def named_vectors():
    vs = [[1] * n for n in range(1, 17)]
    vs += [[int(i == j) for i in range(n)] for n in (1, 2, 3, 5, 16) for j in range(n)]
    return vs + [[255] * 16, [1, 0, 255, 3], [255], [255, 64, 1], list(range(1, 17)), [0, 0, 7], [254, 255] * 8]


def drawn_vectors():
    rng = np.random.default_rng(17)
    vs = []
    for _ in range(200):
        n = int(rng.integers(1, 17))
        v = rng.integers(0, 256, n)
        if rng.random() < 0.3:
            v[rng.random(n) < 0.5] = 0
        if v.sum() == 0:
            v[0] = 1
        vs.append([int(x) for x in v])
    return vs


def masks_for(n, rng):
    """every mask of a small n; 64 drawn ones of n = 16 (and of every n above 6), with 0 and all-ones"""
    if n <= 6:
        return list(range(1 << n))
    return [0, (1 << n) - 1] + [int(x) for x in rng.integers(0, 1 << n, 64)]


def test_entry_points_exported():
    h = C.CDLL(os.path.join(_lib.LIB_DIR, "librtapp.so"))
    for name in ("rt_relight_capture_start", "rt_relight_capture", "rt_render_relight_start", "rt_render_relight",
                 "rt_read_relight_base", "rt_relight_resolve"):
        assert hasattr(h, name), name
    for image in ("rt_aov_base.vxbin", "rt_relight.vxbin"):
        assert image in _lib.REQUIRED
        assert os.path.isfile(os.path.join(_lib.LIB_DIR, image))


def test_resolve_equals_the_definition():
    rng = np.random.default_rng(18)
    assert set(int(c) for sh in (16, 8, 0) for c in (PACKED >> np.uint32(sh)) & np.uint32(0xFF)) == set(range(256))
    checked = 0
    # (the second alpha of COLOURS: the tests below)
    for cols, vectors in ((COLOURS[:256], named_vectors()), (PACKED, drawn_vectors())):
        for w in vectors:
            for m in masks_for(len(w), rng):
                got = rt.relight_resolve(cols, np.uint32(SRAY), np.uint32(m), w)
                want = model(cols, True, m, w)
                assert got.dtype == np.uint32 and np.array_equal(got, want), (w, hex(m))
                checked += 1
    assert checked > 10000


def test_zero_one_weights_are_lights_resolve_on_the_enabled_subset():
    rng = np.random.default_rng(19)
    cols = COLOURS[::5]
    for n in range(1, 17):
        for _ in range(12):
            en = int(rng.integers(1, 1 << n))
            m = int(rng.integers(0, 1 << n))
            w = [(en >> i) & 1 for i in range(n)]
            k, o = bin(en).count("1"), bin(m & en).count("1")
            got = rt.relight_resolve(cols, np.uint32(SRAY | 0x123456), np.uint32(m), w)
            want = np.array([rt.lights_resolve(int(c), o, k) for c in cols], np.uint32)
            assert np.array_equal(got, want), (n, hex(en), hex(m))
            # and through rt_aov_relight when the enabled lights are the first k
            if en == (1 << k) - 1:
                assert np.array_equal(got, rt.aov_relight(cols, np.uint32(m), k))


def test_mask_bits_at_or_above_n_are_ignored():
    for w in ([3], [1, 0, 255, 3], [9] * 15):
        n = len(w)
        high = (0xFFFFFFFF << n) & 0xFFFFFFFF
        for m in (0, 1, (1 << n) - 1):
            want = model(COLOURS, True, m, w)
            for extra in (high, 1 << n, 0x80000000, high & 0x55555555):
                assert np.array_equal(rt.relight_resolve(COLOURS, np.uint32(SRAY), np.uint32(m | extra), w), want)


def test_base_colour_returned():
    """without RT_AOV_SHADOW_RAY, with W = 0, with n = 17 (and n = 0): the base colour"""
    for w in ([1, 2, 3], [255] * 16):
        for df in (0, rt.RT_AOV_GEOM | 0x00ABCDEF, 0xFFFFFFFF & ~SRAY):
            assert np.array_equal(rt.relight_resolve(COLOURS, np.uint32(df), np.uint32(0xFFFF), w), COLOURS)
    for w in ([0], [0, 0, 0], [0] * 16, [1] * 17, [255] * 17):
        assert np.array_equal(rt.relight_resolve(COLOURS, np.uint32(SRAY), np.uint32(0xFFFFFFFF), w), COLOURS)
        assert rt.relight_resolve(0x80FE0100, SRAY, 0xFFFF, w) == 0x80FE0100
    h = rt.lib()
    one = (C.c_uint8 * 1)(5)
    assert h.rt_relight_resolve(0x80FE0100, SRAY, 1, C.cast(one, C.c_void_p), 0) == 0x80FE0100
    assert h.rt_relight_resolve(0x80FE0100, SRAY, 1, None, 1) == 0x80FE0100
    # scalars; one light that does not see the pixel: c >> 1 per channel whatever its weight
    assert rt.relight_resolve(0x80FE0100, SRAY, 1, [7]) == 0x807F0000
    assert rt.relight_resolve(0x80FE0100, SRAY, 0, [7]) == 0x80FE0100
    # a flag and a mask per pixel (arrays broadcast)
    rng = np.random.default_rng(20)
    masks = rng.integers(0, 1 << 16, COLOURS.size, dtype=np.uint64).astype(np.uint32)
    flags = np.where(rng.random(COLOURS.size) < 0.5, np.uint32(SRAY), np.uint32(0)).astype(np.uint32)
    w = list(range(16, 0, -1))
    got = rt.relight_resolve(COLOURS, flags, masks, w)
    for i in range(0, COLOURS.size, 7):
        assert int(got[i]) == int(model(COLOURS[i:i + 1], bool(flags[i]), int(masks[i]), w)[0]), i
