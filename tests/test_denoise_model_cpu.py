"""The denoiser (vx_rt.h rt_denoise_capture_start / rt_render_denoise_start): the
exported entry points and shipped images, and hand-worked known answers that
pin the numpy model of tests/denoise_reference.py, which the device frames are
held to bit for bit (tests/test_gpu_denoise.py).  Expected values are worked
here with Python integers from the definition's formulas.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_reference as dr
from skybox_rt_amd import _lib, rt

H, W = 40, 48  # a stride of 16 reaches every border from the middle


def scene(h=H, w=W, pid=7, z=5000, normal=(0, 0, 127)):
    """a flat field: every pixel geometry of one primitive"""
    return dict(pid=np.full((h, w), pid, np.int32), z=np.full((h, w), z, np.uint32),
                geom=np.ones((h, w), bool), normal=np.tile(np.array(normal, np.int64), (h, w, 1)))


def records(h, w, s, n):
    rec = np.zeros((h, w, 4), np.uint32)
    rec[..., :3] = s
    rec[..., 3] = n
    return rec


def argb(a, r, g, b):
    return (a << 24) | (r << 16) | (g << 8) | b


def irr(s, n, a):
    d = n * max(a, 1)
    return min(65535, (256 * s + d // 2) // d)


def remod(i, a):
    return min(255, (i * a + 128) >> 8)


def test_exports_and_images():
    h = C.CDLL(os.path.join(_lib.LIB_DIR, "librtapp.so"))
    for name in ("rt_denoise_capture_start", "rt_denoise_capture", "rt_render_denoise_start", "rt_render_denoise",
                 "rt_read_denoise_guide", "rt_write_accum"):
        assert hasattr(h, name), name
    for img in ("rt_aov_guide.vxbin", "rt_denoise_prep.vxbin", "rt_denoise_pass.vxbin"):
        assert img in _lib.REQUIRED and os.path.exists(os.path.join(_lib.LIB_DIR, img)), img
    for m in ("denoise_capture", "denoise", "denoise_guide", "write_accum"):
        assert callable(getattr(rt.Renderer, m))


@pytest.mark.parametrize("passes,zs,ls", [(1, 0, 0), (3, 8, 6), (5, 23, 16), (5, 0, 0), (2, 23, 0)])
def test_constant_irradiance_returns_itself(passes, zs, ls):
    """whatever the guide says (random pids, depths and normals), weights only mix equal values"""
    rng = np.random.default_rng(3)
    g = scene()
    g["pid"] = rng.integers(0, 50, (H, W)).astype(np.int32)
    g["z"] = rng.integers(0, 1 << 24, (H, W)).astype(np.uint32)
    g["normal"] = rng.integers(-127, 128, (H, W, 3))
    s, n, A = (400, 200, 40), 4, (200, 100, 50)
    base = np.full((H, W), argb(0x80, *A), np.uint32)
    got = dr.denoise(records(H, W, s, n), base=base, passes=passes, zs=zs, ls=ls, **g)
    # d = 800, 400, 200: I = (102400 + 400) // 800 = 128, (51200 + 200) // 400 = 128, (10240 + 100) // 200 = 51
    I = [irr(c, n, a) for c, a in zip(s, A)]
    assert I == [128, 128, 51]
    # (128 * 200 + 128) >> 8 = 100, (128 * 100 + 128) >> 8 = 50, (51 * 50 + 128) >> 8 = 10
    want = argb(0x80, *[remod(i, a) for i, a in zip(I, A)])
    assert want == argb(0x80, 100, 50, 10)
    assert (got == want).all()


def test_one_bright_pixel_is_the_kernel():
    """a flat same-pid field, the irradiance stop off: every weight is 256, den = 256 * 256, and the
    response to one pixel of irradiance I0 is (h * I0 + 128) // 256 over the 5 x 5 footprint"""
    g = scene()
    I = np.zeros((H, W, 3), np.int64)
    cy, cx, I0 = 20, 24, (65280, 1000, 37)
    I[cy, cx] = I0
    out = dr.one_pass(I, g["pid"], g["z"], g["geom"], g["normal"], k=1, zs=0, ls=16)
    want = np.zeros_like(I)
    for j in range(-2, 3):
        for i in range(-2, 3):
            h = dr.B[i + 2] * dr.B[j + 2]
            want[cy + j, cx + i] = [(h * v + 128) // 256 for v in I0]
    assert want[cy, cx, 0] == 9180 and want[cy + 2, cx + 2, 0] == 255 and want[cy + 1, cx, 1] == 94
    assert np.array_equal(out, want)
    # and pass 3 puts the same footprint at stride 4
    out = dr.one_pass(I, g["pid"], g["z"], g["geom"], g["normal"], k=3, zs=0, ls=16)
    want4 = np.zeros_like(I)
    want4[cy - 8:cy + 9:4, cx - 8:cx + 9:4] = want[cy - 2:cy + 3, cx - 2:cx + 3]
    assert np.array_equal(out, want4)
    # with the irradiance stop on at ls = 0 the bright pixel's neighbours see a difference >= 9: untouched
    out = dr.one_pass(I, g["pid"], g["z"], g["geom"], g["normal"], k=1, zs=0, ls=0)
    assert np.array_equal(out[..., 0], I[..., 0])


def test_depth_gap_does_not_mix():
    """two half planes of different primitives, equal normals, a depth gap whose E is 0 in every pass:
    |dz| >> (zs + 4) >= 9 needs |dz| >= 9 << 12 at zs = 8"""
    g = scene()
    g["pid"][:, W // 2:] = 9
    g["z"][:, W // 2:] = 5000 + 40000
    rec = records(H, W, (100, 100, 100), 1)
    rec[:, W // 2:, :3] = 200
    base = np.full((H, W), argb(0xFF, 255, 255, 255), np.uint32)
    got = dr.denoise(rec, base=base, passes=5, zs=8, ls=16, **g)
    # I = (25600 + 127) // 255 = 100 and (51200 + 127) // 255 = 201; back: (100 * 255 + 128) >> 8 = 100,
    # (201 * 255 + 128) >> 8 = 200
    assert irr(100, 1, 255) == 100 and irr(200, 1, 255) == 201
    assert (got[:, :W // 2] == argb(0xFF, 100, 100, 100)).all()
    assert (got[:, W // 2:] == argb(0xFF, 200, 200, 200)).all()
    # the same planes one depth step apart mix across the edge (the stop is what held them apart)
    g["z"][:, W // 2:] = 5001
    mixed = dr.denoise(rec, base=base, passes=1, zs=8, ls=16, **g)
    assert (mixed[:, W // 2 - 1] & 0xFF).min() > 100 and (mixed[:, W // 2] & 0xFF).max() < 200


def test_normal_stop():
    """different primitives at one depth: perpendicular normals give c = 0, no mixing; equal unit normals
    give c = 16129 >> 6 = 252, wn = ((252 * 252) >> 8) ** 2 >> 8 = 240"""
    g = scene()
    g["pid"][:, W // 2:] = 9
    g["normal"][:, W // 2:] = (127, 0, 0)
    rec = records(H, W, (100, 100, 100), 1)
    rec[:, W // 2:, :3] = 200
    base = np.full((H, W), argb(0xFF, 255, 255, 255), np.uint32)
    got = dr.denoise(rec, base=base, passes=3, zs=0, ls=16, **g)
    assert (got[:, :W // 2] == argb(0xFF, 100, 100, 100)).all() and (got[:, W // 2:] == argb(0xFF, 200, 200, 200)).all()
    # one tap of another primitive with the same normal: weight 240 of 256
    g = scene(5, 5)
    g["pid"][2, 3] = 9
    I = np.zeros((5, 5, 3), np.int64)
    I[2, 3] = 25600
    out = dr.one_pass(I, g["pid"], g["z"], g["geom"], g["normal"], k=1, zs=0, ls=16)
    # at (2, 2): den = 256 * 256 - 24 * 256 + 24 * 240 = 65152, num = 24 * 240 * 25600
    assert out[2, 2, 0] == (24 * 240 * 25600 + 65152 // 2) // 65152 == 2263


def test_non_geometry_pixel_is_the_accumulation_resolve():
    g = scene()
    g["geom"][5:9, 5:9] = False
    rng = np.random.default_rng(5)
    n = 7
    rec = records(H, W, 0, n)
    rec[..., :3] = rng.integers(0, 255 * n + 1, (H, W, 3))
    base = rng.integers(0, 1 << 32, (H, W), dtype=np.uint64).astype(np.uint32)
    got = dr.denoise(rec, base=base, passes=4, zs=8, ls=6, **g)
    for y in range(5, 9):
        for x in range(5, 9):
            s = [int(v) for v in rec[y, x, :3]]
            want = (int(base[y, x]) & 0xFF000000) | ((2 * s[0] + n) // (2 * n)) << 16 | \
                ((2 * s[1] + n) // (2 * n)) << 8 | (2 * s[2] + n) // (2 * n)
            assert int(got[y, x]) == want == rt.accum_resolve(rec[y, x], int(base[y, x]))
    # and such pixels are no taps: their neighbours equal a run where the hole holds other values
    rec2 = rec.copy()
    rec2[5:9, 5:9, :3] = 0
    got2 = dr.denoise(rec2, base=base, passes=4, zs=8, ls=6, **g)
    keep = g["geom"]
    assert np.array_equal(got[keep], got2[keep])


def test_borders_renormalise():
    """a corner pixel of a flat field sees 3 x 3 of the 5 x 5 taps: den = 256 * (6 + 4 + 1) ** 2; a constant
    field stays constant, and a single bright corner keeps (36 * I0 + den / 2) // den of itself"""
    g = scene()
    I = np.zeros((H, W, 3), np.int64)
    I[0, 0] = 10000
    out = dr.one_pass(I, g["pid"], g["z"], g["geom"], g["normal"], k=1, zs=0, ls=16)
    den = 256 * 121
    assert out[0, 0, 0] == (36 * 256 * 10000 + den // 2) // den == 2975
    # its neighbour (0, 1) sees columns -1..3 minus one: b sums to 4 + 6 + 4 + 1 = 15 across, 11 down
    den = 256 * 15 * 11
    assert out[0, 1, 0] == (4 * 6 * 256 * 10000 + den // 2) // den == 1455
    # at stride 16 a pixel 10 from the left edge loses the taps at -32 and -16
    I = np.full((H, W, 3), 500, np.int64)
    I[20, 10 + 16] = 4596
    out = dr.one_pass(I, g["pid"], g["z"], g["geom"], g["normal"], k=5, zs=0, ls=16)
    # columns 0, +16, +32: b = 6 + 4 + 1; rows 4, 20, 36 (-12 and 52 lie outside): b = 4 + 6 + 4
    den = 256 * 11 * (4 + 6 + 4)
    num = 256 * (11 * 14 * 500 + 4 * 6 * (4596 - 500))
    assert out[20, 10, 0] == (num + den // 2) // den


@pytest.mark.parametrize("n", [1 << 24, 1])
@pytest.mark.parametrize("a", [0, 1, 255])
def test_extreme_records_do_not_overflow(n, a):
    """n = 2^24 with s = 255 n, base channels 0, 1 and 255: 256 s passes 2^40; the model's own check that
    every pass sum stays below 2^32 runs inside one_pass"""
    g = scene()
    rec = records(H, W, 255 * n, n)
    rec[::2, ::3, :3] = 0
    base = np.full((H, W), argb(0xFF, a, a, a), np.uint32)
    got = dr.denoise(rec, base=base, passes=5, zs=0, ls=16, **g)
    # a bright pixel's irradiance: (256 * 255 n + d // 2) // d with d = n * max(a, 1)
    I = irr(255 * n, n, a)
    assert I == {0: 65280, 1: 65280, 255: 256}[a]
    assert int(got.max() & 0xFF) <= remod(I, a) and int((got >> 24).min()) == 0xFF
    if a == 0:
        assert (got == 0xFF000000).all()
    # all bright: the field is constant
    got = dr.denoise(records(H, W, 255 * n, n), base=base, passes=5, zs=0, ls=0, **g)
    assert (got == argb(0xFF, *[remod(I, a)] * 3)).all()


def test_normal_restatement():
    """normals_f64 on two triangles: e1 x e2 normalised, times 127, rounded; a degenerate one is 0"""
    t = np.zeros((3, 12), np.float32)
    t[0, 4:7], t[0, 8:11] = (1, 0, 0), (0, 1, 0)          # +z
    t[1, 4:7], t[1, 8:11] = (0, 2, 0), (1, 0, 1)          # (2, 0, -2) / sqrt(8)
    t[2, 4:7], t[2, 8:11] = (1, 1, 1), (2, 2, 2)          # parallel edges
    pid = np.array([[0, 1, 2, 0]], np.int32)
    geom = np.array([[True, True, True, False]])
    N = dr.normals_f64(t, pid, geom)
    assert N.tolist() == [[[0, 0, 127], [90, 0, -90], [0, 0, 0], [0, 0, 0]]]
    assert dr.unpack_normal(np.uint32(90 | (0 << 8) | ((-90 & 0xFF) << 16))).tolist() == [90, 0, -90]
