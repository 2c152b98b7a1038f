"""Soft shadows without a GPU: the resolve formula of include/vx_rt.h, the
definition composed from the oracle's primitives (tests/soft_reference.py)
against the oracle's own hard shadows at radius 0, against the float64 model's
verdict on the same rays, against what a penumbra means, and against known
totals."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ao_reference as ar  # noqa: E402
import rt_model_checks as mc  # noqa: E402
import soft_reference as sr  # noqa: E402
from test_ao_cpu import oracle_records  # noqa: E402

SEED = 1000
NS = 4   # samples of the totals' table: seeds 1000..1003
# sixteen lights above and around the scenes, for the packed table's last light
LIGHTS16 = [(-60.0 + 8.0 * i, 60.0 - 5.0 * i, 80.0 + 5.0 * (i % 3)) for i in range(16)]
RADII16 = [0.5 * i for i in range(16)]
CASES = {
    "shadow_edge": ("shadow_edge", 32, 32, [mc.LIGHT], [4.0]),
    "interreflection": ("interreflection", 32, 32, mc.PATH_LIGHTS, [0.0, 4.0]),
    "tekkaman": ("tekkaman", 64, 64, mc.TEKKAMAN_LIGHTS, [2.0, 4.0, 8.0]),
    "tekkaman-edge": ("tekkaman", 200, 136, [mc.LIGHT], [4.0]),
    "tekkaman-16": ("tekkaman", 16, 16, LIGHTS16, RADII16),
    "convex": ("convex", 32, 32, [mc.LIGHT], [4.0]),
    "carnival": ("carnival", 32, 32, [mc.LIGHT], [4.0]),
}
# case -> per light the occluded rays of seeds 1000..1003, and the ray pixels: the composition, measured on the
# CPU (convex is a known answer: a convex object shadows none of its own points; carnival has no occluder)
TOTALS = {
    "shadow_edge": (((175, 179, 179, 177),), 928),
    "interreflection": (((170, 170, 170, 170), (170, 155, 158, 160)), 332),
    "tekkaman": (((130, 136, 132, 133), (105, 95, 104, 99), (223, 216, 223, 223)), 417),
    "convex": (((0, 0, 0, 0),), 306),
    "carnival": (((0, 0, 0, 0),), None),
}


def composition(case, S, seed=SEED, radii=None):
    """(verdicts uint8[n, S, H, W], fv, dirs) of a case, once per process"""
    name, W, H, lights, rad = CASES[case]
    sc, pid, t = oracle_records(name, W, H)
    return sr.cached_verdicts(name, sc, W, H, lights, rad if radii is None else radii, seed, S, pid, t)


def formula(base, geom, counts, N, weights):
    """the resolve in numpy uint64"""
    w = np.asarray(weights, np.uint64)
    o = np.minimum(np.asarray(counts, np.uint64), np.uint64(N))
    D = np.uint64(N) * w.sum(dtype=np.uint64)
    O = (w.reshape((-1,) + (1,) * (o.ndim - 1)) * o).sum(0, dtype=np.uint64)
    base = np.asarray(base, np.uint32)
    out = base & np.uint32(0xFF000000)
    for sh in (16, 8, 0):
        c = ((base >> sh) & 0xFF).astype(np.uint64)
        out = out | (((2 * ((D - O) * c + O * (c >> np.uint64(1))) + D) // (2 * D)).astype(np.uint32) << sh)
    return np.where(geom, out, base)


def test_fmaf_vec_is_the_single_rounding():
    """soft_reference.fmaf_vec against the rational fmaf: random operands, and sums built to fall exactly
    on, just above and just below the midpoint of two float32 values"""
    rng = np.random.default_rng(7)
    a = (rng.standard_normal(2000) * 50).astype(np.float32)
    b = rng.standard_normal(2000).astype(np.float32)
    c = (rng.standard_normal(2000) * 80).astype(np.float32)
    # beside c = 1 + j * 2^-23 (quantum 2^-23): a * b = 2^-24 puts the sum exactly on a midpoint; a * b =
    # 2^-24 * (1 + 2^-23) * (1 - 2^-23) = 2^-24 - 2^-70 puts it below one by less than float64 resolves,
    # where rounding the float64 sum again would go to even instead of down (above, with a negated)
    j = rng.integers(0, 1 << 22, 600)
    near = (np.arange(600) % 2).astype(bool)
    ta = np.where(near, 2.0 ** -24 * (1.0 + 2.0 ** -23), 2.0 ** -24).astype(np.float32)
    tb = np.where(near, 1.0 - 2.0 ** -23, 1.0).astype(np.float32)
    tc = (1.0 + j.astype(np.float64) * 2.0 ** -23).astype(np.float32)
    a, b, c = np.concatenate([a, ta, -ta]), np.concatenate([b, tb, tb]), np.concatenate([c, tc, tc])
    got = sr.fmaf_vec(a, b, c)
    want = np.array([sr.fmaf(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    ties = sum(1 for x, y, z in zip(ta, tb, tc) if (Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)))
               * 2 ** 23 % 1 == Fraction(1, 2))
    print(f"{len(a)} operands, {ties} exact ties among them")
    assert ties == 300
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("N", [1, 2, 3, 7, 64, 1024])
def test_resolve_is_the_formula(N, n):
    from skybox_rt_amd import rt
    rng = np.random.default_rng(N * 31 + n)
    c = np.arange(256, dtype=np.uint32)
    base = (np.uint32(0x5A) << 24) | (c << 16) | ((255 - c) << 8) | ((c * 7) & 0xFF)
    geom = np.full(256, rt.RT_AOV_GEOM | 0x1234, np.uint32)
    levels = sorted({0, 1, N // 2, max(N - 1, 0), N, N + 1, 2000})
    wsets = [np.full(n, 255), np.ones(n, np.int64), rng.integers(0, 256, n), np.eye(1, n, n - 1, dtype=np.int64)[0] * 9]
    for w in wsets:
        if w.sum() == 0:
            w[0] = 1
        for o in levels:
            counts = np.full((n, 256), o, np.uint16)
            assert np.array_equal(rt.soft_resolve(base, geom, counts, N, w), formula(base, True, counts, N, w)), (N, n, o)
        # every light at a level of its own
        counts = np.array([[levels[(i + s) % len(levels)] for s in range(256)] for i in range(n)], np.uint16)
        got = rt.soft_resolve(base, geom, counts, N, w)
        assert np.array_equal(got, formula(base, True, counts, N, w)), (N, n)
        assert rt.soft_resolve(int(base[200]), int(geom[200]), counts[:, 200], N, w) == int(got[200])
        # counts at 0 or N: the relight resolve of the mask of the lights at N
        bits = rng.integers(0, 1 << n, 256).astype(np.uint32)
        counts = np.array([np.where((bits >> i) & 1, N, 0) for i in range(n)], np.uint16)
        flags = np.full(256, rt.RT_AOV_GEOM | rt.RT_AOV_SHADOW_RAY, np.uint32)
        assert np.array_equal(rt.soft_resolve(base, flags, counts, N, w), rt.relight_resolve(base, flags, bits, w))
    # a pixel that is not a geometry pixel is its base colour
    counts = np.full((n, 256), N, np.uint16)
    assert np.array_equal(rt.soft_resolve(base, np.zeros(256, np.uint32), counts, N, np.ones(n, np.int64)), base)


def test_resolve_bound_and_degenerate_returns():
    from skybox_rt_amd import rt
    L = rt.lib()
    # the 32-bit bound: N = 1024, sixteen lights at weight 255, white
    N, n = 1024, 16
    w = np.full(n, 255, np.uint8)
    for o in (0, 1, 511, 512, 1023, 1024):
        counts = np.full(n, o, np.uint16)
        assert rt.soft_resolve(0xFFFFFFFF, rt.RT_AOV_GEOM, counts, N, w) == int(formula(0xFFFFFFFF, True, counts, N, w))
    assert 511 * N * int(w.sum()) < 1 << 32
    assert rt.soft_resolve(0xFFFFFFFF, rt.RT_AOV_GEOM, np.full(n, N, np.uint16), N, w) == 0xFF7F7F7F
    # unchanged: N = 0, n outside 1..16, every weight 0
    c17, w17 = np.full(17, 5, np.uint16), np.ones(17, np.uint8)
    g = rt.RT_AOV_GEOM
    assert L.rt_soft_resolve(0x12345678, g, c17.ctypes.data, 0, w17.ctypes.data, 3) == 0x12345678
    assert L.rt_soft_resolve(0x12345678, g, c17.ctypes.data, 8, w17.ctypes.data, 0) == 0x12345678
    assert L.rt_soft_resolve(0x12345678, g, c17.ctypes.data, 8, w17.ctypes.data, 17) == 0x12345678
    z = np.zeros(3, np.uint8)
    assert L.rt_soft_resolve(0x12345678, g, c17.ctypes.data, 8, z.ctypes.data, 3) == 0x12345678
    assert L.rt_soft_resolve(0x12345678, g, c17.ctypes.data, 8, w17.ctypes.data, 3) != 0x12345678


@pytest.mark.parametrize("name,W,H,lights", [("shadow_edge", 32, 32, [mc.LIGHT]),
                                             ("interreflection", 32, 32, mc.PATH_LIGHTS),
                                             ("tekkaman", 64, 64, mc.TEKKAMAN_LIGHTS)])
def test_radius_zero_is_the_oracles_hard_shadow(oracle_lib, name, W, H, lights):
    """the anchor: at R = 0 every sample's verdict for light i is the oracle's shadowed frame under that
    light -- its occluded counter, and its shadowed pixels (the pixels the shadow darkens)"""
    from oracle import py_oracle as po
    sc, pid, t = oracle_records(name, W, H)
    v = sr.verdicts(sc, W, H, lights, [0.0] * len(lights), SEED, 2, pid, t)
    plain, _, _, _ = po.rt_render(po.OracleScene(sc), po.rt_params(W, H, shadows=False))
    for i, light in enumerate(lights):
        lit, _, _, k = po.rt_render(po.OracleScene(sc), po.rt_params(W, H, shadows=True, light=light, shadow_lists=False))
        assert np.array_equal(v[i, 0], v[i, 1])
        occ = v[i, 0].astype(bool)
        print(f"{name} light {i}: {int(occ.sum())} occluded, oracle {k['occluded']} of {k['shadow_rays']}")
        assert int(occ.sum()) == k["occluded"]
        dark = (np.asarray(lit).reshape(H, W) != np.asarray(plain).reshape(H, W))
        assert not (dark & ~occ).any()
        # (a shadow halves every channel: it shows wherever the unshadowed pixel is not black)
        shows = (np.asarray(plain).reshape(H, W) & 0xFFFFFF) != 0
        assert np.array_equal(dark, occ & shows)
        assert dark.any()


@pytest.mark.parametrize("case", ["shadow_edge", "interreflection"])
def test_composition_against_the_float64_model(oracle_lib, case):
    name, W, H, lights, radii = CASES[case]
    assert max(radii) > 0
    _, model = mc.model(name, W, H)
    v, fv, dirs = composition(case, NS)
    undecided = bad = n = 0
    for i in range(len(lights)):
        for j in range(NS):
            occ, robust = ar.model_verdict(model, fv["P"], dirs[i][j], fv["tri"], radius=1.0)
            got = v[i, j].reshape(-1)[fv["idx"]].astype(bool)
            undecided += int((~robust).sum())
            bad += int((got != occ)[robust].sum())
            n += len(got)
    print(f"{case} radii {radii}: {undecided} of {n} rays undecided ({100.0 * undecided / n:.2f} %), "
          f"{bad} robust verdicts differ")
    assert bad == 0
    assert undecided <= mc.AMBIGUOUS_CAP * n


def test_meaning(oracle_lib):
    """a penumbra: with a radius some pixels of shadow_edge see part of the light, without none does; a
    convex object and a scene without an occluder shadow nothing"""
    S = 16
    o = composition("shadow_edge", S)[0].astype(np.uint32).sum(1)[0]
    partial = int(((o > 0) & (o < S)).sum())
    print(f"shadow_edge R = 4: {partial} pixels with 0 < o < {S}, {int((o == S).sum())} in full shadow")
    assert partial > 0 and (o == S).any()
    o0 = composition("shadow_edge", S, radii=[0.0])[0].astype(np.uint32).sum(1)[0]
    assert not ((o0 > 0) & (o0 < S)).any() and (o0 == S).any()
    for case in ("convex", "carnival"):
        assert not composition(case, S)[0].any()


@pytest.mark.parametrize("case", sorted(TOTALS))
def test_composition_totals(oracle_lib, case):
    totals, npix = TOTALS[case]
    v, fv, _ = composition(case, NS)
    got = tuple(tuple(int(x) for x in row) for row in v.reshape(v.shape[0], NS, -1).sum(2))
    print(f"{case}: occluded per light and sample {got}, {len(fv['idx'])} ray pixels")
    assert got == totals
    if npix is not None:
        assert len(fv["idx"]) == npix
    assert not v[:, :, ~fv["rays"]].any()
