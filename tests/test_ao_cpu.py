"""Ambient occlusion without a GPU: the resolve formula of include/vx_rt.h, the
definition composed from the oracle's primitives (tests/ao_reference.py)
against the oracle's own path tracer and against known totals, and the float64
model's verdict on the same rays."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ao_reference as ar  # noqa: E402
import rt_model_checks as mc  # noqa: E402

INF = float("inf")
SEEDS = (1000, 1001, 1002, 1003)
# (scene, W, H, radius) -> occluded rays of seeds 1000..1003 and the ray pixels: the composition,
# measured on the CPU (convex is a known answer: a convex object occludes none of its own rays)
TOTALS = {
    ("interreflection", 32, 32, INF): ((83, 86, 99, 71), 332),
    ("interreflection", 32, 32, 8.0): ((30, 26, 34, 22), 332),
    ("shadow_edge", 32, 32, INF): ((220, 229, 233, 203), 928),
    ("convex", 32, 32, INF): ((0, 0, 0, 0), 306),
    ("carnival", 32, 32, INF): ((0, 0, 0, 0), None),
    ("tekkaman", 64, 64, INF): ((38, 38, 45, 43), 417),
    ("tekkaman", 64, 64, 8.0): ((26, 22, 25, 26), 417),
    ("tekkaman", 64, 64, 2.0): ((11, 9, 8, 12), 417),
}


def oracle_records(name, W, H):
    """(scene, oracle pid, t [H, W]) of the unshadowed frame, once per process"""
    from oracle import py_oracle as po
    key = ("records", name, W, H)
    if key not in ar._cache:
        sc, _ = mc.model(name, W, H)
        _, pid, t, _ = po.rt_render(po.OracleScene(sc), po.rt_params(W, H, shadows=False))
        ar._cache[key] = (sc, pid, t)
    return ar._cache[key]


def composition(name, W, H, seed, radius, S):
    sc, pid, t = oracle_records(name, W, H)
    return ar.cached_verdicts(name, sc, W, H, seed, radius, S, pid, t)


@pytest.mark.parametrize("N", [1, 2, 3, 7, 64, 255, 65535])
def test_resolve_is_the_formula(N):
    from skybox_rt_amd import rt
    c = np.arange(256, dtype=np.uint32)
    for o in sorted({0, 1, N // 2, N - 1, N}):
        if o > N:
            continue
        argb = (np.uint32(0x5A) << 24) | (c << 16) | ((255 - c) << 8) | ((c * 7) & 0xFF)
        got = rt.ao_resolve(argb, np.uint32(o), N)
        want = argb & np.uint32(0xFF000000)
        for sh in (16, 8, 0):
            ch = ((argb >> sh) & 0xFF).astype(np.uint64)
            want = want | (((2 * ch * (N - o) + N) // (2 * N)).astype(np.uint32) << sh)
        assert np.array_equal(got, want), (N, o)
        assert rt.ao_resolve(int(argb[200]), o, N) == int(want[200])
    assert rt.ao_resolve(0x12345678, 5, 0) == 0x12345678  # N = 0: the pixel itself
    assert rt.ao_resolve(0xFFFFFFFF, 0, N) == 0xFFFFFFFF and rt.ao_resolve(0xFFFFFFFF, N, N) == 0xFF000000


@pytest.mark.parametrize("case", sorted(TOTALS, key=str), ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-r{c[3]}")
def test_composition_totals(oracle_lib, case):
    name, W, H, radius = case
    totals, npix = TOTALS[case]
    v, fv, _ = composition(name, W, H, SEEDS[0], radius, len(SEEDS))
    got = tuple(int(x) for x in v.reshape(len(SEEDS), -1).sum(1))
    print(f"{case}: occluded per sample {got}, {len(fv['idx'])} ray pixels")
    assert got == totals
    if npix is not None:
        assert len(fv["idx"]) == npix
    assert not v[:, ~fv["rays"]].any()


@pytest.mark.parametrize("name,W,H,seeds", [("interreflection", 32, 32, (1000, 7)), ("tekkaman", 64, 64, (1000,)),
                                            ("carnival", 32, 32, (1000,))])
def test_composition_is_the_oracle_path_tracers_first_bounce(oracle_lib, name, W, H, seeds):
    """at radius inf the occluded rays of sample seed s are the one-bounce path frame's bounce rays
    that hit: every path traces a shadow ray at its first vertex and one more where the bounce hit"""
    from oracle import py_oracle as po
    sc, pid, t = oracle_records(name, W, H)
    for s in seeds:
        v = ar.verdicts(sc, W, H, s, INF, 1, pid, t)
        _, _, _, k = po.rt_render(po.OracleScene(sc), po.rt_params(W, H, shadows=False, path=True, bounces=1, seed=s,
                                                                   shadow_lists=False))
        print(f"{name} seed {s}: {int(v.sum())} occluded, oracle shadow {k['shadow_rays']} bounce {k['bounce_rays']}")
        assert int(v.sum()) == k["shadow_rays"] - k["bounce_rays"]


@pytest.mark.parametrize("name,radius", [("interreflection", INF), ("shadow_edge", INF), ("interreflection", 8.0)])
def test_composition_against_the_float64_model(oracle_lib, name, radius):
    W = H = 32
    _, model = mc.model(name, W, H)
    v, fv, dirs = composition(name, W, H, SEEDS[0], radius, len(SEEDS))
    undecided = bad = 0
    for j in range(len(SEEDS)):
        occ, robust = ar.model_verdict(model, fv["P"], dirs[j], fv["tri"], radius)
        got = v[j].reshape(-1)[fv["idx"]].astype(bool)
        undecided += int((~robust).sum())
        bad += int((got != occ)[robust].sum())
    n = len(SEEDS) * len(fv["idx"])
    print(f"{name} radius {radius}: {undecided} of {n} rays undecided, {bad} robust verdicts differ")
    assert bad == 0
    assert undecided <= mc.AMBIGUOUS_CAP * n


def test_kernel_divisions_are_exact(tmp_path):
    """the resolve launch's reciprocal form (rt_common.h rt_ao_quot, rt_ao_mix, rt_ao_relight_mix) against
    integer division and rt_relight_mix: every N, every W, every channel value (tests/ao_quot_check.cpp)"""
    import shutil
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    exe = os.path.join(str(tmp_path), "ao_quot_check")
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    p = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I",
                        os.path.join(here, "..", "skybox_rt_amd", "csrc", "kernels"), "-o", exe,
                        os.path.join(here, "ao_quot_check.cpp")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and " 0 failure(s)" in r.stdout, r.stdout + r.stderr
