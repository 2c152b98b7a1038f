"""GPU tests of ambient occlusion from the visibility records (vx_rt.h
rt_renderer_ao_begin / rt_render_ao_start / rt_render_ao_resolve_start; images
rt_ao -- kernels/rt_ao_kernel.hip -- and rt_ao_resolve,
kernels/rt_ao_resolve_kernel.hip).

The counts are held bit for bit to the definition composed from the untouched
oracle's primitives by brute force (tests/ao_reference.py, itself held to the
oracle's path tracer and a float64 model in tests/test_ao_cpu.py), to the
device's own path tracer, and per ray to the float64 model; the resolved frames
to rt.ao_resolve over the buffers read back.  No reference exists for this row."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ao_reference as ar  # noqa: E402
import rt_model_checks as mc  # noqa: E402
from conftest import scene_path  # noqa: E402
from test_ao_cpu import SEEDS, TOTALS, composition, oracle_records  # noqa: E402

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, rt  # noqa: E402

INF = float("inf")
SEED = SEEDS[0]
LIGHTS = [(0.0, 60.0, 80.0), (40.0, 10.0, 60.0), (-30.0, -20.0, 90.0)]
_state = {}


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def renderer(name="tekkaman", key=""):
    if (name, key) not in _state:
        s = rt.Scene.load(mc.scene_file(name))
        _state[(name, key)] = (s, rt.Renderer(s))
    return _state[(name, key)][1]


def same(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} pixels differ"


def session(r, W, H, radius=INF, seed=SEED, **kw):
    """configure, one record launch, begin"""
    r.configure(W, H, **kw)
    rec = r.aov()
    r.ao_begin(radius=radius, seed=seed)
    return rec


def counts(name, W, H, radius, S, seed=SEED):
    """the composition's occluded samples per pixel, uint32 [H, W]"""
    v, fv, _ = composition(name, W, H, seed, radius, S)
    return v.astype(np.uint32).sum(0), fv


# ---- the counts against the composition ----------------------------------------------------

CASES = [("tekkaman", 64, 64, 5, INF), ("tekkaman", 64, 64, 5, 8.0), ("tekkaman", 200, 136, 3, INF),
         ("interreflection", 32, 32, 64, INF), ("carnival", 32, 32, 4, INF), ("convex", 32, 32, 4, INF)]


@pytest.mark.parametrize("name,W,H,S,radius", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-S{c[3]}-r{c[4]}" for c in CASES])
def test_records_equal_the_composition(po, name, W, H, S, radius):
    r = renderer(name)
    rec = session(r, W, H, radius)
    _, pid, t = oracle_records(name, W, H)
    want, fv = counts(name, W, H, radius, S)
    # the device's records are the oracle's: the composition starts from the same pixels
    rays = ((rec["depth_flags"] & rt.RT_AOV_GEOM) != 0) & (rec["t"] > 0) & np.isfinite(rec["t"])
    same(rays, fv["rays"])
    assert np.array_equal(rec["t"][rays].view(np.uint32), np.asarray(t, np.float32)[rays].view(np.uint32))
    assert r.ao_samples() == 0
    r.ao(S)
    got = r.ao_records()
    print(f"{name} {W}x{H} S={S} radius {radius}: {int(rays.sum())} ray pixels, {int(got.sum())} occluded "
          f"of {S * int(rays.sum())} rays")
    same(got, want)
    assert not got[~rays].any()
    assert r.ao_samples() == S
    if name in ("carnival", "convex"):
        assert not got.any()
    else:
        assert got.any()


@pytest.mark.parametrize("variant", ["ao_w1", "ao_w4", "ao_packet"])
def test_variant_images_count_the_same(po, variant):
    """the A/B images of scripts/bench_ao.py (lib/variants: one and four waves per block, the packet walk)
    against the same composition: a single round, several rounds, a radius"""
    name, W, H = "tekkaman", 64, 64
    vdir = os.path.join(_lib.LIB_DIR, "variants", variant)
    assert os.path.isfile(os.path.join(vdir, "rt_ao.vxbin"))
    s = rt.Scene.load(mc.scene_file(name))
    r = rt.Renderer(s, kernel_dir=vdir)
    for S, radius in ((1, INF), (5, INF), (5, 8.0)):
        session(r, W, H, radius)
        r.ao(S)
        same(r.ao_records(), counts(name, W, H, radius, S)[0])
    r.close()
    s.close()


def test_accumulation(po):
    name, W, H = "tekkaman", 64, 64
    r = renderer(name)
    session(r, W, H)
    want8, _ = counts(name, W, H, INF, 8)
    for _ in range(2):
        r.ao(3)
        r.ao(5, wait=False)
        assert r.ao_samples() == 8
        same(r.ao_records(), want8)
        r.ao_reset()
        assert r.ao_samples() == 0
    r.ao(8)
    same(r.ao_records(), want8)
    # single samples, differenced: the per-sample totals
    for radius in (INF, 8.0, 2.0):
        r.ao_begin(radius=radius, seed=SEED)
        prev, totals = np.zeros((H, W), np.uint32), []
        for _ in SEEDS:
            r.ao(1)
            cur = r.ao_records()
            assert ((cur - prev) <= 1).all() and (cur >= prev).all()
            totals.append(int((cur - prev).sum()))
            prev = cur
        print(f"tekkaman 64x64 radius {radius}: occluded per sample {totals}")
        assert tuple(totals) == TOTALS[(name, W, H, radius)][0]


@pytest.mark.parametrize("name,W,H,radius", [("interreflection", 32, 32, INF), ("interreflection", 32, 32, 8.0),
                                             ("shadow_edge", 32, 32, INF), ("convex", 32, 32, INF)])
def test_per_sample_totals_and_the_float64_model(po, name, W, H, radius):
    """the verdicts of single rays -- the differences between 1-sample launches -- against the table of
    tests/test_ao_cpu.py and, ray by ray, the float64 model (same cases and caps as on the CPU)"""
    r = renderer(name)
    session(r, W, H, radius)
    _, model = mc.model(name, W, H)
    _, fv, dirs = composition(name, W, H, SEED, radius, len(SEEDS))
    prev, totals, undecided, bad = np.zeros((H, W), np.uint32), [], 0, 0
    for j in range(len(SEEDS)):
        r.ao(1)
        cur = r.ao_records()
        got = (cur - prev).reshape(-1)[fv["idx"]]
        assert (got <= 1).all()
        totals.append(int(got.sum()))
        prev = cur
        if name != "convex":
            occ, robust = ar.model_verdict(model, fv["P"], dirs[j], fv["tri"], radius)
            undecided += int((~robust).sum())
            bad += int((got.astype(bool) != occ)[robust].sum())
    n = len(SEEDS) * len(fv["idx"])
    print(f"{name} radius {radius}: per sample {totals}; {undecided} of {n} rays undecided, {bad} robust verdicts differ")
    assert tuple(totals) == TOTALS[(name, W, H, radius)][0]
    assert bad == 0
    assert undecided <= mc.AMBIGUOUS_CAP * n


@pytest.mark.parametrize("name,W,H,seed", [("interreflection", 32, 32, 1000), ("interreflection", 32, 32, 7),
                                           ("tekkaman", 64, 64, 1000)])
def test_identity_on_the_devices_path_tracer(po, name, W, H, seed):
    """radius inf, one sample: the occluded rays are the one-bounce path frame's bounce rays that hit,
    each of which costs that frame one more shadow ray"""
    r = renderer(name)
    session(r, W, H, INF, seed)
    r.ao(1)
    total = int(r.ao_records().sum())
    r.configure(W, H, path=True, bounces=1, seed=seed)
    r.render()
    st = r.stats()
    print(f"{name} seed {seed}: {total} occluded; path frame shadow {st['shadow_rays']} bounce {st['bounce_rays']}")
    assert total == st["shadow_rays"] - st["bounce_rays"]
    assert total > 0


# ---- what the counts do not depend on ---------------------------------------------------------

def test_independence(po):
    name, W, H, S = "tekkaman", 64, 64, 5
    want, _ = counts(name, W, H, INF, S)
    r = renderer(name)
    r.configure(W, H, shadows=True, light=LIGHTS[0])
    r.render()
    frame = r.framebuffer().copy()
    rec = r.aov().copy()
    r.ao_begin(radius=INF, seed=SEED)
    r.ao(S)
    same(r.ao_records(), want)
    same(r.framebuffer(), frame)                                # ao() writes no framebuffer
    assert np.array_equal(r.aov_records().view(np.uint32), rec.view(np.uint32))   # and no record
    # the light: the session goes on, the counts are the same
    r.set_light(LIGHTS[1])
    r.ao_reset()
    r.ao(S)
    same(r.ao_records(), want)
    r.set_lights(LIGHTS)
    r.ao_reset()
    r.ao(S)
    same(r.ao_records(), want)
    assert r.ao_samples() == S
    for kw in (dict(shadows=False), dict(bvh_walk=True), dict(host_setup=True)):
        session(r, W, H, INF, **kw)
        r.ao(S)
        same(r.ao_records(), want)


def test_counters(po):
    name, W, H, S = "tekkaman", 64, 64, 5
    want, fv = counts(name, W, H, INF, S)
    r = renderer(name)
    session(r, W, H, counters=True)
    r.ao(S)
    st = r.stats()
    assert st["shadow_rays"] == S * len(fv["idx"])
    assert st["occluded"] == int(want.sum()) == int(r.ao_records().sum())
    assert st["primary_rays"] == 0 and st["geometry_hits"] == 0 and st["bounce_rays"] == 0
    assert r.kernel_ms() > 0


# ---- the resolve ------------------------------------------------------------------------------

def test_resolve(po):
    name, W, H, S = "tekkaman", 64, 64, 8
    want, _ = counts(name, W, H, 8.0, S)
    r = renderer(name)
    r.configure(W, H, shadows=True, light=LIGHTS[0])
    r.set_lights(LIGHTS)
    r.relight_capture()
    r.ao_begin(radius=8.0, seed=SEED)
    r.ao(S)
    o = r.ao_records()
    same(o, want)
    base, rec = r.relight_base(), r.aov_records()
    r.ao_resolve("grey")
    assert r.kernel_ms() > 0
    grey = r.framebuffer().copy()
    same(grey, rt.ao_resolve(np.full((H, W), 0xFFFFFFFF, np.uint32), o, S))
    assert len(np.unique(grey)) > 2
    for weights in ([1, 1, 1], [255, 64, 1]):
        r.ao_resolve("modulate", weights)
        lit = rt.relight_resolve(base, rec["depth_flags"], rec["light_mask"], weights)
        got = r.framebuffer().copy()
        same(got, rt.ao_resolve(lit, o, S))
        assert int((got != lit).sum()) >= 50, "the ambient term changes too few pixels to show"
    r.ao_resolve("modulate", None, wait=False)
    r.wait()
    same(r.framebuffer(), rt.ao_resolve(base, o, S))
    # more samples, another N: the resolve follows the cursor
    r.ao(3)
    r.ao_resolve("grey")
    same(r.framebuffer(), rt.ao_resolve(np.full((H, W), 0xFFFFFFFF, np.uint32), r.ao_records(), S + 3))
    # one light, frames in between: into the framebuffer in use
    r.configure(W, H, shadows=True, light=LIGHTS[1], counters=False)
    r.relight_capture()
    r.ao_begin(radius=8.0, seed=SEED)
    r.start()
    r.ao(S, wait=False)
    r.start()
    r.ao_resolve("modulate", [9], wait=False)
    r.wait()
    rec = r.aov_records()
    same(r.framebuffer(), rt.ao_resolve(rt.relight_resolve(r.relight_base(), rec["depth_flags"], rec["light_mask"], [9]),
                                        want, S))


# ---- refusals -----------------------------------------------------------------------------------

def _refused(fn, *a, **kw):
    with pytest.raises(rt.RtError, match=r"\(-2\): \S+"):
        fn(*a, **kw)


@pytest.mark.parametrize("kw", [dict(path=True), dict(flat=True), dict(raster=True, shadows=False),
                                dict(instrumented=True), dict(compact=True), dict(shard_index=0, shard_count=2),
                                dict(bvh_width=2)],
                         ids=["path", "flat", "raster", "instrumented", "compact", "shards", "deep-tree"])
def test_begin_refused(po, kw):
    # (a renderer of its own, the deep tree last: one that ran the generic images keeps them)
    r = renderer(key="/refusals")
    r.configure(64, 64, **dict(dict(shadows=True), **kw))
    if "compact" in kw or "shard_count" in kw:
        r.aov()                                                  # records exist: the layout is what is refused
    _refused(r.ao_begin)
    _refused(r.ao, 1)
    _refused(r.ao_resolve, "grey")
    _refused(r.ao_samples)
    r.render()                                                   # the renderer still renders its frame


def test_refused_ordered_tail(po):
    sv = rt.Scene.load(scene_path("vase"), om_layers=True)
    assert sv.om_split()[1] > 0
    ro = rt.Renderer(sv)
    ro.configure(64, 64, shadows=True)
    _refused(ro.ao_begin)
    _refused(ro.ao, 1)
    ro.close()
    sv.close()


def test_state(po):
    W = H = 32
    s = rt.Scene.load(mc.scene_file("convex"))
    r = rt.Renderer(s)
    with pytest.raises(rt.RtError):
        r.ao_begin()                                             # before any configure
    r.configure(W, H, shadows=True)
    _refused(r.ao_begin)                                         # no record launch since the configure
    _refused(r.ao, 1)
    _refused(r.ao_reset)
    _refused(r.ao_records)
    r.aov()
    for radius in (0.0, -1.0, float("nan"), float("-inf")):
        _refused(r.ao_begin, radius=radius)
    _refused(r.ao, 1)                                            # the refused begins began nothing
    r.ao_begin(radius=0.5)
    _refused(r.ao_resolve, "grey")                               # N = 0
    _refused(r.ao_resolve, "modulate")
    _refused(r.ao_records)
    for k in (0, 65, 1 << 20):
        _refused(r.ao, k)
        _refused(r.ao, k, wait=False)
    assert r.ao_samples() == 0
    r.ao(1)
    with pytest.raises(rt.RtError):
        r.ao_resolve("gray")
    _refused(r.ao_resolve, "modulate")                           # no relight capture
    _refused(r.ao_resolve, "modulate", [1])
    r.ao_resolve("grey")
    r.relight_capture()                                          # (a record launch: the session goes on)
    r.ao_resolve("modulate", [1])
    _refused(r.ao_resolve, "modulate", [1, 1])                   # a wrong n
    _refused(r.ao_resolve, "modulate", [0])                      # every weight 0
    r.set_light((10.0, 20.0, 70.0))                              # ends the capture, not the session
    _refused(r.ao_resolve, "modulate", [1])
    _refused(r.ao_resolve, "modulate")
    r.ao(2)
    assert r.ao_samples() == 3
    r.ao_resolve("grey")
    # the cursor's cap: 65535 samples
    r.ao_reset()
    for _ in range(1023):
        r.ao(64, wait=False)
    assert r.ao_samples() == 65472
    _refused(r.ao, 64)
    r.ao(63)
    assert r.ao_samples() == 65535
    _refused(r.ao, 1)
    assert not r.ao_records().any()                              # convex: no ray of 65535 is occluded
    r.ao_resolve("grey")
    same(r.framebuffer(), np.full((H, W), 0xFFFFFFFF, np.uint32))
    r.configure(W, H, shadows=True)                              # ends the session
    _refused(r.ao, 1)
    _refused(r.ao_resolve, "grey")
    r.close()
    s.close()


# ---- the CLI --------------------------------------------------------------------------------------

def test_rtapp_ambient_occlusion(po, tmp_path):
    from PIL import Image
    W = H = 64
    out = tmp_path / "out.png"
    p = subprocess.run([os.path.join(_lib.LIB_DIR, "rtapp"), "-t", scene_path("tekkaman"), "-S", "-K8,8", "-w64", "-h64",
                        "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "AO: 8 samples, radius 8" in p.stdout, p.stdout
    got = np.array(Image.open(out).convert("RGBA"))
    # the same frame composed here: the relit frame under a unit weight times the composition's term
    o, _ = counts("tekkaman", W, H, 8.0, 8, seed=rt.AO_SEED)
    r = renderer("tekkaman")
    r.configure(W, H, shadows=True)
    r.relight_capture()
    rec = r.aov_records()
    want = rt.ao_resolve(rt.relight_resolve(r.relight_base(), rec["depth_flags"], rec["light_mask"], [1]), o, 8)
    assert po.compare_images(got, po.argb_to_rgba_image(want), tol=0) == 0
    r.render()
    assert int((want != r.framebuffer()).sum()) >= 50, "the ambient term changes too few pixels to show"
    bad = subprocess.run([os.path.join(_lib.LIB_DIR, "rtapp"), "-t", scene_path("tekkaman"), "-K8", "-o", "null"],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "Error: -K" in bad.stdout and "AO:" not in bad.stdout, bad.stdout
