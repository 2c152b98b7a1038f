"""GPU tests of soft shadows from the visibility records (vx_rt.h
rt_renderer_soft_begin / rt_render_soft_start / rt_render_soft_resolve_start;
images rt_soft -- kernels/rt_soft_kernel.hip -- and rt_soft_resolve,
kernels/rt_soft_resolve_kernel.hip).

The counts are held bit for bit to the definition composed from the untouched
oracle's primitives by brute force (tests/soft_reference.py, itself held to the
oracle's hard shadows and a float64 model in tests/test_soft_cpu.py) and, at
radius 0, to the device's own hard shadows: the records' light masks, the
relight frame and the set_lights frame; the resolved frames to rt.soft_resolve
over the buffers read back.  No reference exists for this row."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rt_model_checks as mc  # noqa: E402
from conftest import scene_path  # noqa: E402
from test_soft_cpu import CASES, NS, SEED, TOTALS, composition  # noqa: E402

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, rt  # noqa: E402

VARIANTS = ["soft_w1", "soft_w2", "soft_w4", "soft_lmajor", "soft_packet", "soft_packet_lmajor_w1",
            "soft_packet_lmajor_w2"]
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
    assert np.array_equal(got, want), f"{int((got != want).sum())} entries differ"


def lit(r, W, H, lights, **kw):
    """configure under the lights"""
    r.configure(W, H, **dict(dict(shadows=True, light=lights[0]), **kw))
    if len(lights) > 1:
        r.set_lights(lights)


def session(r, case, radii=None, seed=SEED, capture=False, **kw):
    """configure under the case's lights, one record launch, begin -> the records"""
    _, W, H, lights, rad = CASES[case]
    lit(r, W, H, lights, **kw)
    if capture:
        r.relight_capture()
        rec = r.aov_records()
    else:
        rec = r.aov()
    r.soft_begin(rad if radii is None else radii, seed=seed)
    return rec


def counts(case, S, seed=SEED, radii=None):
    """the composition's occluded samples per light and pixel, uint16 [n, H, W]"""
    v, fv, _ = composition(case, S, seed, radii)
    return v.astype(np.uint16).sum(1, dtype=np.uint16), fv


def ray_pixels(rec):
    return ((rec["depth_flags"] & rt.RT_AOV_GEOM) != 0) & (rec["t"] > 0) & np.isfinite(rec["t"])


# ---- the counts against the composition ----------------------------------------------------

RECORD_CASES = [("shadow_edge", 5), ("interreflection", 64), ("tekkaman", 5), ("tekkaman-edge", 3), ("tekkaman-16", 2),
                ("carnival", 4)]


@pytest.mark.parametrize("case,S", RECORD_CASES, ids=[f"{c}-S{s}" for c, s in RECORD_CASES])
def test_records_equal_the_composition(po, case, S):
    name, W, H, lights, radii = CASES[case]
    r = renderer(name)
    rec = session(r, case)
    want, fv = counts(case, S)
    rays = ray_pixels(rec)
    same(rays, fv["rays"])                                        # the composition starts from the same pixels
    assert r.soft_samples() == 0
    r.soft(S)
    got = r.soft_records()
    print(f"{case} {W}x{H} n={len(lights)} S={S}: {int(rays.sum())} ray pixels, occluded per light "
          f"{got.reshape(len(lights), -1).sum(1, dtype=np.int64).tolist()} of {S * int(rays.sum())} rays each")
    assert got.dtype == np.uint16 and got.shape == (len(lights), H, W)
    same(got, want)
    assert not got[:, ~rays].any()                                # a pixel that is not a ray pixel stays 0
    assert r.soft_samples() == S
    if case == "carnival":
        assert not got.any()
    else:
        assert got.any() and ((got > 0) & (got < S)).any()
    if case == "tekkaman-16":
        assert got[15].any()                                      # the packed table's last light


# ---- the anchor: radius 0 is the frame's own hard shadow ------------------------------------------

@pytest.mark.parametrize("case", ["tekkaman", "shadow_edge"])
def test_radius_zero_is_the_hard_shadow(po, case):
    name, W, H, lights, _ = CASES[case]
    n, S = len(lights), 6
    r = renderer(name)
    rec = session(r, case, radii=[0.0] * n, capture=True)
    rays = ray_pixels(rec)
    r.soft(S)
    got = r.soft_records()
    for i in range(n):
        bit = ((rec["light_mask"] >> i) & 1).astype(np.uint16)
        same(got[i], np.where(rays, S * bit, 0).astype(np.uint16))
    assert got.any()
    wsets = [[1] * n, [255, 64, 1][:n]] + ([[1, 0, 1], [0, 1, 0]] if n == 3 else [])
    for w in wsets:
        r.soft_resolve("lit", w)
        soft = r.framebuffer().copy()
        r.relight(w)
        same(soft, r.framebuffer())
        if set(w) <= {0, 1}:
            on = [light for light, x in zip(lights, w) if x]
            lit(r2 := renderer(name, "/frames"), W, H, on)
            r2.render()
            same(soft, r2.framebuffer())


# ---- accumulation, reset and the cursor -----------------------------------------------------

def test_accumulation_reset_and_cursor(po):
    case = "tekkaman"
    r = renderer("tekkaman")
    session(r, case)
    want8, _ = counts(case, 8)
    for _ in range(2):
        r.soft(3)
        r.soft(5, wait=False)
        assert r.soft_samples() == 8
        same(r.soft_records(), want8)
        r.soft_reset()
        assert r.soft_samples() == 0
    r.soft(8)
    same(r.soft_records(), want8)
    # single samples, differenced: the per-sample totals of tests/test_soft_cpu.py
    r.soft_reset()
    prev, totals = np.zeros_like(want8), []
    for _ in range(NS):
        r.soft(1)
        cur = r.soft_records()
        assert ((cur - prev) <= 1).all() and (cur >= prev).all()
        totals.append((cur - prev).reshape(len(cur), -1).sum(1, dtype=np.int64))
        prev = cur
    got = tuple(tuple(int(x) for x in row) for row in np.array(totals).T)
    print(f"tekkaman 64x64: occluded per light and sample {got}")
    assert got == TOTALS[case][0]
    # the cursor's cap: 1024 samples
    r.soft_reset()
    for _ in range(15):
        r.soft(64, wait=False)
    r.soft(60)
    assert r.soft_samples() == 1020
    before = r.soft_records()
    for k in (5, 64):
        with pytest.raises(rt.RtError, match=r"\(-2\): \S+"):
            r.soft(k)
    assert r.soft_samples() == 1020
    same(r.soft_records(), before)
    r.soft(4)
    assert r.soft_samples() == 1024
    with pytest.raises(rt.RtError, match=r"\(-2\): \S+"):
        r.soft(1, wait=False)
    assert int(r.soft_records().max()) <= 1024 and (r.soft_records() >= before).all()


# ---- the A/B images -----------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_variant_images_count_the_same(po, variant):
    """the A/B images of scripts/bench_soft.py (lib/variants: the waves per block, the deal order, the
    packet walk) against the same composition: a single round and several rounds"""
    vdir = os.path.join(_lib.LIB_DIR, "variants", variant)
    assert os.path.isfile(os.path.join(vdir, "rt_soft.vxbin"))
    # shadow_edge, one light, one sample: a block deals at most 64 triples, a single round; tekkaman, three
    # lights, 5 samples: up to 64 x 3 x 5 triples a block, several rounds, the last one partly filled
    for case, S in (("shadow_edge", 1), ("tekkaman", 5)):
        s = rt.Scene.load(mc.scene_file(CASES[case][0]))
        r = rt.Renderer(s, kernel_dir=vdir)
        session(r, case)
        r.soft(S)
        same(r.soft_records(), counts(case, S)[0])
        r.close()
        s.close()


# ---- the resolve ----------------------------------------------------------------------------------

def test_resolve(po):
    case, S = "tekkaman", 8
    name, W, H, lights, _ = CASES[case]
    want, _ = counts(case, S)
    r = renderer(name)
    rec = session(r, case, capture=True)
    r.soft(S)
    o = r.soft_records()
    same(o, want)
    base = r.relight_base()
    white = np.full((H, W), 0xFFFFFFFF, np.uint32)
    r.soft_resolve("grey")
    assert r.kernel_ms() > 0
    grey = r.framebuffer().copy()
    same(grey, rt.soft_resolve(white, rec["depth_flags"], o, S, [1, 1, 1]))
    assert len(np.unique(grey)) > 3
    hard = rt.relight_resolve(base, rec["depth_flags"], rec["light_mask"], [1, 1, 1])
    for weights in (None, [1, 1, 1], [255, 64, 1], [0, 0, 7]):
        r.soft_resolve("lit", weights)
        got = r.framebuffer().copy()
        same(got, rt.soft_resolve(base, rec["depth_flags"], o, S, [1, 1, 1] if weights is None else weights))
    r.soft_resolve("lit", wait=False)
    r.wait()
    assert int((r.framebuffer() != hard).sum()) >= 50, "the penumbra changes too few pixels to show"
    # more samples, another N: the resolve follows the cursor
    r.soft(3)
    r.soft_resolve("grey")
    same(r.framebuffer(), rt.soft_resolve(white, rec["depth_flags"], r.soft_records(), S + 3, [1, 1, 1]))
    # one light, frames in between: into the framebuffer in use, the second one
    case = "tekkaman-edge"
    want, _ = counts(case, 3)
    rec = session(r, case, capture=True, counters=False)
    r.start()
    r.soft(3, wait=False)
    r.start()
    r.soft_resolve("lit", [9], wait=False)
    r.wait()
    same(r.soft_records(), want)
    same(r.framebuffer(), rt.soft_resolve(r.relight_base(), rec["depth_flags"], want, 3, [9]))
    r.start()
    r.soft_resolve("grey", wait=False)
    r.wait()
    same(r.framebuffer(), rt.soft_resolve(np.full(want.shape[1:], 0xFFFFFFFF, np.uint32), rec["depth_flags"], want, 3, [1]))


# ---- what a session leaves alone, and what ends it ---------------------------------------------------

def test_isolation(po):
    case, S = "tekkaman", 5
    name, W, H, lights, radii = CASES[case]
    want, _ = counts(case, S)
    r = renderer(name)
    lit(r, W, H, lights)
    r.render()
    frame = r.framebuffer().copy()
    rec = r.aov().copy()
    r.ao_begin(radius=8.0, seed=SEED)
    r.ao(4)
    ao = r.ao_records().copy()
    r.soft_begin(radii, seed=SEED)
    r.soft(S)
    same(r.soft_records(), want)
    same(r.framebuffer(), frame)                                  # soft() writes no framebuffer,
    assert np.array_equal(r.aov_records().view(np.uint32), rec.view(np.uint32))   # no record
    same(r.ao_records(), ao)                                      # and no ambient-occlusion count
    # frames, record launches and ambient-occlusion launches in between leave the planes alone
    r.render()
    r.start()
    r.start()
    r.wait()
    r.aov()
    r.ao(2)
    same(r.soft_records(), want)
    assert r.soft_samples() == S
    # a change of lights ends the session
    def path_lights():
        # (refused itself under a configuration that is no path frame; the lights are not trusted past it)
        with pytest.raises(rt.RtError, match=r"\(-2\): \S+"):
            r.set_path_lights(lights[:2])

    changes = [(3, lambda: r.set_lights(lights[:2])), (2, lambda: r.set_light(lights[1])),
               (1, lambda: r.set_lights(lights)), (3, path_lights)]
    for n, change in changes:
        r.soft_begin([1.0] * n, seed=SEED)
        r.soft(1)
        change()
        for fn, a in ((r.soft, (1,)), (r.soft_samples, ()), (r.soft_records, ()), (r.soft_reset, ()),
                      (r.soft_resolve, ("grey",))):
            with pytest.raises(rt.RtError, match=r"\(-2\): \S+"):
                fn(*a)
    r.ao(1)                                                       # (the ambient-occlusion session goes on)
    r.set_lights(lights)
    # a session begun again after the change counts under the new lights
    r.aov()
    r.soft_begin(radii, seed=SEED)
    r.soft(S)
    same(r.soft_records(), want)


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
    _refused(r.soft_begin, [1.0])
    _refused(r.soft, 1)
    _refused(r.soft_resolve, "grey")
    _refused(r.soft_samples)
    r.render()                                                   # the renderer still renders its frame


def test_refused_ordered_tail(po):
    sv = rt.Scene.load(scene_path("vase"), om_layers=True)
    assert sv.om_split()[1] > 0
    ro = rt.Renderer(sv)
    ro.configure(64, 64, shadows=True)
    _refused(ro.soft_begin, [1.0])
    _refused(ro.soft, 1)
    ro.close()
    sv.close()


def test_state(po):
    W = H = 32
    s = rt.Scene.load(mc.scene_file("convex"))
    r = rt.Renderer(s)
    with pytest.raises(rt.RtError):
        r.soft_begin([1.0])                                      # before any configure
    r.configure(W, H, shadows=True)
    _refused(r.soft_begin, [1.0])                                # no record launch since the configure
    _refused(r.soft, 1)
    _refused(r.soft_reset)
    _refused(r.soft_records)
    r.aov()
    for radius in (-1.0, float("nan"), float("inf"), float("-inf")):
        _refused(r.soft_begin, [radius])
    _refused(r.soft_begin, [1.0, 1.0])                           # one light in use
    _refused(r.soft, 1)                                          # the refused begins began nothing
    r.soft_begin([0.5])
    r.soft(3)
    for bad in ([float("nan")], [1.0, 1.0]):                     # a refused begin leaves the session as it was
        _refused(r.soft_begin, bad)
    r.soft(2)
    assert r.soft_samples() == 5 and r.soft_records().shape == (1, H, W)
    r.soft_begin([0.5])
    _refused(r.soft_resolve, "grey")                             # N = 0
    _refused(r.soft_resolve, "lit")
    _refused(r.soft_records)
    for k in (0, 65, 1 << 20):
        _refused(r.soft, k)
        _refused(r.soft, k, wait=False)
    assert r.soft_samples() == 0
    r.soft(1)
    with pytest.raises(rt.RtError):
        r.soft_resolve("gray")
    _refused(r.soft_resolve, "lit")                              # no relight capture
    _refused(r.soft_resolve, "lit", [1])
    assert rt.lib().rt_render_soft_resolve(r._h, 7, None, 0) == -2   # an unknown mode
    r.soft_resolve("grey")
    same(r.framebuffer(), np.full((H, W), 0xFFFFFFFF, np.uint32))   # convex: nothing is shadowed
    r.relight_capture()                                          # (a record launch: the session goes on)
    r.soft_resolve("lit", [1])
    r.soft_resolve("lit")
    _refused(r.soft_resolve, "lit", [1, 1])                      # a wrong n
    _refused(r.soft_resolve, "lit", [0])                         # every weight 0
    r.set_lights([mc.LIGHT, (30.0, -20.0, 95.0)])                # ends the session
    _refused(r.soft_resolve, "grey")
    r.aov()
    _refused(r.soft_begin, [1.0])                                # two lights in use
    _refused(r.soft_begin, [1.0, 1.0, 1.0])
    r.soft_begin([1.0, 0.0])
    r.soft(2)
    assert r.soft_records().shape == (2, H, W) and not r.soft_records().any()
    r.configure(W, H, shadows=True)                              # ends the session
    _refused(r.soft, 1)
    _refused(r.soft_resolve, "grey")
    r.close()
    s.close()


def test_begin_the_arena_cannot_hold(po):
    """sixteen lights at 8192 x 4096 need planes of 16 * 2^25 * 2 B = 1 GiB in one piece.  The arena's 4 GiB
    hold the kernel images at their fixed addresses, 16 MiB apart from 1.2 GiB up, and below them the
    frame's own buffers (framebuffers 256 MiB, records 512 MiB): no piece of 1 GiB is left.  The begin is
    refused and begins nothing, and a begin the arena can hold then works in the same renderer."""
    from test_soft_cpu import LIGHTS16, RADII16
    r = renderer("tekkaman", "/arena")
    # (a small session first: the images are loaded at their fixed arena addresses before the large
    # configuration's buffers could come to lie across them)
    session(r, "tekkaman-16")
    r.soft(1)
    r.configure(8192, 4096, shadows=True, light=LIGHTS16[0], counters=False)
    r.set_lights(LIGHTS16)
    r.aov(wait=False)
    r.wait()
    for _ in range(2):
        with pytest.raises(rt.RtError, match=r"\(-2\): .*arena cannot hold 1073741824 bytes"):
            r.soft_begin(RADII16, seed=SEED)
        _refused(r.soft, 1)
        _refused(r.soft_samples)
        _refused(r.soft_resolve, "grey")
    session(r, "tekkaman-16")
    r.soft(2)
    same(r.soft_records(), counts("tekkaman-16", 2)[0])


# ---- counters -----------------------------------------------------------------------------------

def test_counters(po):
    case, S = "tekkaman", 5
    want, fv = counts(case, S)
    r = renderer("tekkaman")
    session(r, case, counters=True)
    r.soft(S)
    st = r.stats()
    assert st["shadow_rays"] == S * 3 * len(fv["idx"])
    assert st["occluded"] == int(want.sum(dtype=np.int64)) == int(r.soft_records().sum(dtype=np.int64))
    assert st["primary_rays"] == 0 and st["geometry_hits"] == 0 and st["bounce_rays"] == 0
    assert r.kernel_ms() > 0


# ---- the CLI --------------------------------------------------------------------------------------

def test_rtapp_soft_shadows(po, tmp_path):
    from PIL import Image
    W = H = 64
    lights = mc.TEKKAMAN_LIGHTS
    out = tmp_path / "out.png"
    largs = ["-L" + ",".join(str(x) for x in lights[0])] + ["-M" + ",".join(str(x) for x in l) for l in lights[1:]]
    p = subprocess.run([os.path.join(_lib.LIB_DIR, "rtapp"), "-t", scene_path("tekkaman"), "-S", *largs, "-E16,4",
                        "-w64", "-h64", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Soft: 16 samples, radius 4" in p.stdout, p.stdout
    got = np.array(Image.open(out).convert("RGBA"))
    # the same frame by the Python path
    r = renderer("tekkaman")
    lit(r, W, H, lights)
    r.relight_capture()
    r.soft_begin([4.0] * 3, seed=rt.RT_SOFT_DEFAULT_SEED)
    r.soft(16)
    r.soft_resolve("lit")
    want = r.framebuffer().copy()
    assert po.compare_images(got, po.argb_to_rgba_image(want), tol=0) == 0
    r.relight([1, 1, 1])
    assert int((want != r.framebuffer()).sum()) >= 50, "the penumbra changes too few pixels to show"
    bad = subprocess.run([os.path.join(_lib.LIB_DIR, "rtapp"), "-t", scene_path("tekkaman"), "-E8", "-o", "null"],
                         capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "Error: -E" in bad.stdout and "Soft:" not in bad.stdout, bad.stdout
