"""CPU tests holding the oracle's shadow rays and path tracer (oracle/rt.c) to
the independent float64 model of tests/rt_reference.py: the shadow verdict of
every robust pixel, the plane parameter behind the secondary-ray origin, the
path frames that no random number reaches to the last bit, and the others in
distribution -- per channel and pooled over the image, against the model's
own sampling error, with the constants measured model against model
(tests/rt_model_checks.py).  Primary visibility and the unlit frame
are inputs of the model: they are the raster's, pinned by the reference's
goldens."""
import os

import numpy as np
import pytest

os.environ.setdefault("SKYBOX_RT_NO_TORCH", "1")

import rt_model_checks as mc  # noqa: E402
import synth_scene  # noqa: E402
from skybox_rt_amd import rt  # noqa: E402

_osc = {}
_frames = {}


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def oscene(po, name):
    """(oracle scene, the product host's BVH of it)"""
    if name not in _osc:
        s = rt.Scene.load(mc.scene_file(name))
        _osc[name] = (po.OracleScene(po.cgltrace.load(mc.scene_file(name))), s.bvh())
        s.close()
    return _osc[name]


def frame(po, name, w, h, bvh=True, **kw):
    """(colour, pid, t) of an oracle frame; computed once, left unchanged"""
    key = (name, w, h, bvh, tuple(sorted(kw.items())))
    if key not in _frames:
        osc, tree = oscene(po, name)
        c, pid, t, _ = po.rt_render(osc, po.rt_params(w, h, nthreads=8, **kw), bvh=tree if bvh else None)
        for a in (c, pid, t):
            a.setflags(write=False)
        _frames[key] = (c, pid, t)
    return _frames[key]


def plain_of(po):
    return lambda name, w, h: frame(po, name, w, h, shadows=False)[0]


def pid_of(po):
    return lambda name, w, h: frame(po, name, w, h, shadows=False)[1]


# ---- shadow verdicts and the plane parameter ----------------------------------------

VERDICT_CASES = [("tekkaman", 128, 128, mc.TEKKAMAN_LIGHTS), ("tekkaman", 200, 136, mc.TEKKAMAN_LIGHTS),
                 ("box", 64, 64, mc.TEKKAMAN_LIGHTS), ("shadow_edge", 64, 64, synth_scene.SHADOW_EDGE_LIGHTS),
                 ("shadow_edge", 65, 33, synth_scene.SHADOW_EDGE_LIGHTS)]


@pytest.mark.parametrize("bvh", (True, False), ids=("bvh", "brute"))
@pytest.mark.parametrize("lists", (True, False), ids=("lists", "nolists"))
@pytest.mark.parametrize("nlights", (1, 3), ids=("K1", "K3"))
@pytest.mark.parametrize("name,w,h,lights", VERDICT_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in VERDICT_CASES])
def test_shadow_verdicts_equal_model(po, name, w, h, lights, nlights, lists, bvh):
    plain, pid, _ = frame(po, name, w, h, shadows=False)
    known = (plain & np.uint32(0xFFFFFF)) != 0               # a shadowed colour is c >> 1 per channel
    for L in lights[:nlights]:
        c, _, t = frame(po, name, w, h, bvh=bvh, shadows=True, light=tuple(L), shadow_lists=lists)
        v = mc.verdict(name, w, h, pid, L)
        # the oracle starts a shadow ray where its own t is finite and > 0
        geom = (pid >= 0) & mc.model(name, w, h)[1].is_geom[np.maximum(pid, 0)]
        with np.errstate(invalid="ignore"):
            rays = geom & (t > 0) & np.isfinite(t)
        amb = mc.check_verdicts(v, rays, c != plain, t, known, what=f"{name} {w}x{h} light {L}")
        print(f"{name} {w}x{h} light {L}: {int(v['rays'].sum())} rays, {amb} ambiguous, "
              f"{int(v['occluded'].sum())} occluded")


@pytest.mark.parametrize("name,w,h", [("tekkaman", 200, 200), ("interreflection", 32, 32), ("interreflection", 128, 128),
                                      ("convex", 32, 32)])
def test_plane_t_within_a_quarter_of_the_pull_back(po, name, w, h):
    _, pid, t = frame(po, name, w, h, shadows=True)
    v = mc.verdict(name, w, h, pid, mc.LIGHT)
    assert v["rays"].any()
    mc.check_plane_t(v, t, f"{name} {w}x{h}")


def test_shadow_edge_scene_has_its_cases(po):
    """the scene's parts do what they are there for, on the model alone: under the
    close light the triangle past the light would shadow many pixels if the segment
    did not end there, the averted quad's pixels are lit only through the self-skip,
    and the wall behind the pair of triangles sharing an edge lies in one shadow"""
    w = h = 64
    pid = pid_of(po)("shadow_edge", w, h)
    m = mc.model("shadow_edge", w, h)[1]
    L = synth_scene.SHADOW_EDGE_LIGHTS[0]
    v = mc.verdict("shadow_edge", w, h, pid, L)
    both = v["robust"] & v["rays"]
    for kw in (dict(segment_end=False), dict(self_skip=False)):
        vv = m.shadow_verdict(pid, L, v=mc.rr.variant(**kw))
        assert int((vv["occluded"] != v["occluded"])[both].sum()) >= 50, kw
    assert int((v["occluded"] & (pid <= 1)).sum()) >= 100    # wall pixels in shadow


# ---- path frames no random number reaches ------------------------------------------------

DET_CASES = [("tekkaman", 64, 0, (1,)), ("box", 64, 0, (1,)), ("shadow_edge", 64, 0, (1,)),
             ("interreflection", 32, 0, (1,)), ("convex", 32, 0, (1,)), ("convex", 32, 1, (1, 2, 3)),
             ("convex", 32, 4, (1, 2, 3))]


@pytest.mark.parametrize("name,size,bounces,seeds", DET_CASES, ids=[f"{c[0]}-{c[1]}-b{c[2]}" for c in DET_CASES])
def test_deterministic_path_frames_equal_model(po, name, size, bounces, seeds):
    plain, pid, _ = frame(po, name, size, size, shadows=False)
    for seed in seeds:
        c = frame(po, name, size, size, path=True, bounces=bounces, seed=seed)[0]
        mc.check_deterministic(name, size, size, pid, plain, mc.LIGHT, bounces, c, f"{name} {size} b{bounces} seed {seed}")


# ---- path frames in distribution ------------------------------------------------------------

def oracle_frames(po, bounces, light=mc.LIGHT):
    """int64 [N_FRAMES, n, 3]: the path pixels of the oracle's frames of seeds SEED0 ..."""
    key = ("stack", bounces, tuple(light))
    if key not in _frames:
        osc = oscene(po, "interreflection")[0]
        plain, pid, _ = frame(po, "interreflection", 32, 32, shadows=False)
        idx = np.flatnonzero(mc.model("interreflection", 32, 32)[1].primary(pid)[0].reshape(-1))
        out = np.empty((mc.N_FRAMES, len(idx), 3), np.int64)
        for i in range(mc.N_FRAMES):
            # (brute force, no lists: neither changes a frame -- tests/test_oracle_pt.py,
            # test_oracle_slists.py -- and both are built anew for every frame)
            c = po.rt_render(osc, po.rt_params(32, 32, path=True, bounces=bounces, seed=mc.SEED0 + i, light=light,
                                               shadow_lists=False))[0]
            out[i] = mc.rgb(c.reshape(-1)[idx])
        out.setflags(write=False)
        _frames[key] = (idx, out)
    return _frames[key]


@pytest.mark.parametrize("bounces", mc.BOUNCES)
def test_path_frame_means_equal_model(po, bounces):
    plain, pid, _ = frame(po, "interreflection", 32, 32, shadows=False)
    idx, mean_m, var_m = mc.model_moments("interreflection", 32, 32, pid, plain, mc.LIGHT, bounces)
    oidx, fr = oracle_frames(po, bounces)
    assert np.array_equal(idx, oidx) and len(idx) >= 300
    assert fr.mean() < 0.3 * 255                              # the clamp rarely binds
    mc.check_means(fr.mean(0), mc.N_FRAMES, mean_m, var_m, what=f"oracle, {bounces} bounces")


def test_two_light_path_frame_means_equal_model(po):
    """a K-light sample is the rounded mean of the single-light samples along one path
    (DESIGN 2.1): the oracle's single-light frames of one seed share their paths"""
    plain, pid, _ = frame(po, "interreflection", 32, 32, shadows=False)
    idx, mean_m, var_m = mc.model_moments("interreflection", 32, 32, pid, plain, mc.PATH_LIGHTS, 4)
    per = [oracle_frames(po, 4, L)[1] for L in mc.PATH_LIGHTS]
    K = len(per)
    fr = (2 * sum(per) + K) // (2 * K)
    mc.check_means(fr.mean(0), mc.N_FRAMES, mean_m, var_m, what="oracle, 2 lights, 4 bounces")


@pytest.mark.parametrize("bounces", mc.BOUNCES)
def test_path_samples_independent_over_pixels_and_seeds(po, bounces):
    idx, fr = oracle_frames(po, bounces)
    mc.check_independence(fr, idx, 32, what=f"oracle, {bounces} bounces")


# ---- the criteria notice what they should ------------------------------------------------------

def test_criteria_notice_every_variant(po):
    mc.check_sensitivity(pid_of(po), plain_of(po))
