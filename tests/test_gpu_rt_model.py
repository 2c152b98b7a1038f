"""GPU tests holding the device's shadow rays and path tracer to the independent
float64 model of tests/rt_reference.py, directly (no oracle frame is read):
the visibility records of Renderer.aov() -- which pixels start a shadow ray,
the plane t, every robust verdict per light -- and path frames: those no
random number reaches to 0.5 LSB, the others through the exact 8-bit sums of
accumulate(), per channel and pooled, with the criteria and constants of
tests/rt_model_checks.py (measured model against model).  The
model's inputs, the raster's winner per pixel and the unlit frame, are read
from the device too (pinned by the raster goldens through test_gpu_aov.py and
test_gpu_rt.py)."""
import os

import numpy as np
import pytest

import rt_model_checks as mc
import synth_scene

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, rt  # noqa: E402

_dev = {}
_inputs = {}


def renderer(name, key=""):
    if (name, key) not in _dev:
        s = rt.Scene.load(mc.scene_file(name))
        kd = os.path.join(_lib.LIB_DIR, key) if key else None
        _dev[(name, key)] = (s, rt.Renderer(s, kernel_dir=kd))
    return _dev[(name, key)][1]


def inputs(name, w, h):
    """(pid, plain) of the device at a size; read once, left unchanged"""
    if (name, w, h) not in _inputs:
        r = renderer(name)
        r.configure(w, h, shadows=False)
        r.render()
        plain = r.framebuffer().copy().reshape(h, w)
        pid = r.aov()["pid"].copy()
        for a in (plain, pid):
            a.setflags(write=False)
        _inputs[(name, w, h)] = (pid, plain)
    return _inputs[(name, w, h)]


# ---- shadows through the visibility records -------------------------------------------

AOV_CASES = [("shadow_edge", 64, 64, 1), ("shadow_edge", 64, 64, 3), ("shadow_edge", 65, 33, 1),
             ("shadow_edge", 65, 33, 3), ("tekkaman", 128, 128, 1)]


@pytest.mark.parametrize("mode", ("lists", "bvh_walk", "host_setup"))
@pytest.mark.parametrize("name,w,h,K", AOV_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-K{c[3]}" for c in AOV_CASES])
def test_visibility_records_equal_model(name, w, h, K, mode):
    lights = (synth_scene.SHADOW_EDGE_LIGHTS if name == "shadow_edge" else mc.TEKKAMAN_LIGHTS)[:K]
    r = renderer(name)
    kw = {} if mode == "lists" else {mode: True}
    if mode == "bvh_walk":                                    # one light per launch: no several-light image walks the BVH
        recs = []
        for L in lights:
            r.configure(w, h, shadows=True, light=L, **kw)
            recs.append(r.aov().copy())
        masks = [rec["light_mask"] for rec in recs]
        rec = recs[0]
    else:
        r.configure(w, h, shadows=True, light=lights[0], **kw)
        if K > 1:
            r.set_lights(lights)
        rec = r.aov()
        masks = [rec["light_mask"] >> np.uint32(i) for i in range(K)]
        assert not (rec["light_mask"] >> np.uint32(K)).any()
    if mode != "lists":
        assert r.setup_stats()["slist_on"] == 0
    pid = rec["pid"]
    assert np.array_equal(pid, inputs(name, w, h)[0])
    rays = (rec["depth_flags"] & np.uint32(rt.RT_AOV_SHADOW_RAY)) != 0
    for L, mask in zip(lights, masks):
        v = mc.verdict(name, w, h, pid, L)
        amb = mc.check_verdicts(v, rays, (mask & np.uint32(1)) != 0, rec["t"], what=f"{name} {w}x{h} {mode} light {L}")
        print(f"{name} {w}x{h} {mode} light {L}: {int(rays.sum())} rays, {amb} ambiguous")


# ---- path frames no random number reaches -------------------------------------------------

DET_CASES = [("shadow_edge", 64, 0, (1,)), ("interreflection", 32, 0, (1,)), ("tekkaman", 64, 0, (1,)),
             ("convex", 32, 0, (1,)), ("convex", 32, 1, (1, 2, 3)), ("convex", 32, 4, (1, 2, 3))]


@pytest.mark.parametrize("name,size,bounces,seeds", DET_CASES, ids=[f"{c[0]}-{c[1]}-b{c[2]}" for c in DET_CASES])
def test_deterministic_path_frames_equal_model(name, size, bounces, seeds):
    pid, plain = inputs(name, size, size)
    r = renderer(name)
    for seed in seeds:
        r.configure(size, size, path=True, bounces=bounces, seed=seed)
        r.render()
        mc.check_deterministic(name, size, size, pid, plain, mc.LIGHT, bounces, r.framebuffer(),
                               f"{name} {size} b{bounces} seed {seed}")


# ---- path frames in distribution ---------------------------------------------------------------

def accumulated_means(r, idx, n):
    """n samples in launches of 32 -> the path pixels' exact means sum / n"""
    r.accum_begin()
    for _ in range(n // 32):
        r.accumulate(32)
    rec = r.accum().reshape(-1, 4)[idx].astype(np.float64)
    assert (rec[:, 3] == n).all()
    return rec[:, :3] / n


@pytest.mark.parametrize("bounces", mc.BOUNCES)
def test_accumulated_means_equal_model(bounces):
    pid, plain = inputs("interreflection", 32, 32)
    idx, mean_m, var_m = mc.model_moments("interreflection", 32, 32, pid, plain, mc.LIGHT, bounces)
    assert len(idx) >= 300
    r = renderer("interreflection")
    r.configure(32, 32, path=True, bounces=bounces, seed=mc.SEED0)
    mean_d = accumulated_means(r, idx, mc.N_FRAMES)
    mc.check_means(mean_d, mc.N_FRAMES, mean_m, var_m, what=f"device, {bounces} bounces")


def test_two_light_accumulated_means_equal_model():
    pid, plain = inputs("interreflection", 32, 32)
    idx, mean_m, var_m = mc.model_moments("interreflection", 32, 32, pid, plain, mc.PATH_LIGHTS, 4)
    r = renderer("interreflection")
    r.configure(32, 32, path=True, bounces=4, seed=mc.SEED0, light=mc.PATH_LIGHTS[0])
    r.set_path_lights(mc.PATH_LIGHTS)
    mean_d = accumulated_means(r, idx, mc.N_FRAMES)
    mc.check_means(mean_d, mc.N_FRAMES, mean_m, var_m, what="device, 2 lights, 4 bounces")


COMPACT_FRAMES = 256       # the compacting image has no accumulating form: whole frames, one seed each


def test_compact_image_means_equal_model():
    pid, plain = inputs("interreflection", 32, 32)
    idx, mean_m, var_m = mc.model_moments("interreflection", 32, 32, pid, plain, mc.LIGHT, 4)
    r = renderer("interreflection", "pt_compact")
    tot = np.zeros((len(idx), 3), np.int64)
    for i in range(COMPACT_FRAMES):
        r.configure(32, 32, path=True, bounces=4, seed=mc.SEED0 + i)
        r.render()
        tot += mc.rgb(r.framebuffer().reshape(-1)[idx])
    assert r.stats()["block"] == 256                          # the compacting image ran
    mc.check_means(tot / COMPACT_FRAMES, COMPACT_FRAMES, mean_m, var_m, what="device, pt_compact, 4 bounces")
