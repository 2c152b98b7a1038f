"""GPU tests of frames lit by several point lights in one launch (vx_rt.h
rt_renderer_set_lights; images rt_lights / rt_lights_stats, rt_kernel.hip
RT_LIGHTS) against the untouched oracle, bit for bit.

The model is built here from frames the oracle already produces: a K-light
frame is, per pixel and colour channel, the rounded mean (2 * sum + K) //
(2 * K) of the K single-light RT_RENDER_SHADOWS frames, under the primary
colour's alpha (the same in every one of them); its shadow-ray counters are the
no-shadow frame's plus every light's own share.  No reference exists for this
row; the oracle's verdicts themselves are held to the model of
tests/rt_reference.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from test_gpu_light import LIGHTS

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, rt  # noqa: E402

# the measurement script's grid (scripts/bench_lights.py): 4 x 4, side 20, centred on the
# default light, in the plane w = 80
GRID = [(-10.0 + 20.0 * i / 3.0, 50.0 + 20.0 * j / 3.0, 80.0) for j in range(4) for i in range(4)]
SIXTEEN = list(LIGHTS) + GRID[:11]
_state = {}
_frames = {}


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def setup(po):
    if not _state:
        s = rt.Scene.load(scene_path("tekkaman"))
        _state["s"] = (s, rt.Renderer(s), po.OracleScene(po.cgltrace.load(scene_path("tekkaman"))),
                       s.bvh() + (s.bvh4(),))
    return _state["s"]


def single(po, w, h, light, shadows=True, **kw):
    """(frame, counters) of the oracle's single-light frame; computed once, left unchanged."""
    key = (w, h, tuple(light) if shadows else None, tuple(sorted(kw.items())))
    if key not in _frames:
        _, _, osc, bvh = setup(po)
        c, _, _, k = po.rt_render(osc, po.rt_params(w, h, shadows=shadows, light=light, nthreads=8, **kw), bvh=bvh)
        c = c.reshape(h, w)
        c.setflags(write=False)
        _frames[key] = (c, k)
    return _frames[key]


def mean_frame(po, w, h, lights, min_mixed=100, **kw):
    """The numpy mean of the single-light frames.  At least min_mixed of its pixels have lights
    that see them and lights that do not (their frames differ): the resolve is exercised."""
    fr = [single(po, w, h, L, **kw)[0] for L in lights]
    n = len(fr)
    out = fr[0] & np.uint32(0xFF000000)
    for sh in (16, 8, 0):
        tot = sum(((c >> np.uint32(sh)) & np.uint32(0xFF)).astype(np.uint64) for c in fr)
        out = out | (((2 * tot + n) // (2 * n)).astype(np.uint32) << np.uint32(sh))
    mixed = int(np.any([c != fr[0] for c in fr[1:]], axis=0).sum()) if n > 1 else 0
    print(f"{w}x{h} K={n}: {mixed} pixels whose single-light frames differ")
    assert mixed >= min_mixed, f"only {mixed} pixels with 0 < o < K"
    for c in fr:
        assert np.array_equal(c >> np.uint32(24), fr[0] >> np.uint32(24))
    return out


def counters(po, w, h, lights, **kw):
    """shadow-ray counters: P + sum_i (oracle_i - P), P the no-shadow frame's; the rest any frame's."""
    p = single(po, w, h, LIGHTS[0], shadows=False)[1]
    ks = [single(po, w, h, L, **kw)[1] for L in lights]
    want = {key: p[key] + sum(k[key] - p[key] for k in ks)
            for key in ("shadow_rays", "occluded", "tri_tests", "node_visits")}
    for key in ("primary_rays", "geometry_hits", "layer_tests"):
        assert all(k[key] == ks[0][key] for k in ks)
        want[key] = ks[0][key]
    return want


@pytest.mark.parametrize("w,h,lights", [(128, 128, LIGHTS[:1]), (128, 128, LIGHTS[:2]), (128, 128, LIGHTS[:3]),
                                        (128, 128, LIGHTS), (128, 128, SIXTEEN), (200, 136, LIGHTS[:3])],
                         ids=["128-K1", "128-K2", "128-K3", "128-K5", "128-K16", "200x136-K3"])
def test_frames_equal_mean_of_oracle_frames(po, w, h, lights):
    _, r, _, _ = setup(po)
    r.configure(w, h, shadows=True, light=lights[0])
    if len(lights) == 1:
        r.render()
        plain = r.framebuffer()
    r.set_lights(lights)
    r.render()
    fb = r.framebuffer()
    want = mean_frame(po, w, h, lights, min_mixed=100 if len(lights) > 1 else 0)
    assert np.array_equal(fb, want), f"{int((fb != want).sum())} pixels differ"
    if len(lights) == 1:
        assert np.array_equal(fb, plain)
    info = r.lights_info()
    assert len(info) == len(lights)
    for i, L in zip(info, lights):
        assert np.array_equal(np.float32(i["light"]), np.float32(L))


def test_counters(po):
    _, r, _, _ = setup(po)
    lights = LIGHTS[:3]
    r.configure(256, 256, shadows=True, light=lights[0], instrumented=True)
    r.set_lights(lights)
    r.render()
    st = r.stats()
    want = counters(po, 256, 256, lights)
    for key, v in want.items():
        assert st[key] == v, (key, st[key], v)
    assert np.array_equal(r.framebuffer(), mean_frame(po, 256, 256, lights))


def test_lists_per_light(po):
    _, r, osc, _ = setup(po)
    r.configure(128, 128, shadows=True, light=LIGHTS[0])
    r.set_lights(LIGHTS)
    info = r.lights_info()
    geom = r.records("geom")
    for i, L in enumerate(LIGHTS):
        idx, ent = po.shadow_lists(osc, L)
        assert info[i]["slist_on"] == 1 and info[i]["slist_entries"] == len(ent), (i, info[i])
        assert np.array_equal(r.light_records(i, "sidx"), idx), i
        slist = r.light_records(i, "slist")
        assert slist.shape == (len(ent) + 1, 12)
        got = slist[:-1].copy()
        got[:, 7] = 0.0
        assert np.array_equal(got.view(np.uint32), geom[ent].view(np.uint32)), i


def test_bvh_shadow_path(po, monkeypatch):
    monkeypatch.setenv("RT_SHADOW_LISTS", "0")
    _, r, _, _ = setup(po)
    lights = LIGHTS[:3]
    r.configure(128, 128, shadows=True, light=lights[0], instrumented=True)
    r.set_lights(lights)
    assert [i["slist_on"] for i in r.lights_info()] == [0, 0, 0]
    r.render()
    st = r.stats()
    fb = r.framebuffer()
    assert np.array_equal(fb, mean_frame(po, 128, 128, lights, shadow_lists=False))
    for key, v in counters(po, 128, 128, lights, shadow_lists=False).items():
        assert st[key] == v, (key, st[key], v)


def test_mixed_lists_and_bvh(po, monkeypatch):
    """LIGHTS[3]'s lists (244 783 entries) exceed the limit: that light walks the BVH, the
    other two scan their lists, in the same drain."""
    monkeypatch.setenv("RT_BLIST_MAX_ENTRIES", "100000")
    _, r, _, _ = setup(po)
    lights = [LIGHTS[0], LIGHTS[3], LIGHTS[4]]
    r.configure(128, 128, shadows=True, light=lights[0])
    r.set_lights(lights)
    assert [i["slist_on"] for i in r.lights_info()] == [1, 0, 1]
    r.render()
    fb = r.framebuffer()
    want = mean_frame(po, 128, 128, lights)
    assert np.array_equal(fb, want), f"{int((fb != want).sum())} pixels differ"


def test_host_setup_walks_the_bvh(po):
    """RT_RENDER_HOST_SETUP builds no shadow lists: every light walks the BVH."""
    _, r, _, _ = setup(po)
    lights = LIGHTS[:2]
    r.configure(128, 128, shadows=True, light=lights[0], host_setup=True)
    r.set_lights(lights)
    assert [i["slist_on"] for i in r.lights_info()] == [0, 0]
    r.render()
    assert np.array_equal(r.framebuffer(), mean_frame(po, 128, 128, lights))


def test_shards(po):
    _, r, _, _ = setup(po)
    lights = LIGHTS[:2]
    fbs = []
    for i in range(3):
        r.configure(128, 128, shadows=True, light=lights[0], shard_index=i, shard_count=3)
        r.set_lights(lights)
        r.render()
        fbs.append(r.framebuffer().copy())
    want = mean_frame(po, 128, 128, lights)
    assert np.array_equal(rt.deinterleave_tiles(fbs, 128, 128), want)
    # each compact buffer alone: its shard's tiles of the mean frame
    for i in range(3):
        others = [fbs[j] if j == i else np.zeros_like(fbs[j]) for j in range(3)]
        tiles = rt.deinterleave_tiles([np.ones_like(f) if j == i else np.zeros_like(f)
                                       for j, f in enumerate(fbs)], 128, 128).astype(bool)
        assert np.array_equal(rt.deinterleave_tiles(others, 128, 128)[tiles], want[tiles]), i


def _refused(fn, *a):
    with pytest.raises(rt.RtError, match=r"\(-2\)"):
        fn(*a)


def test_state(po):
    s, _, _, _ = setup(po)
    r = rt.Renderer(s)
    L = LIGHTS[2]
    one = single(po, 128, 128, L)[0]
    r.configure(128, 128, shadows=True, light=LIGHTS[0], counters=False)
    r.set_lights(LIGHTS[:3])
    r.render()
    assert np.array_equal(r.framebuffer(), mean_frame(po, 128, 128, LIGHTS[:3]))
    r.set_light(L)                                            # back to one light
    assert len(r.lights_info()) == 1
    r.render()
    assert np.array_equal(r.framebuffer(), one)
    r.start()                                                 # overlapped frames, two framebuffers
    r.start()
    r.wait()
    assert np.array_equal(r.framebuffer(), one) and np.array_equal(r.framebuffer_prev(), one)
    r.start()                                                 # set_lights behind queued frames
    r.start()
    r.set_lights(LIGHTS[3:5])
    r.start()
    r.wait()
    assert np.array_equal(r.framebuffer(), mean_frame(po, 128, 128, LIGHTS[3:5]))
    r.configure(128, 128, shadows=True, light=L, counters=False)   # a configure: one light again
    r.render()
    assert np.array_equal(r.framebuffer(), one)
    _refused(r.set_lights, [])                                # 0 lights
    _refused(r.set_lights, SIXTEEN + [GRID[11]])              # 17
    r.configure(128, 128, path=True)
    _refused(r.set_lights, LIGHTS[:2])
    r.configure(128, 128, shadows=True, flat=True)
    _refused(r.set_lights, LIGHTS[:2])
    r.configure(128, 128, shadows=True, bvh_walk=True)
    _refused(r.set_lights, LIGHTS[:2])
    r.configure(128, 128, shadows=False)
    _refused(r.set_lights, LIGHTS[:2])                        # no shadow rays
    r.configure(128, 128, shadows=True, bvh_width=2)
    _refused(r.set_lights, LIGHTS[:2])                        # a layout the generic images run
    r.close()


def test_refusals_by_scene_and_kernel_directory(po):
    s, _, _, _ = setup(po)
    # a kernel directory with an rt_kernel.vxbin of its own and no rt_lights.vxbin
    rv = rt.Renderer(s, kernel_dir=os.path.join(_lib.LIB_DIR, "variants", "stamp"))
    rv.configure(128, 128, shadows=True)
    _refused(rv.set_lights, LIGHTS[:2])
    rv.close()
    # a scene whose ordered tail is not empty renders with rt_om: one light
    sv = rt.Scene.load(scene_path("vase"), om_layers=True)
    assert sv.om_split()[1] > 0
    ro = rt.Renderer(sv)
    ro.configure(128, 128, shadows=True)
    _refused(ro.set_lights, LIGHTS[:2])
    ro.close()
    sv.close()


def test_rtapp_lights(po, tmp_path):
    out = tmp_path / "lights.png"
    lights = LIGHTS[:3]
    arg = [f"{x:g},{y:g},{w:g}" for x, y, w in lights]
    p = subprocess.run([os.path.join(_lib.LIB_DIR, "rtapp"), "-t", scene_path("tekkaman"), "-w", "128", "-h", "128",
                        "-S", "-L", arg[0], "-M", arg[1], "-M", arg[2], "-o", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Lights: 3" in p.stdout
    got = po.load_png_argb(str(out))[::-1]                    # the PNG is top-down
    assert np.array_equal(got, mean_frame(po, 128, 128, lights))
