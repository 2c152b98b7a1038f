"""GPU test (MI355X) of the in-place last chunk of image rt_kernel
(kernels/rt_kernel.hip RT_FUSED_CHUNK: under RT_FLAG_FUSED a wave traces its
last geometry chunk's shadow rays behind its shading's loads instead of through
the LDS queue and the drain; env RT_FUSED_CHUNK=0 at configure: the queue and
the drain as before).

On the smallest shapes that still hold every case -- tekkaman at 40x24 (blocks
overhang the image's edge) and at 128^2 (blocks full of rays and blocks mixing
winners with layer pixels, lit and occluded rays, scans of several rounds), box
and scene at 96^2 under the lights of tests/test_oracle_slists.py that lie
inside the model, on a cube-face diagonal and far away -- the frames with the
knob on equal the frames with the knob off and the oracle's, bit for bit:

* rendered synchronously and as overlapped frames (several start(), one wait());
* with RT_BG_TIER 0, 1 and 2, each with RT_LANE_CHUNKS 1 and 2 (two chunks per
  wave: the queue and the fused last chunk run in one wave);
* behind set_light under the default list policy (stale lists: the frame takes
  the queue and the BVH walk with the flag set) and under set_list_policy(0)
  (lists rebuilt at once: the fused chunk under the new light);
* as three shards;
* and the plain image's ray counters (shadow rays, occluded) are the oracle's.

test_cases_hold_every_kind asserts from the oracle's pid arrays and counters
that the cases contain a block full of rays, a block mixing winners with other
pixels, a lit ray and an occluded ray: a case set that lost them fails.
No test asserts a time."""
import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402

DEFAULT_LIGHT = (0.0, 60.0, 80.0)
LIGHT2 = (10.0, 40.0, 60.0)
# tests/test_oracle_slists.py LIGHTS: inside the model, on a cube-face diagonal (two of them), far away
INSIDE, DIAG_A, DIAG_B, FAR = (0.0, 0.0, 0.5), (5.0, 5.0, 99.5), (40.0, 40.0, 140.0), (-200.0, 150.0, 50.0)
CASES = [("tekkaman", 40, 24, DEFAULT_LIGHT), ("tekkaman", 128, 128, DEFAULT_LIGHT)] + \
        [(n, 96, 96, L) for n in ("box", "scene") for L in (INSIDE, DIAG_A, DIAG_B, FAR)]
KNOBS = ("RT_FUSED_CHUNK", "RT_BG_TIER", "RT_LANE_CHUNKS", "RT_BG_COST", "RT_BG_LAYERS", "RT_BG_STALE")

_scenes, _open, _ref = {}, {}, {}


@pytest.fixture(scope="module")
def renderers():
    yield _open
    for r in _open.values():
        r.close()
    _open.clear()
    for s in _scenes.values():
        s.close()
    _scenes.clear()


def _scene(name):
    if name not in _scenes:
        _scenes[name] = rt.Scene.load(scene_path(name))
    return _scenes[name]


def _renderer(name):
    if name not in _open:
        _open[name] = rt.Renderer(_scene(name))
    return _open[name]


def _oracle(po, name, w, h, light):
    """(colour, pid, counters) of the oracle's frame, once per case, left unchanged"""
    key = (name, w, h, light)
    if key not in _ref:
        s = _scene(name)
        bvh = s.bvh() + (s.bvh4(),) if s.info()["bvh4_nodes"] else None
        c, pid, _, k = po.rt_render(po.OracleScene(po.cgltrace.load(scene_path(name))),
                                    po.rt_params(w, h, shadows=True, light=light, nthreads=8),
                                    **({"bvh": bvh} if bvh else {}))
        c.setflags(write=False)
        pid.setflags(write=False)
        _ref[key] = (c, pid, k)
    return _ref[key]


def _sync_and_overlapped(r, ref):
    r.render()
    assert np.array_equal(r.framebuffer(), ref)
    for _ in range(4):
        r.start()
    r.wait()
    assert np.array_equal(r.framebuffer(), ref)
    assert np.array_equal(r.framebuffer_prev(), ref)


def _configure(r, m, w, h, light, knob, **env):
    for k in KNOBS:
        m.delenv(k, raising=False)
    m.setenv("RT_FUSED_CHUNK", "1" if knob else "0")
    for k, v in env.items():
        m.setenv(k, str(v))
    r.configure(w, h, shadows=True, light=light, counters=False)
    assert r.setup_stats()["fused_chunk"] == (1 if knob else 0)


@pytest.mark.parametrize("name,w,h,light", CASES)
def test_frames_equal_with_the_knob_on_and_off(oracle_lib, renderers, monkeypatch, name, w, h, light):
    r = _renderer(name)
    ref, _, k = _oracle(oracle_lib, name, w, h, light)
    ref2, _, _ = _oracle(oracle_lib, name, w, h, LIGHT2)
    for knob in (True, False):
        with monkeypatch.context() as m:
            # every tier mode, one and two chunks per wave
            for tier in (0, 1, 2):
                for per in (1, 2):
                    _configure(r, m, w, h, light, knob, RT_BG_TIER=tier, RT_LANE_CHUNKS=per)
                    assert r.setup_stats()["slist_on"] == 1
                    _sync_and_overlapped(r, ref)
            # the light moves under the default policy: stale lists, the queue and the BVH walk
            _configure(r, m, w, h, light, knob)
            _sync_and_overlapped(r, ref)
            r.set_light(LIGHT2)
            assert r.setup_stats()["slist_stale"] == 1
            _sync_and_overlapped(r, ref2)
            assert r.setup_stats()["slist_stale"] == 1
            # ... and with the lists rebuilt at once: the fused chunk under the new light
            r.set_list_policy(0)
            try:
                r.set_light(light)
                assert r.setup_stats()["slist_stale"] == 0
                _sync_and_overlapped(r, ref)
                r.set_light(LIGHT2)
                assert r.setup_stats()["slist_stale"] == 0
                _sync_and_overlapped(r, ref2)
            finally:
                r.set_list_policy(8)  # (rt_renderer_set_list_policy's default)
            # three shards
            fbs = []
            for i in range(3):
                for k_ in KNOBS[1:]:
                    m.delenv(k_, raising=False)
                r.configure(w, h, shadows=True, light=light, counters=False, shard_index=i, shard_count=3)
                assert r.setup_stats()["fused_chunk"] == (1 if knob else 0)
                r.render()
                for _ in range(3):
                    r.start()
                r.wait()
                fbs.append(r.framebuffer().copy())
            assert np.array_equal(rt.deinterleave_tiles(fbs, w, h), ref)
            # the ray counters of the plain image
            r.configure(w, h, shadows=True, light=light)
            r.render()
            st = r.stats()
            assert np.array_equal(r.framebuffer(), ref)
            for key in ("primary_rays", "shadow_rays", "occluded"):
                assert st[key] == k[key], (key, knob)


def test_other_configurations_do_not_carry_the_flag(renderers, monkeypatch):
    r = _renderer("tekkaman")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    r.configure(64, 64, shadows=True)
    assert r.setup_stats()["fused_chunk"] == 1  # the default
    r.configure(64, 64, shadows=False)
    assert r.setup_stats()["fused_chunk"] == 0
    r.configure(64, 64, shadows=True, path=True)
    assert r.setup_stats()["fused_chunk"] == 0
    monkeypatch.setenv("RT_FUSED_CHUNK", "0")
    r.configure(64, 64, shadows=True)
    assert r.setup_stats()["fused_chunk"] == 0


def test_cases_hold_every_kind(oracle_lib, renderers):
    po = oracle_lib
    full = mixed = lit = occluded = overhang = 0
    for name, w, h, light in CASES:
        _, pid, k = _oracle(po, name, w, h, light)
        sc = po.cgltrace.load(scene_path(name))
        layer = np.zeros(sc.num_prims + 1, bool)
        for dc in sc.drawcalls:
            if not dc.states["depth_test"]:
                layer[dc.prim_offset:dc.prim_offset + dc.prim_count] = True
        p = np.array(pid, np.int64)
        geo = (p >= 0) & ~layer[np.clip(p, 0, sc.num_prims)]  # a geometry winner: the pixel shoots a shadow ray
        for by in range(0, h, 8):
            for bx in range(0, w, 8):
                b = geo[by:by + 8, bx:bx + 8]
                n = int(b.sum())
                full += n == 64
                mixed += 0 < n < 64 and b.size == 64
                overhang += n > 0 and b.size < 64
        lit += k["shadow_rays"] - k["occluded"]
        occluded += k["occluded"]
    print(f"blocks full of rays {full}, mixed {mixed}, with rays over the image's edge {overhang}; "
          f"rays lit {lit}, occluded {occluded}")
    assert full > 0 and mixed > 0 and lit > 0 and occluded > 0
    # tekkaman at 128^2 alone holds the four kinds
    _, pid, k = _oracle(po, "tekkaman", 128, 128, DEFAULT_LIGHT)
    assert 0 < k["occluded"] < k["shadow_rays"]
