"""GPU test (MI355X) of the background-layer table (rt_common.h rt_bglayer_t;
kernels/rt_setup.hip RTS_BGLAYER builds it at configure, kernels/rt_kernel.hip
RT_BG_LAYERS reads it in the background tier), on the scenes and sizes of
tests/test_bg_layers_cpu.py:

* records("bglayer") -- the device's table -- equals records("bglayer_host")
  byte for byte and the oracle's per-pixel pids under the device's own work
  order (every chunk behind the first background chunk is a background block;
  the non-zero entries are exactly the uniform full ones), and set_light
  leaves it as it is; an untiered configuration, RT_BG_LAYERS=0, RT_BG_TIER=0
  and an instrumented configuration have no table; word 1 is the drawcall
  word of the device's own primitive record;
* four frames started back to back leave both framebuffers equal to the
  oracle's with the table on, with RT_BG_LAYERS=0, at the RT_BG_COST extremes,
  and after set_light with stale lists (untiered by default, and tiered --
  through the table -- under RT_BG_STALE=1) and with rebuilt lists;
* the RT_BG_TIER=2 instrumented frame (which keeps the layer loop) still gives
  the oracle's layer_tests, shaded and texel_bytes.
No test asserts a time."""
import numpy as np
import pytest

import test_bg_layers_cpu as cpu

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402

LIGHT2 = (10.0, 40.0, 60.0)

_scenes, _frames_ref = {}, {}


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    yield tmp_path_factory.mktemp("bg_layers_gpu")
    for s, r in _scenes.values():  # the module's renderers and scenes
        r.close()
        s.close()
    _scenes.clear()


def _renderer(name, scene_dir):
    if name not in _scenes:
        s = rt.Scene.load(cpu.scene_file(name, scene_dir))
        _scenes[name] = (s, rt.Renderer(s))
    return _scenes[name]


def _oracle_frame(po, name, scene_dir, w, h, light=None):
    key = (name, w, h, light)
    if key not in _frames_ref:
        s, _ = _renderer(name, scene_dir)
        kw = {} if light is None else {"light": light}
        bvh = s.bvh() + (s.bvh4(),) if s.info()["bvh4_nodes"] else None
        c, _, _, k = po.rt_render(po.OracleScene(po.cgltrace.load(cpu.scene_file(name, scene_dir))),
                                  po.rt_params(w, h, shadows=True, nthreads=8, **kw),
                                  **({"bvh": bvh} if bvh else {}))
        c.setflags(write=False)
        _frames_ref[key] = (c, k)
    return _frames_ref[key]


def _frames(r, ref, n=4):
    for _ in range(n):
        r.start()
    r.wait()
    st = r.stats()
    assert st["tasks"] == st["num_tasks"]
    assert np.array_equal(r.framebuffer(), ref)
    assert np.array_equal(r.framebuffer_prev(), ref)


def _no_table(r):
    for name in ("bglayer", "bglayer_host"):
        with pytest.raises(rt.RtError, match="not present"):
            r.records(name)


@pytest.mark.parametrize("w,h", cpu.SIZES)
@pytest.mark.parametrize("name", cpu.SCENES)
def test_table_and_frames(oracle_lib, scene_dir, monkeypatch, name, w, h):
    _, r = _renderer(name, scene_dir)
    ref, _ = _oracle_frame(oracle_lib, name, scene_dir, w, h)
    ref2, _ = _oracle_frame(oracle_lib, name, scene_dir, w, h, LIGHT2)
    pid, layers, pdc = cpu.oracle_pids(oracle_lib, name, scene_dir, w, h)
    for k in ("RT_BG_TIER", "RT_BG_COST", "RT_BG_LAYERS"):
        monkeypatch.delenv(k, raising=False)
    r.configure(w, h, shadows=True, counters=False)
    r.set_list_policy(8)
    ss = r.setup_stats()
    tiered = ss["tier_groups"] != 0
    if (w, h) == (256, 256):
        assert tiered
    if tiered:
        first = ss["bg_first_chunk"]
        tab = r.records("bglayer")
        assert tab.tobytes() == r.records("bglayer_host").tobytes()
        order = r.records("order").ravel()
        exp, uniform, background = cpu.expected(pid, layers, pdc, w, h, order, first)
        assert None not in exp  # behind the heavy tiles: no geometry pixel
        assert cpu.check_table(tab, exp) == uniform
        if (w, h) == (256, 256):
            assert 0 < uniform
            assert uniform < background or name == "sparse"
        # word 1: the drawcall word (30) of the device's own record of that primitive
        prims = r.records("prims").view(np.uint32)
        one = (tab[:, 0] != 0) & (tab[:, 0] != cpu.NONE)
        assert np.array_equal(tab[one, 1], prims[tab[one, 0] - 1, 30])
    else:
        _no_table(r)
    _frames(r, ref)
    # the light moves: stale lists, then rebuilt lists; the table stays
    r.set_light(LIGHT2)
    assert r.setup_stats()["slist_stale"] == 1
    _frames(r, ref2)
    r.set_list_policy(0)
    r.set_light(LIGHT2)
    _frames(r, ref2)
    if tiered:
        assert r.records("bglayer").tobytes() == tab.tobytes()
    r.set_list_policy(8)
    # without the table, at the extremes of the split, and with stale-list frames tiered too
    for env in ({"RT_BG_LAYERS": "0"}, {"RT_BG_COST": "0.001"}, {"RT_BG_COST": "1000"}, {"RT_BG_STALE": "1"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            r.configure(w, h, shadows=True, counters=False)
            assert (r.setup_stats()["tier_groups"] != 0) == tiered
            if "RT_BG_LAYERS" in env or not tiered:
                _no_table(r)
            else:
                assert r.records("bglayer").tobytes() == tab.tobytes()
            _frames(r, ref)
            if "RT_BG_STALE" in env:  # the light moves: these stale-list frames run the tier, on the table
                r.set_light(LIGHT2)
                assert r.setup_stats()["slist_stale"] == 1
                assert (r.setup_stats()["tier_groups"] != 0) == tiered
                _frames(r, ref2)
                if tiered:
                    assert r.records("bglayer").tobytes() == tab.tobytes()
    # never tiered: no table is built
    with monkeypatch.context() as m:
        m.setenv("RT_BG_TIER", "0")
        r.configure(w, h, shadows=True, counters=False)
        _no_table(r)
        _frames(r, ref)


@pytest.mark.parametrize("w,h", [(96, 64), (256, 256)])
@pytest.mark.parametrize("name", cpu.SCENES)
def test_instrumented_tiered_frame_keeps_the_oracle_counts(oracle_lib, scene_dir, monkeypatch, name, w, h):
    _, r = _renderer(name, scene_dir)
    ref, k = _oracle_frame(oracle_lib, name, scene_dir, w, h)
    monkeypatch.setenv("RT_BG_TIER", "2")
    monkeypatch.delenv("RT_BG_LAYERS", raising=False)
    r.configure(w, h, shadows=True, instrumented=True)
    assert r.setup_stats()["tier_groups"] != 0
    _no_table(r)  # the instrumented image keeps the layer loop
    r.render()
    st = r.stats()
    assert np.array_equal(r.framebuffer(), ref)
    for key in ("layer_tests", "shaded", "texel_bytes", "primary_rays"):
        assert st[key] == k[key], key
    # and the plain image's frame rendered alone, tiered, through the table
    r.configure(w, h, shadows=True, counters=True)
    assert r.setup_stats()["tier_groups"] != 0
    r.render()
    assert np.array_equal(r.framebuffer(), ref)
