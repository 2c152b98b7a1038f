"""GPU test (MI355X) of the overlapped frames' grid (vortex_hip.h
vx_hip_set_launch_grid, rt_app.cpp lane_grid): a primary + shadow frame that
goes to a launch lane (rt_render_start, frames overlapping) launches the
workgroups that give every wave two chunks, not the image's oversubscribed
grid; vx_spawn deals chunk c to wave c mod W for whatever grid it finds, so
the frame is the same.  A frame rendered alone (rt_render) keeps the image's
grid, and the grid request is for one launch only.

On `tekkaman`, a sparse synthetic scene (three small triangles at the image's
centre) and `triangle` (no geometry: the generic image), at 8x8, 40x24 (edge
tiles overhang), 96x64 and 128^2:

* setup_stats()["lane_grid"] is ceil(chunks / (2 * waves per workgroup)), and
  stats()["grid"] of a started frame is that grid, of a synchronous frame
  before and after it the image's;
* four frames started back to back leave both framebuffers equal to the
  oracle's, and the task count is the frame's pixel-task count;
* after set_light the started frames equal the oracle's for the new light: on
  the image's grid while the light-space lists are stale (their shadow rays
  walk the BVH), on the lane grid again once the lists are rebuilt;
* env RT_LANE_CHUNKS=3 gives ceil(chunks / (3 * waves)) and the same frames,
  RT_LANE_CHUNKS=1 the image's grid;
* configurations that never go to a lane (compact, shards, counters,
  instrumented) have no lane grid: their started frames run the image's grid,
  with the oracle's counts.
No test asserts a time."""
import os

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402

SCENES = ("tekkaman", "sparse", "triangle")
SIZES = [(8, 8), (40, 24), (96, 64), (128, 128)]
LIGHT2 = (10.0, 40.0, 60.0)

_scenes, _oracle = {}, {}


def _path(name, tmp_root):
    if name != "sparse":
        return scene_path(name)
    from synth_scene import make_scene
    p = os.path.join(str(tmp_root), "lane_grid_sparse.cgltrace.gz")
    if not os.path.exists(p):
        make_scene(p, 3, seed=5, size=0.04, spread=0.02)
    return p


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("lane_grid")


def _renderer(name, scene_dir):
    if name not in _scenes:
        s = rt.Scene.load(_path(name, scene_dir))
        _scenes[name] = (s, rt.Renderer(s))
    return _scenes[name]


def _oracle_frame(po, name, scene_dir, w, h, light=None):
    """the oracle's frame and counts, once per (scene, size, light), left unchanged"""
    key = (name, w, h, light)
    if key not in _oracle:
        s, _ = _renderer(name, scene_dir)
        kw = {} if light is None else {"light": light}
        bvh = s.bvh() + (s.bvh4(),) if s.info()["bvh4_nodes"] else None
        c, _, _, k = po.rt_render(po.OracleScene(po.cgltrace.load(_path(name, scene_dir))),
                                  po.rt_params(w, h, shadows=True, nthreads=8, **kw),
                                  **({"bvh": bvh} if bvh else {}))
        c.setflags(write=False)
        _oracle[key] = (c, k)
    return _oracle[key]


def _lane_grid(st, per):
    """the grid a laned frame must launch: every wave `per` chunks, never above the image's"""
    chunks, waves = (st["num_tasks"] + 63) // 64, st["block"] // 64
    g = max(1, (chunks + per * waves - 1) // (per * waves))
    return g if g < st["grid"] else 0


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_overlapped_frames_on_their_grid_equal_oracle(oracle_lib, scene_dir, monkeypatch, name, w, h):
    s, r = _renderer(name, scene_dir)
    ref, _ = _oracle_frame(oracle_lib, name, scene_dir, w, h)
    r.configure(w, h, shadows=True, counters=False)
    r.set_list_policy(8)
    r.render()  # alone: the image's grid
    st0 = r.stats()
    assert np.array_equal(r.framebuffer(), ref)
    want = _lane_grid(st0, 2)
    assert want != 0  # (these frames have far fewer chunks than the image's grid has waves)
    assert r.setup_stats()["lane_grid"] == want
    for _ in range(4):
        r.start()
    r.wait()
    st = r.stats()
    assert st["grid"] == want and st["block"] == st0["block"]
    assert st["tasks"] == st["num_tasks"] == st0["tasks"]
    assert np.array_equal(r.framebuffer(), ref)
    assert np.array_equal(r.framebuffer_prev(), ref)
    r.render()  # the request was the started frames' only
    assert r.stats()["grid"] == st0["grid"]
    assert np.array_equal(r.framebuffer(), ref)
    # the light moves: the grid stays, the frame is the new light's
    ref2, _ = _oracle_frame(oracle_lib, name, scene_dir, w, h, LIGHT2)
    # (its lists are stale at first -- shadow rays walk the BVH -- and such frames keep the image's grid)
    r.set_list_policy(8)  # (the renderer's default; the renderer is shared between the cases)
    r.set_light(LIGHT2)
    stale = r.setup_stats()["slist_stale"]
    assert stale == (1 if s.info()["num_geometry"] else 0)  # (no geometry: no shadow lists at all)
    r.start()
    r.start()
    r.wait()
    assert r.stats()["grid"] == (st0["grid"] if stale else want)
    assert np.array_equal(r.framebuffer(), ref2)
    assert np.array_equal(r.framebuffer_prev(), ref2)
    # with the lists rebuilt at once: the frame behind the rebuild is an ordinary launch, the next on a lane
    r.set_list_policy(0)
    r.set_light(LIGHT2)
    r.start()
    r.start()
    r.start()
    r.wait()
    assert r.stats()["grid"] == want and r.setup_stats()["lane_grid"] == want
    assert np.array_equal(r.framebuffer(), ref2)
    assert np.array_equal(r.framebuffer_prev(), ref2)
    for per in (3, 1):
        with monkeypatch.context() as m:
            m.setenv("RT_LANE_CHUNKS", str(per))
            r.configure(w, h, shadows=True, counters=False)
            g = _lane_grid(st0, per) if per > 1 else 0
            assert r.setup_stats()["lane_grid"] == g
            for _ in range(3):
                r.start()
            r.wait()
            assert r.stats()["grid"] == (g or st0["grid"])
            assert np.array_equal(r.framebuffer(), ref)
            assert np.array_equal(r.framebuffer_prev(), ref)
    r.set_list_policy(8)


@pytest.mark.parametrize("kw", [dict(compact=True), dict(shard_count=3, shard_index=1, compact=True),
                                dict(counters=True), dict(instrumented=True)],
                         ids=["compact", "shard", "counters", "instrumented"])
def test_frames_off_the_lanes_keep_the_image_grid(oracle_lib, scene_dir, kw):
    w, h = 96, 64
    _, r = _renderer("tekkaman", scene_dir)
    ref, k = _oracle_frame(oracle_lib, "tekkaman", scene_dir, w, h)
    r.configure(w, h, shadows=True, **{"counters": True, **kw})
    assert r.setup_stats()["lane_grid"] == 0
    r.render()
    st0, fb0 = r.stats(), r.framebuffer().copy()
    for _ in range(3):
        r.start()
    r.wait()
    st = r.stats()
    assert st["grid"] == st0["grid"]
    assert np.array_equal(r.framebuffer(), fb0)
    for key in ("tasks", "primary_rays", "shadow_rays", "occluded", "tri_tests", "layer_tests", "shaded"):
        assert st[key] == st0[key], key
    if "shard_count" not in kw:
        assert st["shadow_rays"] == k["shadow_rays"] and st["occluded"] == k["occluded"]
    if not kw.get("compact"):
        assert np.array_equal(fb0, ref)
