"""GPU test (MI355X) of the background tier of the primary + shadow frame
(kernels/rt_kernel.hip RT_BG_TIER, runtime/bg_tier.h, rt_app.cpp): a tiered
launch keeps its grid and carries the number of its geometry-tier workgroups
as its launch tag; those workgroups take the chunks of the tiles geometry
reaches, the workgroups behind them the chunks from 16 * heavy tiles on, which
have empty block lists and are rendered by a lean body (layers, shade, store).
The frame is the same, bit for bit.

On `tekkaman` and a sparse synthetic scene (three small triangles at the
image's centre) at 40x24 (two tiles, edges overhang), 96x64, 128^2 and 256^2
(tekkaman with a real mix of tiers):

* every chunk descriptor at or past 16 * heavy tiles has count 0;
* four frames started back to back leave both framebuffers equal to the
  oracle's, with the frame's task count, on the lane grid; with RT_BG_TIER=0
  the same frames, untiered;
* the same after set_light, with stale lists and with rebuilt lists, at
  RT_BG_COST extremes (many chunks per geometry wave and few background
  workgroups; one chunk per geometry wave and many chunks per background
  wave) and at RT_LANE_CHUNKS=3;
* with RT_BG_TIER=2 an instrumented synchronous frame is tiered and gives the
  oracle's counts;
* compact, sharded and path configurations and a scene whose tiles are all
  heavy report tier_groups == 0 and render as before.
No test asserts a time."""
import os

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402

SCENES = ("tekkaman", "sparse")
SIZES = [(40, 24), (96, 64), (128, 128), (256, 256)]
LIGHT2 = (10.0, 40.0, 60.0)

_scenes, _oracle = {}, {}


def _path(name, tmp_root):
    if name != "sparse":
        return scene_path(name)
    from synth_scene import make_scene
    p = os.path.join(str(tmp_root), "bg_tier_sparse.cgltrace.gz")
    if not os.path.exists(p):
        make_scene(p, 3, seed=5, size=0.04, spread=0.02)
    return p


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bg_tier")


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


def _tiles(w, h):
    return ((w + 31) // 32) * ((h + 31) // 32)


def _check_split(ss, st, w, h):
    """the split the setup reports against the frame's tiles: tiered exactly when both tiers
    have a tile, the geometry tier inside the grid with no wave left without a chunk"""
    heavy, tiles = ss["heavy_tiles"], _tiles(w, h)
    tg = ss["tier_groups"]
    if heavy == 0 or heavy == tiles:
        assert tg == 0 and ss["bg_first_chunk"] == 0
        return
    grid = ss["lane_grid"] or st["grid"]
    assert ss["bg_first_chunk"] == 16 * heavy
    assert 0 < tg < grid
    assert tg * (st["block"] // 64) <= 16 * heavy


def _frames(r, ref, n, want_grid=None, prev=True):
    for _ in range(n):
        r.start()
    r.wait()
    st = r.stats()
    assert st["tasks"] == st["num_tasks"]
    if want_grid:
        assert st["grid"] == want_grid
    assert np.array_equal(r.framebuffer(), ref)
    if prev:
        assert np.array_equal(r.framebuffer_prev(), ref)
    return st


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_tiered_frames_equal_oracle(oracle_lib, scene_dir, monkeypatch, name, w, h):
    s, r = _renderer(name, scene_dir)
    ref, _ = _oracle_frame(oracle_lib, name, scene_dir, w, h)
    ref2, _ = _oracle_frame(oracle_lib, name, scene_dir, w, h, LIGHT2)
    monkeypatch.delenv("RT_BG_TIER", raising=False)
    monkeypatch.delenv("RT_BG_COST", raising=False)
    r.configure(w, h, shadows=True, counters=False)
    r.set_list_policy(8)
    r.render()  # alone: the image's grid, untiered by default
    st0 = r.stats()
    assert np.array_equal(r.framebuffer(), ref)
    ss = r.setup_stats()
    _check_split(ss, st0, w, h)
    tiered = ss["tier_groups"] != 0
    if (w, h) == (256, 256):
        assert tiered  # (a real mix of tiers; the smaller frames as their tiles fall)
    # the descriptors behind the heavy tiles have empty lists
    cd = np.asarray(r.records("cdesc")).view(np.uint32).reshape(-1, 4)
    assert len(cd) == 16 * _tiles(w, h)
    assert not (cd[16 * ss["heavy_tiles"]:, 3] & 0xffff).any()
    lane_grid = ss["lane_grid"]
    assert lane_grid != 0
    _frames(r, ref, 4, lane_grid)
    # the light moves: stale lists (such frames keep the image's grid), then rebuilt lists
    r.set_light(LIGHT2)
    assert r.setup_stats()["slist_stale"] == 1
    _frames(r, ref2, 2, st0["grid"])
    r.set_list_policy(0)
    r.set_light(LIGHT2)
    _frames(r, ref2, 3, lane_grid)
    assert r.setup_stats()["tier_groups"] == ss["tier_groups"]
    r.set_list_policy(8)
    # untiered by the knob: the same frames
    with monkeypatch.context() as m:
        m.setenv("RT_BG_TIER", "0")
        r.configure(w, h, shadows=True, counters=False)
        s0 = r.setup_stats()
        assert s0["tier_groups"] == 0 and s0["lane_grid"] == lane_grid
        _frames(r, ref, 4, lane_grid)
    # the extremes of the split, stale lists tiered too, and three chunks per wave of the lane grid
    for env in ({"RT_BG_COST": "0.001"}, {"RT_BG_COST": "1000"}, {"RT_BG_STALE": "1"},
                {"RT_LANE_CHUNKS": "3"}, {"RT_LANE_CHUNKS": "3", "RT_BG_COST": "0.001"}):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            r.configure(w, h, shadows=True, counters=False)
            se = r.setup_stats()
            _check_split(se, st0, w, h)
            assert (se["tier_groups"] != 0) == tiered
            if tiered and env.get("RT_BG_COST") == "0.001":
                assert se["tier_groups"] == 1
            if tiered and env.get("RT_BG_COST") == "1000":
                grid = se["lane_grid"] or st0["grid"]
                assert se["tier_groups"] == min(grid - 1, 16 * se["heavy_tiles"] // (st0["block"] // 64))
            _frames(r, ref, 4, se["lane_grid"])
            if "RT_BG_STALE" in env:
                r.set_light(LIGHT2)
                assert r.setup_stats()["slist_stale"] == 1
                assert (r.setup_stats()["tier_groups"] != 0) == tiered
                _frames(r, ref2, 2, st0["grid"])


@pytest.mark.parametrize("w,h", [(96, 64), (256, 256)])
@pytest.mark.parametrize("name", SCENES)
def test_tiered_instrumented_frame_gives_the_oracle_counts(oracle_lib, scene_dir, monkeypatch, name, w, h):
    _, r = _renderer(name, scene_dir)
    ref, k = _oracle_frame(oracle_lib, name, scene_dir, w, h)
    monkeypatch.setenv("RT_BG_TIER", "2")
    r.configure(w, h, shadows=True, instrumented=True)
    ss = r.setup_stats()
    assert ss["tier_groups"] != 0 and ss["lane_grid"] == 0
    r.render()
    st = r.stats()
    assert np.array_equal(r.framebuffer(), ref)
    assert st["tasks"] == st["num_tasks"]
    assert st["primary_rays"] == k["primary_rays"] == w * h
    for key in ("shadow_rays", "occluded", "geometry_hits", "layer_tests", "shaded", "texel_bytes",
                "tri_tests"):
        assert st[key] == k[key], key
    # and the plain counters of a frame rendered alone
    r.configure(w, h, shadows=True, counters=True)
    assert r.setup_stats()["tier_groups"] != 0
    r.render()
    st = r.stats()
    assert np.array_equal(r.framebuffer(), ref)
    assert st["primary_rays"] == w * h and st["shadow_rays"] == k["shadow_rays"]
    assert st["occluded"] == k["occluded"] and st["tasks"] == st["num_tasks"]


@pytest.mark.parametrize("kw", [dict(compact=True), dict(shard_count=3, shard_index=1, compact=True),
                                dict(path=True, bounces=2)],
                         ids=["compact", "shard", "path"])
def test_untiered_configurations_render_as_before(scene_dir, monkeypatch, kw):
    w, h = 256, 256
    _, r = _renderer("tekkaman", scene_dir)
    frames = []
    for mode in ("0", "2"):
        monkeypatch.setenv("RT_BG_TIER", mode)
        r.configure(w, h, shadows=True, **kw)
        ss = r.setup_stats()
        assert ss["tier_groups"] == 0 and ss["bg_first_chunk"] == 0
        r.render()
        r.start()
        r.start()
        r.wait()
        frames.append(r.framebuffer().copy())
    assert np.array_equal(frames[0], frames[1])


def test_a_frame_whose_tiles_are_all_heavy_is_untiered(oracle_lib, scene_dir, monkeypatch):
    """tekkaman at 32x32: one tile, and geometry reaches it"""
    w, h = 32, 32
    _, r = _renderer("tekkaman", scene_dir)
    ref, _ = _oracle_frame(oracle_lib, "tekkaman", scene_dir, w, h)
    monkeypatch.setenv("RT_BG_TIER", "2")
    r.configure(w, h, shadows=True, counters=False)
    ss = r.setup_stats()
    assert ss["heavy_tiles"] == _tiles(w, h) == 1
    assert ss["tier_groups"] == 0 and ss["bg_first_chunk"] == 0
    r.render()
    assert np.array_equal(r.framebuffer(), ref)
    _frames(r, ref, 4, ss["lane_grid"])
