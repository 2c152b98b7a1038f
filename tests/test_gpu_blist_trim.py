"""The block lists trimmed to their winners on the device (kernels/rt_btrim_kernel.hip, one launch per
configure) and the frames that scan them.

* device btrim / btidx equal the host restatement (records btrim_host / btidx_host, app/setup.cpp
  TrimBlockLists) byte for byte and the oracle's winners (blist_trim_cases.expected), whole frames and
  3 shards, linear and compact; blist / bidx stay the oracle's untrimmed lists; setup_stats counts them;
* the host setup builds the same arrays;
* the frame equals the oracle's, with the oracle's shadow_rays and occluded; an instrumented configure
  in the same renderer scans the untrimmed lists -- the oracle's tri_tests -- and shows no trim;
* a 64^2 2-bounce path frame equals the oracle;
* set_light leaves both arrays' bytes alone and the next frame is the oracle's for the new light;
* env RT_BLIST_TRIM=0: no trimmed arrays, the same frame."""
import os

import numpy as np
import pytest

from blist_trim_cases import CASES, IDS, check_trim, expected, oscene
from conftest import scene_path

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402

LIGHT2 = (20.0, 50.0, 85.0)


def _trim_records(r):
    return r.records("btidx"), r.records("btrim")


def _check_device(r, name, w, h, index=0, count=1):
    oidx, oent, _, _ = expected(name, w, h, index, count)
    assert np.array_equal(r.records("bidx"), oidx) and np.array_equal(r.records("blist")[:-3], oent)
    btidx, btrim = _trim_records(r)
    assert np.array_equal(btidx, r.records("btidx_host")), "btidx differs from the host restatement"
    assert np.array_equal(btrim, r.records("btrim_host")), "btrim differs from the host restatement"
    kept, blocks, _ = check_trim(btidx, btrim, name, w, h, index, count)
    st = r.setup_stats()
    assert (st["btrim_entries"], st["btrim_blocks"]) == (kept, blocks), st
    assert st["blist_entries"] == len(oent)
    return kept, blocks


@pytest.mark.parametrize("name,w,h,entries,kept,blocks,kblocks,longest", CASES, ids=IDS)
def test_device_trim_equals_host_and_oracle(oracle_lib, name, w, h, entries, kept, blocks, kblocks, longest):
    s = rt.Scene.load(scene_path(name))
    r = rt.Renderer(s)
    for compact in (False, True):
        r.configure(w, h, shadows=True, counters=False, compact=compact)
        assert r.setup_stats()["device"] == 1
        assert _check_device(r, name, w, h) == (kept, kblocks)
    tot = np.zeros(2, np.int64)
    for index in range(3):
        r.configure(w, h, shadows=True, counters=False, shard_index=index, shard_count=3)
        if len(expected(name, w, h, index, 3)[0]) == 0:  # a shard without a tile builds no lists
            assert r.setup_stats()["blist_blocks"] == 0 and r.setup_stats()["btrim_entries"] == 0
            continue
        tot += _check_device(r, name, w, h, index, 3)
    assert tuple(tot) == (kept, kblocks)
    r.configure(w, h, shadows=True, counters=False, host_setup=True)
    assert r.setup_stats()["device"] == 0
    assert _check_device(r, name, w, h) == (kept, kblocks)
    r.close()
    s.close()


@pytest.mark.parametrize("name,w,h", [c[:3] for c in CASES], ids=IDS)
def test_frames_equal_oracle_and_instrumented_keeps_the_lists(oracle_lib, name, w, h):
    po = oracle_lib
    s = rt.Scene.load(scene_path(name))
    r = rt.Renderer(s)
    c, _, _, k = po.rt_render(oscene(name), po.rt_params(w, h, shadows=True, nthreads=8), bvh=s.bvh() + (s.bvh4(),))
    r.configure(w, h, shadows=True)
    assert r.setup_stats()["btrim_entries"] > 0
    r.render()
    st = r.stats()
    assert np.array_equal(r.framebuffer(), c)
    assert st["shadow_rays"] == k["shadow_rays"] and st["occluded"] == k["occluded"]
    # overlapped frames (the timed path) read the same arrays
    r.configure(w, h, shadows=True, counters=False)
    for _ in range(3):
        r.start()
    r.wait()
    assert np.array_equal(r.framebuffer(), c)
    r.configure(w, h, shadows=True, instrumented=True)
    su = r.setup_stats()
    assert su["blist_blocks"] > 0 and su["btrim_entries"] == 0 and su["btrim_blocks"] == 0
    with pytest.raises(RuntimeError):
        r.records("btrim")
    r.render()
    st = r.stats()
    assert np.array_equal(r.framebuffer(), c)
    for key in ("tri_tests", "layer_tests", "shadow_rays", "occluded"):
        assert st[key] == k[key], key
    r.close()
    s.close()


def test_path_frame_equals_oracle(oracle_lib):
    po = oracle_lib
    s = rt.Scene.load(scene_path("tekkaman"))
    r = rt.Renderer(s)
    r.configure(64, 64, path=True, bounces=2)
    assert r.setup_stats()["btrim_entries"] > 0
    r.render()
    c, _, _, k = po.rt_render(oscene("tekkaman"), po.rt_params(64, 64, path=True, bounces=2, nthreads=8),
                              bvh=s.bvh() + (s.bvh4(),))
    assert np.array_equal(r.framebuffer(), c)
    st = r.stats()
    assert st["shadow_rays"] == k["shadow_rays"] and st["bounce_rays"] == k["bounce_rays"]
    r.close()
    s.close()


def test_set_light_leaves_the_trim_alone(oracle_lib):
    po = oracle_lib
    name, w, h = CASES[1][:3]
    s = rt.Scene.load(scene_path(name))
    r = rt.Renderer(s)
    r.configure(w, h, shadows=True)
    r.set_list_policy(0)
    r.render()
    before = [a.tobytes() for a in _trim_records(r)]
    launches = r.setup_stats()["launches"]
    r.set_light(LIGHT2)
    r.render()
    assert [a.tobytes() for a in _trim_records(r)] == before
    assert r.setup_stats()["launches"] == launches  # (the configure's: set_light's chain builds no trim)
    c, _, _, k = po.rt_render(oscene(name), po.rt_params(w, h, shadows=True, light=LIGHT2, nthreads=8),
                              bvh=s.bvh() + (s.bvh4(),))
    st = r.stats()
    assert np.array_equal(r.framebuffer(), c)
    assert st["shadow_rays"] == k["shadow_rays"] and st["occluded"] == k["occluded"]
    r.close()
    s.close()


def test_trim_off_by_env(oracle_lib):
    po = oracle_lib
    name, w, h = CASES[1][:3]
    s = rt.Scene.load(scene_path(name))
    r = rt.Renderer(s)
    r.configure(w, h, shadows=True)
    on = r.setup_stats()["launches"]
    os.environ["RT_BLIST_TRIM"] = "0"
    try:
        r.configure(w, h, shadows=True)
        su = r.setup_stats()
        assert su["blist_blocks"] > 0 and su["btrim_entries"] == 0 and su["launches"] == on - 1
        with pytest.raises(RuntimeError):
            r.records("btrim")
        with pytest.raises(RuntimeError):
            r.records("btidx")
        r.render()
        c, _, _, k = po.rt_render(oscene(name), po.rt_params(w, h, shadows=True, nthreads=8),
                                  bvh=s.bvh() + (s.bvh4(),))
        st = r.stats()
        assert np.array_equal(r.framebuffer(), c)
        assert st["shadow_rays"] == k["shadow_rays"] and st["occluded"] == k["occluded"]
    finally:
        del os.environ["RT_BLIST_TRIM"]
    r.close()
    s.close()
