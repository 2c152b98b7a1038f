"""GPU tests of the per-pixel visibility records (vx_rt.h rt_render_aov_start; image
rt_aov, kernels/rt_aov_kernel.hip) against the untouched oracle, bit for bit.

Every field of a record is something the oracle already returns and no GPU test
compared before: `pid` and `t` are rt_render's per-pixel outputs, the depth bits
are raster_render's depth words & 0xffffff, RT_AOV_GEOM is "the oracle's pid is a
primitive of a depth-tested drawcall", the RT_AOV_SHADOW_RAY pixels number the
oracle's shadow_rays, and bit i of the mask is "the oracle's frame under light i
differs from its unshadowed frame" (a shadowed colour is c >> 1 per channel, so
the frames differ wherever the unshadowed RGB is not zero); the masks' set bits
number the oracle frames' occluded counters.  `t` is compared by bit pattern;
values that are NaN on both sides count as equal (a 0/0 has another sign bit on
the host than on the device).  No reference exists for this row."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import scene_path
from test_gpu_light import LIGHTS
from test_gpu_lights import SIXTEEN

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, rt  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(8, 8), (32, 32), (128, 128), (200, 136)]
SCENES = ["tekkaman", "box", "triangle"]
_scenes = {}
_frames = {}
_state = {}


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def scene(po, name):
    """(oracle scene, its BVH or None, bool per pid: a primitive of a depth-tested drawcall)"""
    if name not in _scenes:
        sc = po.cgltrace.load(scene_path(name))
        tested = np.zeros(max(sc.num_prims, 1), bool)
        for dc in sc.drawcalls:
            tested[dc.prim_offset:dc.prim_offset + dc.prim_count] = bool(dc.states["depth_test"])
        s = rt.Scene.load(scene_path(name))
        bvh = s.bvh() + (s.bvh4(),) if s.info()["bvh_nodes"] else None
        s.close()
        _scenes[name] = (po.OracleScene(sc), bvh, tested)
    return _scenes[name]


def frame(po, name, w, h, light, shadows=True):
    """(colour, pid, t, counters) of the oracle's single-light frame; computed once, left unchanged"""
    key = (name, w, h, tuple(light) if shadows else None)
    if key not in _frames:
        osc, bvh, _ = scene(po, name)
        c, pid, t, k = po.rt_render(osc, po.rt_params(w, h, shadows=shadows, light=light, nthreads=8), bvh=bvh)
        for a in (c, pid, t):
            a.setflags(write=False)
        _frames[key] = (c, pid, t, k)
    return _frames[key]


def depth_words(po, name, w, h):
    key = (name, w, h, "depth")
    if key not in _frames:
        d = po.raster_render(scene(po, name)[0], w, h)[1] & np.uint32(0xFFFFFF)
        d.setflags(write=False)
        _frames[key] = d
    return _frames[key]


def popcount(m):
    m = np.asarray(m, np.uint32)
    return sum(((m >> np.uint32(i)) & np.uint32(1)).astype(np.int64) for i in range(32))


def check(po, rec, name, w, h, lights, shadows=True):
    """every field of the [H, W] records against the oracle; returns the masks' popcounts"""
    lights = list(lights)
    K = len(lights)
    _, _, tested = scene(po, name)
    plain, pid, t, k0 = frame(po, name, w, h, LIGHTS[0], shadows=False)
    assert rec.shape == (h, w) and rec.dtype == rt.AOV_DTYPE
    assert np.array_equal(rec["pid"], pid), f"{int((rec['pid'] != pid).sum())} pids differ"
    got_t, want_t = rec["t"], t
    same = (got_t.view(np.uint32) == want_t.view(np.uint32)) | (np.isnan(got_t) & np.isnan(want_t))
    assert same.all(), f"{int((~same).sum())} plane t differ"
    df = rec["depth_flags"]
    assert np.array_equal(df & np.uint32(0xFFFFFF), depth_words(po, name, w, h))
    assert not (df >> np.uint32(26)).any()
    geom = (pid >= 0) & tested[np.maximum(pid, 0)]
    assert np.array_equal((df & np.uint32(rt.RT_AOV_GEOM)) != 0, geom)
    assert int(geom.sum()) == k0["geometry_hits"]
    sray = (df & np.uint32(rt.RT_AOV_SHADOW_RAY)) != 0
    mask = rec["light_mask"]
    pc = popcount(mask)
    if not shadows:
        assert not sray.any() and not mask.any()
        return pc
    ks = [frame(po, name, w, h, L)[3] for L in lights]
    assert all(k["shadow_rays"] == ks[0]["shadow_rays"] for k in ks)
    assert int(sray.sum()) == ks[0]["shadow_rays"], (int(sray.sum()), ks[0]["shadow_rays"])
    # (the definition: shadow rays start at a geometry hit whose plane t is finite and > 0)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(sray, geom & (t > 0) & np.isfinite(t))
    assert not mask[~sray].any()
    assert not (mask >> np.uint32(K)).any()
    assert int(pc.sum()) == sum(k["occluded"] for k in ks), (int(pc.sum()), [k["occluded"] for k in ks])
    known = (plain & np.uint32(0xFFFFFF)) != 0
    for i, L in enumerate(lights):
        differs = frame(po, name, w, h, L)[0] != plain
        bit = ((mask >> np.uint32(i)) & np.uint32(1)) != 0
        assert np.array_equal(bit[known], differs[known]), f"light {i}: {int((bit != differs)[known].sum())} bits differ"
    return pc


def mean_of_frames(po, name, w, h, lights):
    fr = [frame(po, name, w, h, L)[0] for L in lights]
    n = len(fr)
    out = fr[0] & np.uint32(0xFF000000)
    for sh in (16, 8, 0):
        tot = sum(((c >> np.uint32(sh)) & np.uint32(0xFF)).astype(np.uint64) for c in fr)
        out = out | (((2 * tot + n) // (2 * n)).astype(np.uint32) << np.uint32(sh))
    return out


def renderer(name="tekkaman", key=""):
    if name + key not in _state:
        s = rt.Scene.load(scene_path(name))
        _state[name + key] = (s, rt.Renderer(s))
    return _state[name + key][1]


# ---- fields against the oracle, shadows on ---------------------------------

@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("name", SCENES)
def test_fields_equal_oracle(po, name, w, h):
    r = renderer(name)
    r.configure(w, h, shadows=True, light=LIGHTS[0])
    rec = r.aov()
    check(po, rec, name, w, h, LIGHTS[:1])
    if name == "triangle":  # a layer only: no tree, no shadow ray, no geometry anywhere
        assert not (rec["depth_flags"] & np.uint32(rt.RT_AOV_GEOM | rt.RT_AOV_SHADOW_RAY)).any()
        assert (rec["depth_flags"] == 0xFFFFFF).all() and not rec["light_mask"].any() and not rec["t"].any()
        assert set(np.unique(rec["pid"])) <= {-1, 0}


# ---- the mask ----------------------------------------------------------------

@pytest.mark.parametrize("lights", [LIGHTS[:1], LIGHTS[:2], LIGHTS[:3], SIXTEEN], ids=["K1", "K2", "K3", "K16"])
def test_mask(po, lights):
    w = h = 128
    K = len(lights)
    r = renderer()
    r.configure(w, h, shadows=True, light=lights[0])
    if K > 1:
        r.set_lights(lights)
    rec = r.aov()
    pc = check(po, rec, "tekkaman", w, h, lights)
    mixed = int(((pc > 0) & (pc < K)).sum())
    print(f"K={K}: {mixed} pixels with 0 < popcount < K, {int((pc > 0).sum())} with a set bit")
    if K > 1:
        assert mixed >= 100, f"only {mixed} pixels with 0 < popcount < K"
    plain = frame(po, "tekkaman", w, h, LIGHTS[0], shadows=False)[0]
    got = rt.aov_relight(plain, rec["light_mask"], K)
    want = mean_of_frames(po, "tekkaman", w, h, lights)
    assert np.array_equal(got, want), f"{int((got != want).sum())} pixels differ"
    if K > 1:  # and the device's own K-light frame
        r.render()
        assert np.array_equal(r.framebuffer(), got)


# ---- other configurations ----------------------------------------------------

def test_bvh_walk(po):
    r = renderer()
    r.configure(200, 136, shadows=True, light=LIGHTS[1], bvh_walk=True)
    check(po, r.aov(), "tekkaman", 200, 136, [LIGHTS[1]])


def test_host_setup(po):
    r = renderer()
    r.configure(200, 136, shadows=True, light=LIGHTS[1], host_setup=True)
    check(po, r.aov(), "tekkaman", 200, 136, [LIGHTS[1]])
    r.set_lights(LIGHTS[:2])  # no lists under the host setup: both lights walk the BVH
    assert [i["slist_on"] for i in r.lights_info()] == [0, 0]
    check(po, r.aov(), "tekkaman", 200, 136, LIGHTS[:2])


def _child(out_path):
    """RT_BLOCK_LISTS=0 RT_SHADOW_LISTS=0 (this process): one light, then three"""
    s = rt.Scene.load(scene_path("tekkaman"))
    r = rt.Renderer(s)
    r.configure(200, 136, shadows=True, light=LIGHTS[1])
    st = r.setup_stats()
    if st["blist_blocks"] != 0 or st["slist_on"] != 0:
        raise SystemExit(f"lists still built: {st}")
    one = r.aov()
    r.set_lights(LIGHTS[:3])
    np.savez(out_path, one=one, three=r.aov())
    r.close()
    s.close()


def test_no_lists(po, tmp_path):
    """primary visibility by the packet walk of the tree (the depth word recomputed for the
    winner), every shadow ray by the BVH packet walk"""
    out = str(tmp_path / "aov.npz")
    env = dict(os.environ, RT_BLOCK_LISTS="0", RT_SHADOW_LISTS="0", SKYBOX_RT_NO_TORCH="1",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.load(out)
    check(po, got["one"], "tekkaman", 200, 136, [LIGHTS[1]])
    check(po, got["three"], "tekkaman", 200, 136, LIGHTS[:3])


def test_two_compact_shards(po):
    w, h = 200, 136
    r = renderer()
    lights = LIGHTS[:2]
    parts = []
    for i in range(2):
        r.configure(w, h, shadows=True, light=lights[0], shard_index=i, shard_count=2)
        r.set_lights(lights)
        rec = r.aov()
        assert rec.shape == (r.stats()["local_tiles"] * 1024,)
        parts.append(rec.copy())
    whole = np.zeros((h, w), rt.AOV_DTYPE)
    words = whole.view(np.uint32).reshape(h, w, 4)
    for j in range(4):
        words[:, :, j] = rt.deinterleave_tiles([p.view(np.uint32).reshape(-1, 4)[:, j] for p in parts], w, h)
    check(po, whole, "tekkaman", w, h, lights)
    # one compact shard alone (RT_RENDER_COMPACT): every tile, in task order
    r.configure(w, h, shadows=True, light=lights[0], compact=True)
    rec = r.aov()
    for j in range(4):
        words[:, :, j] = rt.deinterleave_tiles([rec.view(np.uint32).reshape(-1, 4)[:, j]], w, h)
    check(po, whole, "tekkaman", w, h, lights[:1])


def test_without_shadows(po):
    r = renderer()
    r.configure(200, 136, shadows=False)
    check(po, r.aov(), "tekkaman", 200, 136, [], shadows=False)


def test_moved_light_under_the_deferred_policy(po):
    """set_light under the default policy leaves the lists stale: the launch walks the BVH for
    the new light, as the frames do"""
    r = renderer()
    r.configure(128, 128, shadows=True, light=LIGHTS[0])
    check(po, r.aov(), "tekkaman", 128, 128, [LIGHTS[0]])
    r.set_light(LIGHTS[3])
    assert r.setup_stats()["slist_stale"] == 1
    check(po, r.aov(), "tekkaman", 128, 128, [LIGHTS[3]])
    r.set_list_policy(0)
    try:
        r.set_light(LIGHTS[4])  # its lists queued at once
        check(po, r.aov(), "tekkaman", 128, 128, [LIGHTS[4]])
    finally:
        r.set_list_policy(8)    # (the shared renderer keeps the default policy)


@pytest.mark.parametrize("lights", [LIGHTS[:1], LIGHTS[:3]], ids=["K1", "K3"])
def test_counters(po, lights):
    w = h = 128
    r = renderer()
    r.configure(w, h, shadows=True, light=lights[0], counters=True)
    if len(lights) > 1:
        r.set_lights(lights)
    rec = r.aov()
    st = r.stats()
    ks = [frame(po, "tekkaman", w, h, L)[3] for L in lights]
    assert st["primary_rays"] == ks[0]["primary_rays"] == w * h
    assert st["geometry_hits"] == ks[0]["geometry_hits"]
    assert st["shadow_rays"] == sum(k["shadow_rays"] for k in ks)
    assert st["occluded"] == sum(k["occluded"] for k in ks) == int(popcount(rec["light_mask"]).sum())
    assert st["kernel_ms"] > 0


# ---- ordering and state --------------------------------------------------------

def test_behind_two_frames_in_flight(po):
    w = h = 128
    A, B = LIGHTS[0], LIGHTS[1]
    r = renderer()
    r.configure(w, h, shadows=True, light=A, counters=False)
    r.start()
    r.set_light(B)
    r.start()
    assert r.aov(wait=False) is None
    r.wait()
    assert np.array_equal(r.framebuffer(), frame(po, "tekkaman", w, h, B)[0])
    assert np.array_equal(r.framebuffer_prev(), frame(po, "tekkaman", w, h, A)[0])
    check(po, r.aov_records(), "tekkaman", w, h, [B])
    assert r.kernel_ms() > 0
    # and a frame started behind the launch
    r.aov(wait=False)
    r.start()
    r.wait()
    assert np.array_equal(r.framebuffer(), frame(po, "tekkaman", w, h, B)[0])
    check(po, r.aov_records(), "tekkaman", w, h, [B])


def test_state(po):
    s = rt.Scene.load(scene_path("tekkaman"))
    r = rt.Renderer(s)
    with pytest.raises(rt.RtError):
        r.aov()                                                # before any configure
    r.configure(32, 32, shadows=True)
    with pytest.raises(rt.RtError):
        r.aov_records()                                        # configured, no launch yet
    check(po, r.aov(), "tekkaman", 32, 32, LIGHTS[:1])
    r.configure(200, 136, shadows=True)                        # another size: the buffer follows
    with pytest.raises(rt.RtError):
        r.aov_records()                                        # the configure released it
    check(po, r.aov(), "tekkaman", 200, 136, LIGHTS[:1])
    r.close()
    for _ in range(3):                                         # create / aov / close cycles
        r = rt.Renderer(s)
        r.configure(32, 32, shadows=True)
        check(po, r.aov(), "tekkaman", 32, 32, LIGHTS[:1])
        r.close()
    s.close()


# ---- refusals ------------------------------------------------------------------

def _refused(fn, *a):
    with pytest.raises(rt.RtError, match=r"\(-2\)"):
        fn(*a)


@pytest.mark.parametrize("kw", [dict(path=True), dict(flat=True), dict(raster=True), dict(instrumented=True),
                                dict(bvh_width=2)], ids=["path", "flat", "raster", "instrumented", "deep-tree"])
def test_refused_configurations(po, kw):
    r = renderer(key="/refusals")  # (a renderer of its own: one that ran the generic images keeps them)
    r.configure(128, 128, shadows=not kw.get("raster"), **kw)
    _refused(r.aov)
    _refused(r.aov, False)
    r.render()                                                 # the renderer still renders its frame
    if "instrumented" in kw or "bvh_width" in kw:
        assert np.array_equal(r.framebuffer(), frame(po, "tekkaman", 128, 128, LIGHTS[0])[0])


def test_refused_ordered_tail(po):
    sv = rt.Scene.load(scene_path("vase"), om_layers=True)
    assert sv.om_split()[1] > 0
    ro = rt.Renderer(sv)
    ro.configure(128, 128, shadows=True)
    _refused(ro.aov)
    ro.render()
    want = ro.framebuffer().copy()
    _refused(ro.aov)
    ro.render()
    assert np.array_equal(ro.framebuffer(), want)
    ro.close()
    sv.close()


# ---- the CLI ---------------------------------------------------------------------

def test_rtapp_writes_the_records(po, tmp_path):
    out = tmp_path / "out.aov"
    lights = LIGHTS[:3]
    arg = [f"{x:g},{y:g},{w:g}" for x, y, w in lights]
    p = subprocess.run([os.path.join(_lib.LIB_DIR, "rtapp"), "-t", scene_path("tekkaman"), "-w128", "-h128", "-S",
                        "-L", arg[0], "-M", arg[1], "-M", arg[2], "-o", "null", "-V", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = out.read_bytes()
    head = np.frombuffer(raw[:16], np.uint32)
    assert raw[:4] == b"RTAV" and list(head[1:]) == [128, 128, 16]
    got = np.frombuffer(raw[16:], rt.AOV_DTYPE).reshape(128, 128)
    r = renderer()
    r.configure(128, 128, shadows=True, light=lights[0], counters=True)
    r.set_lights(lights)
    rec = r.aov()
    st = r.stats()
    assert np.array_equal(got.view(np.uint32), rec.view(np.uint32))
    check(po, got, "tekkaman", 128, 128, lights)
    line = f"AOV: {st['geometry_hits']} geometry, {st['shadow_rays']} shadow rays, {st['occluded']} occluded"
    assert line in p.stdout, p.stdout
    # one light, the host setup (-H), partial tiles
    p = subprocess.run([os.path.join(_lib.LIB_DIR, "rtapp"), "-t", scene_path("tekkaman"), "-w200", "-h136", "-S", "-H",
                        "-L", arg[1], "-o", "null", "-V", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = out.read_bytes()
    assert raw[:4] == b"RTAV" and list(np.frombuffer(raw[4:16], np.uint32)) == [200, 136, 16]
    check(po, np.frombuffer(raw[16:], rt.AOV_DTYPE).reshape(136, 200), "tekkaman", 200, 136, [lights[1]])


if __name__ == "__main__":
    _child(sys.argv[1])
