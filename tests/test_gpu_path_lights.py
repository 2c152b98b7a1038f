"""GPU tests of path-traced frames lit by several point lights in one launch
(vx_rt.h rt_renderer_set_path_lights; images pt_lights / pt_lights_accum,
pt_kernel.hip PT_LIGHTS) against the untouched oracle, bit for bit.

The model is built here from frames the oracle already produces: a K-light
path frame of seed s is, per pixel and colour channel, the rounded mean
(2 * sum + K) // (2 * K) of the K single-light path frames of seed s, under the
primary colour's alpha (the same in every one of them).  Sample j of an
accumulation under K lights is that frame for seed (s0 + j) mod 2^32; a record
is {sum R, sum G, sum B, n} over the samples' 8-bit values and the accumulated
frame their rounded mean.  primary_rays, geometry_hits and bounce_rays are one
single-light frame's, shadow_rays and occluded the sums over the lights (and,
with bounce_rays, over a launch's samples).  No reference exists for this row;
the oracle's frames themselves are held to the model of tests/rt_reference.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from test_gpu_light import LIGHTS

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, rt  # noqa: E402

S0 = 0x5EED
# three more lights for the 8-light case: the measurement script's grid (scripts/bench_path_lights.py)
GRID = [(-10.0 + 20.0 * i / 3.0, 50.0 + 20.0 * j / 3.0, 80.0) for j in range(4) for i in range(4)]
EIGHT = list(LIGHTS) + [GRID[0], GRID[5], GRID[15]]
K3 = LIGHTS[:3]
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


def single(po, w, h, bounces, seed, light, path=True):
    """(frame, counters) of the oracle's single-light frame; computed once, left unchanged."""
    key = (w, h, bounces, seed & 0xFFFFFFFF, tuple(light), path)
    if key not in _frames:
        _, _, osc, bvh = setup(po)
        kw = dict(path=True, bounces=bounces, seed=seed & 0xFFFFFFFF) if path else dict(shadows=True)
        c, _, _, k = po.rt_render(osc, po.rt_params(w, h, light=light, nthreads=8, **kw), bvh=bvh)
        c = c.reshape(h, w)
        c.setflags(write=False)
        _frames[key] = (c, k)
    return _frames[key]


def channels(c):
    return np.stack([(c >> np.uint32(16)) & np.uint32(0xFF), (c >> np.uint32(8)) & np.uint32(0xFF),
                     c & np.uint32(0xFF)], -1).astype(np.uint64)


def pack(alpha_of, m):
    return (alpha_of & np.uint32(0xFF000000)) | (m[..., 0] << 16 | m[..., 1] << 8 | m[..., 2]).astype(np.uint32)


def mean_frame(po, w, h, bounces, seed, lights, min_mixed=None, min_rounded=0):
    """The numpy mean of the single-light path frames of one seed.  At least min_mixed of its
    pixels have single-light frames that differ, at least min_rounded channel values a rounded
    mean other than the truncated one: the per-light accumulators and the resolve are exercised."""
    fr = [single(po, w, h, bounces, seed, L)[0] for L in lights]
    n = len(fr)
    tot = sum(channels(c) for c in fr)
    out = pack(fr[0], (2 * tot + n) // (2 * n))
    if min_mixed is None:
        min_mixed = 100 if n > 1 else 0
    mixed = int(np.any([c != fr[0] for c in fr[1:]], axis=0).sum()) if n > 1 else 0
    rounded = int(((2 * tot + n) // (2 * n) != tot // n).sum())
    print(f"{w}x{h} K={n} seed {seed & 0xFFFFFFFF:#x}: {mixed} pixels whose single-light frames differ, "
          f"{rounded} channel values rounded up")
    assert mixed >= min_mixed, f"only {mixed} pixels whose single-light frames differ"
    assert rounded >= min_rounded, f"only {rounded} channel values where rounding matters"
    for c in fr:
        assert np.array_equal(c >> np.uint32(24), fr[0] >> np.uint32(24))
    return out


def model(po, w, h, bounces, s0, n, lights):
    """(records uint32[H, W, 4], frame uint32[H, W]) of samples s0 .. s0 + n - 1 under `lights`."""
    frames = [mean_frame(po, w, h, bounces, s0 + j, lights) for j in range(n)]
    rec = np.zeros(frames[0].shape + (4,), np.uint64)
    for c in frames:
        rec[..., :3] += channels(c)
    rec[..., 3] = n
    return rec.astype(np.uint32), pack(frames[0], (2 * rec[..., :3] + n) // (2 * n))


def check(r, rec, frame, what=""):
    got = r.accum()
    assert np.array_equal(got, rec), f"{what}: {int((got != rec).any(axis=-1).sum())} records differ"
    fb = r.framebuffer()
    assert np.array_equal(fb, frame), f"{what}: {int((fb != frame).sum())} pixels differ"


def same(fb, want, what=""):
    assert np.array_equal(fb, want), f"{what}: {int((fb != want).sum())} pixels differ"


@pytest.mark.parametrize("w,h,bounces,lights,rounded",
                         [(128, 128, 4, LIGHTS[:1], 0), (128, 128, 4, LIGHTS[:2], 100), (128, 128, 4, K3, 100),
                          (128, 128, 4, LIGHTS, 0), (128, 128, 4, EIGHT, 0), (200, 136, 4, K3, 0),
                          (333, 333, 2, LIGHTS[:2], 0)],
                         ids=["128-K1", "128-K2", "128-K3", "128-K5", "128-K8", "200x136-K3", "333-b2-K2"])
def test_frames_equal_mean_of_oracle_frames(po, w, h, bounces, lights, rounded):
    _, r, _, _ = setup(po)
    r.configure(w, h, path=True, bounces=bounces, seed=S0, light=lights[0])
    if len(lights) == 1:
        r.render()
        plain = r.framebuffer()
    r.set_path_lights(lights)
    r.render()
    fb = r.framebuffer()
    same(fb, mean_frame(po, w, h, bounces, S0, lights, min_rounded=rounded), f"{w}x{h} K={len(lights)}")
    if len(lights) == 1:
        assert np.array_equal(fb, plain)
    info = r.lights_info()
    assert len(info) == len(lights)
    for i, L in zip(info, lights):
        assert np.array_equal(np.float32(i["light"]), np.float32(L))
        assert i["slist_on"] == 1 and i["slist_entries"] > 0


def test_mixed_pixels_grow_with_the_lights(po):
    """The pixels whose single-light frames differ: a count monotone in K (128^2, 4 bounces)."""
    counts = []
    for lights in (LIGHTS[:2], K3, LIGHTS, EIGHT):
        fr = [single(po, 128, 128, 4, S0, L)[0] for L in lights]
        counts.append(int(np.any([c != fr[0] for c in fr[1:]], axis=0).sum()))
    assert counts == sorted(counts) and counts[0] >= 100, counts


def test_accumulate(po):
    _, r, _, _ = setup(po)
    r.configure(128, 128, path=True, bounces=4, seed=S0, light=K3[0])
    r.set_path_lights(K3)
    r.accum_begin()
    r.accumulate(4)
    assert r.accum_samples() == 4
    check(r, *model(po, 128, 128, 4, S0, 4, K3), what="accumulate(4), K=3")


@pytest.mark.parametrize("wait", [True, False])
def test_launch_split_is_immaterial(po, wait):
    _, r, _, _ = setup(po)
    rec, frame = model(po, 128, 128, 4, S0, 6, K3)
    r.configure(128, 128, path=True, bounces=4, seed=S0, light=K3[0])
    r.accum_begin()                                           # (accumulation begun ahead of the lights)
    r.set_path_lights(K3)
    r.accumulate(6)
    check(r, rec, frame, "one launch of 6")
    r.accum_reset()
    assert r.accum_samples() == 0
    for k in (3, 1, 2):
        r.accumulate(k, wait=wait)
    r.wait()
    assert r.accum_samples() == 6
    check(r, rec, frame, f"launches of 3, 1, 2 (wait={wait})")


def test_light_changes_reset(po):
    _, r, _, _ = setup(po)
    other = LIGHTS[1:4]
    r.configure(128, 128, path=True, bounces=4, seed=S0, light=K3[0])
    r.set_list_policy(0)
    try:
        r.set_path_lights(K3)
        r.accum_begin()
        r.accumulate(3)
        r.set_path_lights(other)                              # in mid-accumulation: the records start over
        assert r.accum_samples() == 0
        r.accumulate(2)
        assert r.accum_samples() == 2
        check(r, *model(po, 128, 128, 4, S0, 2, other), what="new lights")
        r.set_light(LIGHTS[1])                                # back to one light, and over again
        assert r.accum_samples() == 0 and len(r.lights_info()) == 1
        r.accumulate(2)
        check(r, *model(po, 128, 128, 4, S0, 2, LIGHTS[1:2]), what="one light again")
        r.render()
        same(r.framebuffer(), single(po, 128, 128, 4, S0, LIGHTS[1])[0], "plain frame, one light again")
    finally:
        r.set_list_policy(8)


def test_seed_wraps(po):
    _, r, _, _ = setup(po)
    s0 = 0xFFFFFFFE
    r.configure(128, 128, path=True, bounces=4, seed=s0, light=K3[0])
    r.set_path_lights(K3)
    r.accum_begin()
    r.accumulate(3)                                           # seeds 0xFFFFFFFE, 0xFFFFFFFF, 0
    check(r, *model(po, 128, 128, 4, s0, 3, K3), what="seed wrap")


def test_counters(po):
    _, r, _, _ = setup(po)
    r.configure(128, 128, path=True, bounces=4, seed=S0, light=K3[0], counters=True)
    r.set_path_lights(K3)
    r.render()
    st = r.stats()
    ks = [[single(po, 128, 128, 4, S0 + j, L)[1] for L in K3] for j in range(2)]
    for j in range(2):
        for key in ("geometry_hits", "bounce_rays"):
            assert all(k[key] == ks[j][0][key] for k in ks[j]), key   # (the oracle: not the light's)
    assert st["primary_rays"] == 128 * 128
    assert st["geometry_hits"] == ks[0][0]["geometry_hits"]
    assert st["bounce_rays"] == ks[0][0]["bounce_rays"]
    for key in ("shadow_rays", "occluded"):
        assert st[key] == sum(k[key] for k in ks[0]), key
    same(r.framebuffer(), mean_frame(po, 128, 128, 4, S0, K3), "counters")
    r.accum_begin()
    r.accumulate(2)
    st = r.stats()
    assert st["primary_rays"] == 128 * 128
    assert st["geometry_hits"] == ks[0][0]["geometry_hits"]
    assert st["bounce_rays"] == sum(kj[0]["bounce_rays"] for kj in ks)
    for key in ("shadow_rays", "occluded"):
        assert st[key] == sum(k[key] for kj in ks for k in kj), key
    check(r, *model(po, 128, 128, 4, S0, 2, K3), what="counters, accumulate(2)")


def test_shards_and_compact(po):
    _, r, _, _ = setup(po)
    want = mean_frame(po, 128, 128, 4, S0, K3)
    rec, frame = model(po, 128, 128, 4, S0, 2, K3)
    fbs, afbs, recs = [], [], []
    for i in range(2):
        r.configure(128, 128, path=True, bounces=4, seed=S0, light=K3[0], shard_index=i, shard_count=2)
        r.set_path_lights(K3)
        r.render()
        fbs.append(r.framebuffer().copy())
        r.accum_begin()
        r.accumulate(2)
        afbs.append(r.framebuffer().copy())
        recs.append(r.accum().copy())
    same(rt.deinterleave_tiles(fbs, 128, 128), want, "2 shards")
    same(rt.deinterleave_tiles(afbs, 128, 128), frame, "2 shards, accumulate(2)")
    for ch in range(4):
        got = rt.deinterleave_tiles([np.ascontiguousarray(a[:, ch]) for a in recs], 128, 128)
        assert np.array_equal(got, rec[..., ch]), ch
    r.configure(128, 128, path=True, bounces=4, seed=S0, light=K3[0], compact=True)
    r.set_path_lights(K3)
    r.render()
    same(rt.deinterleave_tiles([r.framebuffer()], 128, 128), want, "compact")


def test_plain_and_overlapped_frames_around_the_call(po):
    _, r, _, _ = setup(po)
    one = single(po, 128, 128, 4, S0, K3[0])[0]
    want = mean_frame(po, 128, 128, 4, S0, K3)
    # (counters off: the configuration keeps two framebuffers and overlaps its started frames)
    r.configure(128, 128, path=True, bounces=4, seed=S0, light=K3[0], counters=False)
    r.render()
    same(r.framebuffer(), one, "plain frame ahead")
    r.start()
    r.start()
    r.set_path_lights(K3)                                     # behind an overlapped pair
    r.start()
    r.wait()
    same(r.framebuffer(), want, "behind an overlapped pair")
    r.start()
    r.start()
    r.wait()
    same(r.framebuffer(), want, "started twice")
    r.configure(128, 128, path=True, bounces=4, seed=S0, light=K3[0], counters=False)
    assert len(r.lights_info()) == 1
    r.render()
    same(r.framebuffer(), one, "after a configure")


def _refused(fn, *a):
    with pytest.raises(rt.RtError, match=r"\(-2\)"):
        fn(*a)


def _refused_then_single(po, r, lights, what, path=True):
    """-2, and the renderer is lit by its single light: the next frame is the oracle's."""
    _refused(r.set_path_lights, lights)
    assert len(r.lights_info()) == 1, what
    r.render()
    same(r.framebuffer(), single(po, 128, 128, 4, S0, LIGHTS[0], path=path)[0], what)


def test_refusals(po, monkeypatch):
    s, _, _, _ = setup(po)
    r = rt.Renderer(s)                                        # (its own: bvh_width=2 keeps the generic images)
    cfg = dict(path=True, bounces=4, seed=S0, light=LIGHTS[0])
    r.configure(128, 128, **cfg)
    _refused_then_single(po, r, [], "0 lights")
    _refused_then_single(po, r, EIGHT + [GRID[3]], "9 lights")
    r.set_path_lights(K3)                                     # a refusal after a call that was accepted
    _refused_then_single(po, r, EIGHT + [GRID[3]], "9 lights after 3")
    _refused(r.set_lights, LIGHTS[:2])                        # the shadow frame's call still takes no path frame
    r.configure(128, 128, shadows=True, light=LIGHTS[0])
    _refused_then_single(po, r, K3, "not a path frame", path=False)
    r.configure(128, 128, instrumented=True, **cfg)
    _refused_then_single(po, r, K3, "instrumented")
    r.configure(128, 128, bvh_walk=True, **cfg)
    _refused_then_single(po, r, K3, "bvh_walk")
    r.configure(128, 128, host_setup=True, **cfg)
    _refused_then_single(po, r, K3, "host_setup")
    r.configure(128, 128, bvh_width=2, **cfg)
    _refused_then_single(po, r, K3, "a layout the generic images run")
    r.close()
    with monkeypatch.context() as m:
        m.setenv("RT_SHADOW_LISTS", "0")
        rl = rt.Renderer(s)
        rl.configure(128, 128, **cfg)
        _refused_then_single(po, rl, K3, "RT_SHADOW_LISTS=0")
        rl.close()
    with monkeypatch.context() as m:
        m.setenv("RT_PT_QUEUE", "1")
        rq = rt.Renderer(s)
        rq.configure(128, 128, **cfg)
        assert rq.setup_stats()["path_queue"] == 1
        _refused_then_single(po, rq, K3, "the two-kernel queue")
        rq.close()
    rc = rt.Renderer(s, kernel_dir=os.path.join(_lib.LIB_DIR, "pt_compact"))
    rc.configure(128, 128, **cfg)
    _refused_then_single(po, rc, K3, "a directory without pt_lights.vxbin")
    rc.close()
    with monkeypatch.context() as m:
        # LIGHTS[3]'s lists (244 783 entries) exceed the limit, the other two lights' fit
        m.setenv("RT_BLIST_MAX_ENTRIES", "100000")
        ro = rt.Renderer(s)
        ro.configure(128, 128, **cfg)
        _refused_then_single(po, ro, [LIGHTS[0], LIGHTS[3], LIGHTS[4]], "a light whose lists do not fit")
        ro.close()


@pytest.mark.parametrize("accum", [0, 3])
def test_rtapp_path_lights(po, tmp_path, accum):
    out = tmp_path / "path_lights.png"
    arg = [f"{x:g},{y:g},{w:g}" for x, y, w in K3]
    p = subprocess.run([os.path.join(_lib.LIB_DIR, "rtapp"), "-t", scene_path("tekkaman"), "-w", "128", "-h", "128",
                        "-P4", "-L", arg[0], "-M", arg[1], "-M", arg[2]] + ([f"-A{accum}"] if accum else []) +
                       ["-o", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Lights: 3" in p.stdout
    want = model(po, 128, 128, 4, S0, accum, K3)[1] if accum else mean_frame(po, 128, 128, 4, S0, K3)
    same(po.load_png_argb(str(out))[::-1], want, f"rtapp -A{accum}")   # the PNG is top-down
