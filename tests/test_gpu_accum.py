"""GPU tests of progressive path tracing (vx_rt.h rt_renderer_accum_begin; image
pt_accum, pt_kernel.hip PT_ACCUM) against the untouched oracle, bit for bit.

The model is built here from what the oracle already produces: sample i of a
renderer configured with seed s0 is the oracle's 8-bit path frame of seed
(s0 + i) mod 2^32; a pixel's record is {sum R, sum G, sum B, n} over its
samples; the frame is alpha | mean(R) << 16 | mean(G) << 8 | mean(B) with
mean(c) = (2 * sum_c + n) // (2 * n) and sample 0's alpha.  Records and frames
must equal it exactly however the samples are split over launches, after
resets and light changes, with counters, shards, the BVH walk and plain frames
in between.  No reference exists for this row; the oracle's frames
themselves are held to the model of tests/rt_reference.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, rt  # noqa: E402

S0 = 0x5EED
OTHER_LIGHT = (20.0, 50.0, 85.0)
_scenes = {}
_samples = {}


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def setup(po, name):
    if name not in _scenes:
        s = rt.Scene.load(scene_path(name))
        _scenes[name] = (s, rt.Renderer(s), po.OracleScene(po.cgltrace.load(scene_path(name))),
                         s.bvh() + (s.bvh4(),))
    return _scenes[name]


def sample(po, name, size, bounces, seed, light=rt.DEFAULT_LIGHT):
    """(frame, counters) of the oracle's one-sample path frame; computed once."""
    key = (name, size, bounces, seed & 0xFFFFFFFF, tuple(light))
    if key not in _samples:
        _, _, osc, bvh = setup(po, name)
        c, _, _, k = po.rt_render(osc, po.rt_params(size, size, path=True, bounces=bounces,
                                                    seed=seed & 0xFFFFFFFF, light=light, nthreads=8), bvh=bvh)
        c.setflags(write=False)
        _samples[key] = (c, k)
    return _samples[key]


def model(po, name, size, bounces, s0, n, light=rt.DEFAULT_LIGHT):
    """(records uint32[H, W, 4], frame uint32[H, W]) of samples s0 .. s0 + n - 1."""
    frames = [sample(po, name, size, bounces, s0 + i, light)[0] for i in range(n)]
    rec = np.zeros(frames[0].shape + (4,), np.uint64)
    for c in frames:
        rec[..., 0] += (c >> 16) & 0xFF
        rec[..., 1] += (c >> 8) & 0xFF
        rec[..., 2] += c & 0xFF
    rec[..., 3] = n
    m = (2 * rec[..., :3] + n) // (2 * n)
    frame = (frames[0] & np.uint32(0xFF000000)) | (m[..., 0] << 16 | m[..., 1] << 8 | m[..., 2]).astype(np.uint32)
    return rec.astype(np.uint32), frame


def check(r, rec, frame, what=""):
    got = r.accum()
    assert np.array_equal(got, rec), f"{what}: {int((got != rec).any(axis=-1).sum())} records differ"
    fb = r.framebuffer()
    assert np.array_equal(fb, frame), f"{what}: {int((fb != frame).sum())} pixels differ"


def test_one_sample_is_the_plain_path_frame(po):
    _, r, _, _ = setup(po, "tekkaman")
    r.configure(128, 128, path=True, bounces=4, seed=S0)
    r.render()
    plain = r.framebuffer()
    r.accum_begin()
    r.accumulate(1)
    c = sample(po, "tekkaman", 128, 4, S0)[0]
    fb = r.framebuffer()
    assert np.array_equal(fb, c) and np.array_equal(fb, plain)
    rec = r.accum()
    want = np.stack([(c >> 16) & 0xFF, (c >> 8) & 0xFF, c & 0xFF, np.ones_like(c)], -1)
    assert np.array_equal(rec, want)
    assert r.accum_samples() == 1


@pytest.mark.parametrize("name,size,bounces,walk", [("tekkaman", 128, 4, False), ("tekkaman", 256, 4, False),
                                                     ("triangle", 64, 4, False), ("tekkaman", 333, 2, False),
                                                     ("tekkaman", 256, 4, True)])
def test_k_samples_in_one_launch(po, name, size, bounces, walk):
    """walk: RT_RENDER_BVH_WALK -- no shadow lists, the paired-vertex loop."""
    _, r, _, _ = setup(po, name)
    r.configure(size, size, path=True, bounces=bounces, seed=S0, bvh_walk=walk)
    r.accum_begin()
    r.accumulate(4)
    check(r, *model(po, name, size, bounces, S0, 4), what=f"{name} {size} walk={walk}")


def test_host_setup_accumulates(po):
    """RT_RENDER_HOST_SETUP: no shadow lists either (full waves take the per-lane loop
    with the BVH walk, the split waves the paired vertices)."""
    _, r, _, _ = setup(po, "tekkaman")
    r.configure(128, 128, path=True, bounces=4, seed=S0, host_setup=True)
    r.accum_begin()
    r.accumulate(3)
    r.accumulate(1)
    check(r, *model(po, "tekkaman", 128, 4, S0, 4), what="host setup")


@pytest.mark.parametrize("wait", [True, False])
def test_launch_split_is_immaterial(po, wait):
    _, r, _, _ = setup(po, "tekkaman")
    rec, frame = model(po, "tekkaman", 128, 4, S0, 6)
    r.configure(128, 128, path=True, bounces=4, seed=S0)
    r.accum_begin()
    r.accumulate(6)
    check(r, rec, frame, "one launch of 6")
    r.accum_reset()
    assert r.accum_samples() == 0
    for k in (3, 1, 2):
        r.accumulate(k, wait=wait)
    r.wait()
    assert r.accum_samples() == 6
    check(r, rec, frame, f"launches of 3, 1, 2 (wait={wait})")


def test_reset(po):
    _, r, _, _ = setup(po, "tekkaman")
    rec2, frame2 = model(po, "tekkaman", 128, 4, S0, 2)
    r.configure(128, 128, path=True, bounces=4, seed=S0)
    r.accum_begin()
    r.accumulate(5)
    assert r.accum_samples() == 5
    r.accum_reset()
    r.accumulate(2)
    assert r.accum_samples() == 2
    check(r, rec2, frame2, "after reset")
    # a fresh buffer where another resolution's records lay: the first launch reads none
    r.configure(256, 256, path=True, bounces=4, seed=S0)
    r.accum_begin()
    r.accumulate(4)
    r.configure(128, 128, path=True, bounces=4, seed=S0)
    r.accum_begin()
    r.accumulate(2)
    check(r, rec2, frame2, "after another resolution")


def test_moved_light_resets(po):
    _, r, _, _ = setup(po, "tekkaman")
    r.configure(128, 128, path=True, bounces=4, seed=S0)
    r.set_list_policy(0)
    try:
        r.accum_begin()
        r.accumulate(3)
        r.set_light(OTHER_LIGHT)
        assert r.accum_samples() == 0
        r.accumulate(2)
        assert r.accum_samples() == 2
        check(r, *model(po, "tekkaman", 128, 4, S0, 2, light=OTHER_LIGHT), what="moved light")
    finally:
        r.set_list_policy(8)


def test_seed_wraps(po):
    _, r, _, _ = setup(po, "tekkaman")
    s0 = 0xFFFFFFFE
    r.configure(128, 128, path=True, bounces=4, seed=s0)
    r.accum_begin()
    r.accumulate(4)
    check(r, *model(po, "tekkaman", 128, 4, s0, 4), what="seed wrap")


def test_counters(po):
    _, r, _, _ = setup(po, "tekkaman")
    r.configure(128, 128, path=True, bounces=4, seed=S0, counters=True)
    r.accum_begin()
    r.accumulate(3)
    st = r.stats()
    ks = [sample(po, "tekkaman", 128, 4, S0 + i)[1] for i in range(3)]
    assert st["primary_rays"] == 128 * 128
    assert st["geometry_hits"] == ks[0]["geometry_hits"]
    for key in ("shadow_rays", "occluded", "bounce_rays"):
        assert st[key] == sum(k[key] for k in ks), key
    check(r, *model(po, "tekkaman", 128, 4, S0, 3), what="counters")


def test_shards(po):
    _, r, _, _ = setup(po, "tekkaman")
    rec, frame = model(po, "tekkaman", 128, 4, S0, 2)
    fbs, recs = [], []
    for i in range(2):
        r.configure(128, 128, path=True, bounces=4, seed=S0, shard_index=i, shard_count=2)
        r.accum_begin()
        r.accumulate(2)
        fbs.append(r.framebuffer().copy())
        recs.append(r.accum().copy())
    assert np.array_equal(rt.deinterleave_tiles(fbs, 128, 128), frame)
    for ch in range(4):
        got = rt.deinterleave_tiles([np.ascontiguousarray(a[:, ch]) for a in recs], 128, 128)
        assert np.array_equal(got, rec[..., ch]), ch
    # one compact shard: the same layout
    r.configure(128, 128, path=True, bounces=4, seed=S0, compact=True)
    r.accum_begin()
    r.accumulate(2)
    assert np.array_equal(rt.deinterleave_tiles([r.framebuffer()], 128, 128), frame)


def test_plain_frames_unaffected(po):
    _, r, _, _ = setup(po, "tekkaman")
    rec2, _ = model(po, "tekkaman", 128, 4, S0, 2)
    rec3, frame3 = model(po, "tekkaman", 128, 4, S0, 3)
    c0 = sample(po, "tekkaman", 128, 4, S0)[0]
    # (counters off: the configuration keeps two framebuffers and overlaps its started frames)
    r.configure(128, 128, path=True, bounces=4, seed=S0, counters=False)
    r.accum_begin()
    r.accumulate(2)
    r.render()
    assert np.array_equal(r.framebuffer(), c0)
    assert np.array_equal(r.accum(), rec2)
    r.start()
    r.start()
    r.accumulate(1)
    assert r.accum_samples() == 3
    check(r, rec3, frame3, "behind an overlapped pair")
    r.start()
    r.wait()
    assert np.array_equal(r.framebuffer(), c0)
    assert np.array_equal(r.accum(), rec3)


def _refused(fn, *a):
    with pytest.raises(rt.RtError, match=r"\(-2\)"):
        fn(*a)


def test_refusals(po):
    s, _, _, _ = setup(po, "tekkaman")
    r = rt.Renderer(s)                                        # (its own: RT_RENDER_BVH2 keeps the generic images)
    r.configure(128, 128, path=True)
    _refused(r.accumulate, 1)                                 # before accum_begin
    _refused(r.accum_reset)
    r.accum_begin()
    _refused(r.accumulate, 0)                                 # samples outside 1..32
    _refused(r.accumulate, 33)
    r.accumulate(1)
    r.configure(128, 128, path=True)                          # a configure ends accumulation
    _refused(r.accumulate, 1)
    r.configure(128, 128, shadows=True)
    _refused(r.accum_begin)                                   # not a path frame
    r.configure(128, 128, path=True, instrumented=True)
    _refused(r.accum_begin)                                   # no instrumented image
    r.configure(128, 128, path=True, bvh_width=2)
    _refused(r.accum_begin)                                   # a layout the generic images run
    r.close()
    os.environ["RT_PT_QUEUE"] = "1"
    try:
        rq = rt.Renderer(s)
        rq.configure(128, 128, path=True)
        assert rq.setup_stats()["path_queue"] == 1
        _refused(rq.accum_begin)                              # the two-kernel queue form
        rq.close()
    finally:
        del os.environ["RT_PT_QUEUE"]
    rc = rt.Renderer(s, kernel_dir=os.path.join(_lib.LIB_DIR, "pt_compact"))
    rc.configure(128, 128, path=True)
    _refused(rc.accum_begin)                                  # a directory without pt_accum.vxbin
    rc.close()


def test_sample_cap(po):
    """2^24 samples per pixel are taken -- the u32 sums hold 2^24 * 255 -- and
    the next launch is refused.  The smallest frame there is: triangle at 32^2
    (one tile, no geometry: every pixel adds k x its colour), in launches of
    32, the queue drained now and then."""
    s = rt.Scene.load(scene_path("triangle"))
    r = rt.Renderer(s)
    # (a white background: its sums end at the very top, 2^24 * 255)
    r.configure(32, 32, path=True, bounces=0, seed=S0, counters=False, clear_color=0xFFFFFFFF)
    r.render()
    one = r.framebuffer()                                     # no bounce: every sample is this frame
    r.set_timing(False)
    r.accum_begin()
    cap = 1 << 24
    for i in range(cap // 32):
        r.accumulate(32, wait=False)
        if i % 8192 == 8191:
            r.wait()
    r.wait()
    r.set_timing(True)
    assert r.accum_samples() == cap
    _refused(r.accumulate, 1)                                 # the 2^24 cap
    want = np.stack([((one >> 16) & 0xFF) * cap, ((one >> 8) & 0xFF) * cap, (one & 0xFF) * cap,
                     np.full_like(one, cap)], -1).astype(np.uint32)
    assert (one & 0xFF).max() == 255                          # (a channel at the sums' upper end)
    assert np.array_equal(r.accum(), want)
    assert np.array_equal(r.framebuffer(), one)
    r.close()
    s.close()


def test_rtapp_accumulates(po, tmp_path):
    out = tmp_path / "accum.png"
    p = subprocess.run([os.path.join(_lib.LIB_DIR, "rtapp"), "-t", scene_path("tekkaman"), "-w", "128", "-h", "128",
                        "-P4", "-A5", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Accumulated 5 samples" in p.stdout
    _, frame = model(po, "tekkaman", 128, 4, S0, 5)
    got = po.load_png_argb(str(out))[::-1]                    # the PNG is top-down
    assert np.array_equal(got, frame), f"{int((got != frame).sum())} pixels differ"
