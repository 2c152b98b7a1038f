"""Renderer and device lifecycle in one process: the
round-5 work-in-progress runs r05c / r05d died with SIGSEGV inside
rt_renderer_create while the driver's pinned completion block was being
introduced.  Several renderers created and closed in turn, two alive at once
on one device, each rendering synchronous frames (start + wait: the
completion kernel and its pinned word) and back-to-back frames: every frame
equals the first renderer's, nothing faults."""
import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402


def _frames(r, n_sync=4, n_queued=6):
    for _ in range(n_sync):
        r.render()                      # synchronous: completion kernel + pinned word
    a = r.framebuffer().copy()
    r.set_timing(False)
    try:
        for _ in range(n_queued):       # back to back, no per-launch timing
            r.start()
        r.wait()
    finally:
        r.set_timing(True)
    b = r.framebuffer()
    assert np.array_equal(a, b)
    return a


def test_renderers_created_and_closed_in_turn():
    s = rt.Scene.load(scene_path("tekkaman"))
    ref = None
    for i in range(6):
        r = rt.Renderer(s)
        r.configure(256, 256, shadows=True, counters=False, bvh_walk=(i % 2 == 1))
        fb = _frames(r)
        ref = fb if ref is None else ref
        assert np.array_equal(fb, ref), i
        assert r.kernel_ms() > 0.0
        r.close()
    s.close()


def test_two_renderers_alive_at_once():
    s = rt.Scene.load(scene_path("tekkaman"))
    r1, r2 = rt.Renderer(s), rt.Renderer(s)
    r1.configure(256, 256, shadows=True, counters=False)
    r2.configure(256, 256, shadows=True, path=True, bounces=2, counters=False)
    a1, a2 = _frames(r1), _frames(r2)
    for _ in range(3):                  # interleaved synchronous frames
        r1.render()
        r2.render()
        assert np.array_equal(r1.framebuffer(), a1) and np.array_equal(r2.framebuffer(), a2)
    r2.close()
    assert np.array_equal(_frames(r1), a1)
    r1.close()
    s.close()


# ---- one renderer through every kernel image ---------------------------------------------------
# (the images rt_lights*, pt_accum and pt_lights* are loaded by the first call that runs them and
# stay loaded next to the modes' own: the image a frame runs is chosen anew for every frame)

_L2 = [(0.0, 60.0, 80.0), (20.0, 50.0, 85.0)]
_PATH = dict(path=True, bounces=4, seed=0x5EED)


def _frame(r):
    r.render()
    return [r.framebuffer().copy()]


def _accumulated(r):
    r.accumulate(2)
    return [r.accum().copy(), r.framebuffer().copy()]


# (step, what the walked renderer does on top of the step before, what a fresh renderer does to
# stand in the same state, what is then run and read on both)
_STEPS = [
    ("shadows", lambda r: r.configure(128, 128, shadows=True), None, _frame),
    ("set_lights, 2 lights", lambda r: r.set_lights(_L2),
     lambda r: (r.configure(128, 128, shadows=True), r.set_lights(_L2)), _frame),
    ("path", lambda r: r.configure(128, 128, **_PATH), None, _frame),
    ("accumulate 2 samples", lambda r: r.accum_begin(),
     lambda r: (r.configure(128, 128, **_PATH), r.accum_begin()), _accumulated),
    ("set_path_lights, 2 lights: a frame", lambda r: r.set_path_lights(_L2),
     lambda r: (r.configure(128, 128, **_PATH), r.set_path_lights(_L2)), _frame),
    ("set_path_lights, 2 lights: accumulate 2 samples", lambda r: None,
     lambda r: (r.configure(128, 128, **_PATH), r.set_path_lights(_L2), r.accum_begin()), _accumulated),
    ("bvh_walk", lambda r: r.configure(128, 128, shadows=True, bvh_walk=True), None, _frame),
    ("flat", lambda r: r.configure(128, 128, shadows=True, flat=True), None, _frame),
    ("raster", lambda r: r.configure(128, 128, raster=True), None, _frame),
    ("instrumented shadows", lambda r: r.configure(128, 128, shadows=True, instrumented=True), None, _frame),
]


def test_one_renderer_through_every_image():
    s = rt.Scene.load(scene_path("tekkaman"))
    walked = rt.Renderer(s)
    for what, step, fresh_setup, run in _STEPS:
        step(walked)
        got = run(walked)
        fresh = rt.Renderer(s)
        (fresh_setup or step)(fresh)
        want = run(fresh)
        fresh.close()
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {int((g != w).sum())} values differ"
        # not a cleared buffer on both sides
        assert len(np.unique(got[-1])) > 16, what
    walked.close()
    s.close()
