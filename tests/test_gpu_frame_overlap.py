"""Consecutive frames overlapped on the driver's two launch lanes, double
buffered (vx_rt.h rt_render_start, vortex_hip.h vx_hip_set_launch_lane):
frame n renders into framebuffer n mod 2 on lane n mod 2, so frame n + 1 may
be resident while frame n drains.  What must hold, at 256x256 and at 200x136
(overhanging edge tiles) on tekkaman, exact to the byte:

* 64 frames started back to back with the light alternating A, B: the last
  frame is its light's reference frame and the frame before it the other
  light's -- no late store of one frame lands in the other's pixels; repeated
  with the sequence shifted by one, so each light lands on each buffer;
* the same with set_list_policy(0): the light-space lists are rebuilt before
  every frame, so setup launches sit between the frames; the frames are
  exact and the lists left behind are the last light's; and rebuilt before
  every fourth frame, so the setup launches sit between overlapped frames;
* after framebuffer_device() the renderer keeps to the pointer's buffer and
  lane 0; compact and instrumented configurations never overlap, and their
  counters are those of a frame rendered alone;
* VX_HIP_OVERLAP=0 (a child process: one lane, one framebuffer) gives the
  same bytes;
* VX_HIP_QUEUE_DEPTH=1: 32 synchronous frames, each exact, counted as 32 runs.

The reference frames come from a fresh configure + render per light, checked
against the oracle at 200x136.  No test asserts a time."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, scene_path

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402

A, B = (0.0, 60.0, 80.0), (20.0, 50.0, 85.0)
SIZES = [(256, 256), (200, 136)]
FRAMES = 64
_refs = {}


def _renderer():
    s = rt.Scene.load(scene_path("tekkaman"))
    return s, rt.Renderer(s)


def _ref(w, h, light):
    """The light's frame from a fresh configure + one synchronous render
    (computed once per size and light, never modified)."""
    key = (w, h, light)
    if key not in _refs:
        s, r = _renderer()
        r.configure(w, h, shadows=True, light=light, counters=False)
        r.render()
        fb = r.framebuffer()
        fb.setflags(write=False)
        _refs[key] = fb
        r.close()
        s.close()
    return _refs[key]


def _alternate(r, w, h, lights, frames=FRAMES, policy=None, prev=True):
    """configure, then `frames` frames started with no wait in between, the
    light alternating lights[0], lights[1], ...; returns (last, before last)."""
    r.configure(w, h, shadows=True, light=lights[0], counters=False)
    if policy is not None:
        r.set_list_policy(policy)
    for i in range(frames):
        r.set_light(lights[i % 2])
        r.start()
    r.wait()
    return r.framebuffer(), r.framebuffer_prev() if prev else None


def test_reference_frames_equal_oracle(oracle_lib):
    po = oracle_lib
    w, h = 200, 136
    s = rt.Scene.load(scene_path("tekkaman"))
    osc = po.OracleScene(po.cgltrace.load(scene_path("tekkaman")))
    for light in (A, B):
        c, _, _, _ = po.rt_render(osc, po.rt_params(w, h, shadows=True, light=light, nthreads=8),
                                  bvh=s.bvh() + (s.bvh4(),))
        assert np.array_equal(_ref(w, h, light), c), light
    assert not np.array_equal(_ref(w, h, A), _ref(w, h, B))  # the lights tell the frames apart
    s.close()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("w,h", SIZES)
def test_alternating_lights_back_to_back(w, h, shift):
    lights = (A, B) if shift == 0 else (B, A)
    s, r = _renderer()
    last, prev = _alternate(r, w, h, lights)
    # frame FRAMES - 1 carries lights[1], the one before it lights[0]
    assert np.array_equal(last, _ref(w, h, lights[1]))
    assert np.array_equal(prev, _ref(w, h, lights[0]))
    r.close()
    s.close()


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("w,h", SIZES)
def test_lists_rebuilt_between_overlapped_frames(w, h, shift):
    lights = (A, B) if shift == 0 else (B, A)
    s, r = _renderer()
    last, prev = _alternate(r, w, h, lights, policy=0)
    assert np.array_equal(last, _ref(w, h, lights[1]))
    assert np.array_equal(prev, _ref(w, h, lights[0]))
    ss = r.setup_stats()
    assert (ss["slist_on"], ss["slist_stale"]) == (1, 0), ss
    sidx, slist = r.records("sidx").copy(), r.records("slist").copy()
    r.close()
    s.close()
    # the lists a fresh renderer's configure builds for the last light (the
    # lists are sorted: the comparison is exact)
    s2, r2 = _renderer()
    r2.configure(w, h, shadows=True, light=lights[1], counters=False)
    assert r2.setup_stats()["slist_built"] == 1
    assert np.array_equal(sidx, r2.records("sidx"))
    assert np.array_equal(slist.view(np.uint32), r2.records("slist").view(np.uint32))
    r2.close()
    s2.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_lists_rebuilt_every_fourth_frame(w, h):
    """The light changes before every fourth frame and its lists are queued
    at once: three of four frames follow a frame (overlapped), the fourth
    follows the setup launches, which wait for both frames in flight."""
    s, r = _renderer()
    r.configure(w, h, shadows=True, light=A, counters=False)
    r.set_list_policy(0)
    for i in range(FRAMES + 1):
        if i % 4 == 0:
            r.set_light((A, B)[(i // 4) % 2])
        r.start()
    r.wait()
    # frame 64 is the first of A's group, frame 63 the last of B's
    assert np.array_equal(r.framebuffer(), _ref(w, h, A))
    assert np.array_equal(r.framebuffer_prev(), _ref(w, h, B))
    ss = r.setup_stats()
    assert (ss["slist_on"], ss["slist_stale"]) == (1, 0), ss
    r.close()
    s.close()


def _hip_runtime():
    """The HIP runtime the driver plugin loaded, by the path it is mapped from."""
    with open("/proc/self/maps") as f:
        for line in f:
            path = line.split()[-1]
            if os.path.basename(path).startswith("libamdhip64.so"):
                return ctypes.CDLL(path)
    raise RuntimeError("the driver has not loaded libamdhip64")


def _device_bytes(ptr, nbytes):
    hip = _hip_runtime()
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.zeros(nbytes // 4, np.uint32)
    assert hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return out


@pytest.mark.parametrize("before", [3, 4])  # the last frame before the call in buffer 0 / buffer 1
def test_framebuffer_device_falls_back_to_one_buffer(before):
    w, h = 200, 136
    s, r = _renderer()
    r.configure(w, h, shadows=True, light=A, counters=False)
    for _ in range(before):
        r.start()
    ptr, nbytes = r.framebuffer_device()
    assert nbytes == w * h * 4
    r.wait()
    assert np.array_equal(_device_bytes(ptr, nbytes).reshape(h, w), _ref(w, h, A))
    for i in range(6):  # B, A, B, ... : every frame lands in the pointer's buffer
        r.set_light((B, A)[i % 2])
        r.start()
    r.wait()
    assert np.array_equal(r.framebuffer(), _ref(w, h, A))
    assert np.array_equal(_device_bytes(ptr, nbytes).reshape(h, w), _ref(w, h, A))
    r.set_light(B)
    r.render()
    assert np.array_equal(_device_bytes(ptr, nbytes).reshape(h, w), _ref(w, h, B))
    assert np.array_equal(r.framebuffer(), _ref(w, h, B))
    with pytest.raises(rt.RtError):  # one buffer: no earlier frame is kept
        r.framebuffer_prev()
    r.close()
    s.close()


COUNTERS = ("primary_rays", "shadow_rays", "geometry_hits", "occluded", "node_visits", "tri_tests",
            "layer_tests", "shaded", "tasks")


@pytest.mark.parametrize("kw", [dict(compact=True, counters=True), dict(instrumented=True)],
                         ids=["compact", "instrumented"])
def test_ineligible_configurations_stay_ordered(kw):
    w, h = 200, 136
    s, r = _renderer()
    r.configure(w, h, shadows=True, light=A, **kw)
    r.render()  # one frame alone: the non-overlapped run
    alone, fb_alone = r.stats(), r.framebuffer().copy()
    for _ in range(8):
        r.start()
    r.wait()
    st = r.stats()
    for k in COUNTERS:
        assert st[k] == alone[k], k
    assert alone["primary_rays"] > 0
    assert np.array_equal(r.framebuffer(), fb_alone)
    with pytest.raises(rt.RtError):  # the ordered path: one framebuffer
        r.framebuffer_prev()
    if not kw.get("compact"):
        assert np.array_equal(fb_alone, _ref(w, h, A))
    r.close()
    s.close()


def _child(out_path):
    """The first test's sequences in this process (run with VX_HIP_OVERLAP=0)."""
    frames = {}
    for w, h in SIZES:
        for shift in (0, 1):
            lights = (A, B) if shift == 0 else (B, A)
            s, r = _renderer()
            last, _ = _alternate(r, w, h, lights, prev=False)
            frames[f"last_{w}_{h}_{shift}"] = last
            # one lane, one framebuffer: the frames ran one after the other
            # into the same pixels and no earlier frame is kept
            try:
                r.framebuffer_prev()
                raise SystemExit("VX_HIP_OVERLAP=0 still keeps two framebuffers")
            except rt.RtError:
                pass
            r.close()
            s.close()
    np.savez(out_path, **frames)


def test_overlap_off_gives_the_same_bytes(tmp_path):
    out = str(tmp_path / "frames.npz")
    env = dict(os.environ, VX_HIP_OVERLAP="0", SKYBOX_RT_NO_TORCH="1",
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.load(out)
    for w, h in SIZES:
        for shift in (0, 1):
            lights = (A, B) if shift == 0 else (B, A)
            assert np.array_equal(got[f"last_{w}_{h}_{shift}"], _ref(w, h, lights[1]))


def test_queue_depth_one_renders_synchronously(monkeypatch):
    w, h = 200, 136
    monkeypatch.setenv("VX_HIP_QUEUE_DEPTH", "1")  # read when the renderer opens its device
    s, r = _renderer()
    r.configure(w, h, shadows=True, light=A, counters=False)
    _, _, n0 = r.run_totals()
    for i in range(32):
        light = (A, B)[i % 2]
        r.set_light(light)
        r.render()
        assert np.array_equal(r.framebuffer(), _ref(w, h, light)), i
    _, _, n1 = r.run_totals()
    assert n1 - n0 == 32
    r.close()
    s.close()


if __name__ == "__main__":
    _child(sys.argv[1])
