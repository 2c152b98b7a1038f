"""GPU tests of the denoiser (vx_rt.h rt_denoise_capture_start /
rt_render_denoise_start; images rt_aov_guide -- kernels/rt_aov_kernel.hip with
RT_AOV_BASE=2 -- rt_denoise_prep and rt_denoise_pass, kernels/
rt_denoise_kernel.hip).

The guide is held to what the project already pins: pid, depth word and
geometry flag to Renderer.aov() of the primary+shadow configuration (itself
held to the oracle by tests/test_gpu_aov.py), the base colours to the oracle's
unshadowed frame, the normals to a float64 restatement from the exported
triangle records.  The filtered frame must equal the numpy model of
tests/denoise_reference.py on the read-back inputs bit for bit, over the
parameter space, after 1 and 4 samples, under two path lights and on extreme
records; accumulation must go on unchanged behind it.  No reference exists for
this row."""
import numpy as np
import pytest

import denoise_reference as dr
from conftest import scene_path
from test_gpu_light import LIGHTS

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402

S0 = 0x5EED
GEOM = np.uint32(rt.RT_AOV_GEOM)
_state = {}
_plain = {}


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def renderer(name="tekkaman"):
    if name not in _state:
        s = rt.Scene.load(scene_path(name))
        _state[name] = (s, rt.Renderer(s), s.bvh() + (s.bvh4(),))
    return _state[name][1]


def unshadowed(po, name, w, h):
    """the oracle's frame without shadows; computed once, left unchanged"""
    key = (name, w, h)
    if key not in _plain:
        renderer(name)
        osc = po.OracleScene(po.cgltrace.load(scene_path(name)))
        c = po.rt_render(osc, po.rt_params(w, h, shadows=False, nthreads=8), bvh=_state[name][2])[0]
        c.setflags(write=False)
        _plain[key] = c
    return _plain[key]


def path_frame(r, w, h, bounces=4, seed=S0, **kw):
    r.configure(w, h, path=True, bounces=bounces, seed=seed, **kw)
    r.accum_begin()


def guide_fields(r):
    g, base = r.denoise_guide()
    return dict(pid=g["pid"], z=g["depth_flags"] & np.uint32(0xFFFFFF), geom=(g["depth_flags"] & GEOM) != 0,
                base=base, normal=dr.unpack_normal(g["normal"]))


def same(got, want, what=""):
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} pixels differ"


# ---- the guide ----------------------------------------------------------------------

@pytest.mark.parametrize("name,w,h", [("tekkaman", 128, 128), ("tekkaman", 200, 136), ("triangle", 64, 64)])
def test_guide(po, name, w, h):
    r = renderer(name)
    r.configure(w, h, shadows=True)
    want = r.aov().copy()
    path_frame(r, w, h)
    r.accumulate(2)
    fb, acc = r.framebuffer().copy(), r.accum().copy()
    r.denoise_capture()
    g, base = r.denoise_guide()
    assert np.array_equal(g["pid"], want["pid"]), f"{int((g['pid'] != want['pid']).sum())} pids differ"
    keep = np.uint32(0xFFFFFF) | GEOM
    assert np.array_equal(g["depth_flags"], want["depth_flags"] & keep), "depth word / geometry flag"
    assert not g["reserved"].any() and not (g["normal"] >> np.uint32(24)).any()
    same(base, unshadowed(po, name, w, h), "base colours")
    geom = (g["depth_flags"] & GEOM) != 0
    if name == "tekkaman":
        assert geom.sum() > 1000
    N, ref = dr.unpack_normal(g["normal"]), dr.normals_f64(r.records("ptris"), g["pid"], geom)
    assert int(np.abs(N - ref)[geom].max(initial=0)) <= 1, "a normal component is more than 1 from the float64 restatement"
    assert not N[~geom].any()
    assert (np.abs(N[geom]).max(-1) > 0).all()      # (these scenes have no degenerate visible triangle)
    # a capture writes neither the framebuffer nor a record
    same(r.framebuffer(), fb, "framebuffer after the capture")
    assert np.array_equal(r.accum(), acc)


# ---- the filter -----------------------------------------------------------------------

def sweep(r, rec, what):
    """every passes x zs x ls of the issue's grid: the device frame against the model on the read-back
    inputs (the model's frames of passes 1..5 share their passes)"""
    g = guide_fields(r)
    for zs in (0, 8, 23):
        for ls in (0, 6, 16):
            want = dr.frames(rec, passes=5, zs=zs, ls=ls, **g)
            for p in range(1, 6):
                r.denoise(passes=p, depth_shift=zs, color_shift=ls)
                same(r.framebuffer(), want[p - 1], f"{what} passes={p} zs={zs} ls={ls}")
    return g


@pytest.mark.parametrize("w,h", [(128, 128), (200, 136)])
@pytest.mark.parametrize("samples", [1, 4])
def test_filter_equals_model(w, h, samples):
    r = renderer()
    path_frame(r, w, h)
    r.denoise_capture()
    r.accumulate(samples)
    rec = r.accum().copy()
    assert (rec[..., 3] == samples).all()
    g = sweep(r, rec, f"{w}x{h} n={samples}")
    # the filter moved pixels (it is not the resolve) and left the pixels without geometry alone
    r.denoise(passes=5, depth_shift=23, color_shift=16)
    fb = r.framebuffer()
    raw = dr.accum_resolve(rec, g["base"])
    assert int((fb != raw)[g["geom"]].sum()) > 100
    same(fb[~g["geom"]], raw[~g["geom"]], "pixels without geometry")


@pytest.mark.parametrize("w,h", [(128, 128), (200, 136)])
def test_filter_under_two_path_lights(w, h):
    r = renderer()
    path_frame(r, w, h)
    r.denoise_capture()
    r.set_path_lights(LIGHTS[:2])              # (the guide survives: it depends on view and size only)
    r.accumulate(4)
    rec = r.accum().copy()
    assert (rec[..., 3] == 4).all()
    sweep(r, rec, f"two lights {w}x{h}")


@pytest.mark.parametrize("n", [1 << 24, 1])
def test_extreme_records(n):
    w = h = 128
    r = renderer()
    path_frame(r, w, h)
    r.denoise_capture()
    rng = np.random.default_rng(n & 0xFFFF)
    rec = np.zeros((h, w, 4), np.uint32)
    rec[..., :3] = rng.integers(0, 255 * n + 1, (h, w, 3), dtype=np.uint64)
    rec[..., 3] = n
    rec[::7, ::5, :3] = 255 * n
    rec[3::7, 2::5, :3] = 0
    r.write_accum(rec)
    assert r.accum_samples() == n and np.array_equal(r.accum(), rec)
    g = guide_fields(r)
    for p, zs, ls in [(1, 0, 0), (5, 23, 16), (3, 8, 6), (5, 0, 16)]:
        r.denoise(passes=p, depth_shift=zs, color_shift=ls)
        same(r.framebuffer(), dr.denoise(rec, passes=p, zs=zs, ls=ls, **g), f"n={n} passes={p} zs={zs} ls={ls}")


# ---- continuation ---------------------------------------------------------------------

def test_accumulation_goes_on(po):
    from test_gpu_accum import model
    w = h = 128
    r = renderer()
    path_frame(r, w, h)
    r.denoise_capture()
    r.accumulate(2)
    acc = r.accum().copy()
    r.denoise()
    assert np.array_equal(r.accum(), acc), "denoise wrote an accumulation record"
    assert r.accum_samples() == 2
    r.accumulate(2)
    rec4, frame4 = model(po, "tekkaman", w, 4, S0, 4)
    assert np.array_equal(r.accum(), rec4)
    same(r.framebuffer(), frame4, "the frame of 4 samples after a denoise")
    # checkpoint and resume: the saved records written back, then two more samples
    saved = r.accum().copy()
    r.accumulate(2)
    rec6, frame6 = model(po, "tekkaman", w, 4, S0, 6)
    assert np.array_equal(r.accum(), rec6)
    r.accum_reset()
    r.write_accum(saved)
    assert r.accum_samples() == 4
    r.accumulate(2)
    assert np.array_equal(r.accum(), rec6)
    same(r.framebuffer(), frame6, "resumed accumulation")
    # records whose n differ, or an n out of range, are refused
    bad = saved.copy()
    bad[5, 5, 3] += 1
    _refused(r.write_accum, bad)
    bad = saved.copy()
    bad[..., 3] = 0
    _refused(r.write_accum, bad)


# ---- refusals, lifecycle -------------------------------------------------------------

def _refused(fn, *a, **kw):
    with pytest.raises(rt.RtError, match=r"\(-2\)"):
        fn(*a, **kw)


def test_refusals():
    w = h = 128
    r = renderer()
    r.configure(w, h, path=True, bounces=4, seed=S0, compact=True)
    _refused(r.denoise_capture)                       # compact output
    r.configure(w, h, shadows=True)
    _refused(r.denoise_capture)                       # what accum_begin refuses
    path_frame(r, w, h)
    r.accumulate(1)
    _refused(r.denoise)                               # no capture
    r.denoise_capture()
    r.accum_reset()
    _refused(r.denoise)                               # no samples
    r.accumulate(1)
    _refused(r.denoise, passes=0)
    _refused(r.denoise, passes=6)
    _refused(r.denoise, depth_shift=24)
    _refused(r.denoise, color_shift=17)
    r.denoise()
    path_frame(r, w, h)                               # a new configure releases the guide
    r.accumulate(1)
    _refused(r.denoise)
    with pytest.raises(rt.RtError):
        r.denoise_guide()
    fb = r.framebuffer()
    r.accum_reset()
    r.accumulate(1)
    same(r.framebuffer(), fb, "the renderer after the refusals")


def test_queued_behind_overlapped_frames():
    """capture, samples and two filters queued back to back behind two frames in flight, one wait"""
    w = h = 128
    r = renderer()
    path_frame(r, w, h, counters=False)
    r.start()
    r.start()
    r.denoise_capture(wait=False)
    r.accumulate(3, wait=False)
    r.denoise(passes=5, depth_shift=8, color_shift=6, wait=False)
    r.denoise(passes=3, depth_shift=8, color_shift=6, wait=False)
    r.wait()
    assert r.kernel_ms() > 0
    rec = r.accum()
    assert (rec[..., 3] == 3).all()
    g = guide_fields(r)
    same(r.framebuffer(), dr.denoise(rec, passes=3, zs=8, ls=6, **g), "the last queued filter")
    # and a frame started behind it is the plain path frame
    r.denoise(wait=False)
    r.start()
    r.wait()
    r.accum_reset()
    r.accumulate(1)
    one = r.framebuffer().copy()
    r.render()
    same(r.framebuffer(), one, "a plain frame after the filter")


# ---- it helps --------------------------------------------------------------------------

def test_denoised_frame_is_closer_to_the_converged_one():
    """128^2, 4 bounces, the defaults: squared error over the geometry pixels of the denoised 4-sample
    frame against a 512-sample accumulation of disjoint seeds, over the raw 4-sample frame's"""
    w = h = 128
    r = renderer()
    path_frame(r, w, h, seed=S0 + 1000)
    for _ in range(16):
        r.accumulate(32, wait=False)
    r.wait()
    rec = r.accum().astype(np.float64)
    ref = rec[..., :3] / rec[..., 3:4]
    assert (rec[..., 3] == 512).all()
    path_frame(r, w, h, seed=S0)
    r.denoise_capture()
    r.accumulate(4)
    raw = r.framebuffer().copy()
    r.denoise()
    den = r.framebuffer()
    geom = guide_fields(r)["geom"]
    e_raw = float(((dr.channels(raw).astype(np.float64) - ref)[geom] ** 2).sum())
    e_den = float(((dr.channels(den).astype(np.float64) - ref)[geom] ** 2).sum())
    print(f"squared error over {int(geom.sum())} geometry pixels: raw {e_raw:.1f}, denoised {e_den:.1f}, "
          f"ratio {e_den / e_raw:.4f}")
    assert e_raw > 0 and e_den / e_raw < 1
