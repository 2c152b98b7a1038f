"""GPU tests of relighting from the visibility records (vx_rt.h
rt_relight_capture_start / rt_render_relight_start; images rt_aov_base --
kernels/rt_aov_kernel.hip with RT_AOV_BASE -- and rt_relight,
kernels/rt_relight_kernel.hip) against the untouched oracle, bit for bit.

The model is built from frames the oracle already produces: the capture's base
colours are its frame without shadows; a relit frame under weights w_i is, per
pixel and channel, (2 * sum w_i f_i + W) // (2 * W) over the single-light
RT_RENDER_SHADOWS frames f_i, under their common alpha; with weights 0 / 1 that
is test_gpu_lights.mean_frame of the enabled lights, which a fresh set_lights
frame of them must equal too.  No reference exists for this row."""
import os
import subprocess

import numpy as np
import pytest

from conftest import scene_path
from test_gpu_light import LIGHTS
from test_gpu_lights import SIXTEEN, mean_frame, single

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, rt  # noqa: E402

RAMP = list(range(1, 17))
_state = {}


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


def renderer(key=""):
    if key not in _state:
        s = rt.Scene.load(scene_path("tekkaman"))
        _state[key] = (s, rt.Renderer(s))
    return _state[key][1]


def weighted_frame(po, w, h, lights, weights):
    """(2 * sum w_i f_i + W) // (2 * W) per channel over the oracle's single-light frames"""
    fr = [single(po, w, h, L)[0] for L in lights]
    W = int(sum(weights))
    out = fr[0] & np.uint32(0xFF000000)
    for sh in (16, 8, 0):
        tot = sum(np.uint64(wi) * ((c >> np.uint32(sh)) & np.uint32(0xFF)).astype(np.uint64)
                  for wi, c in zip(weights, fr))
        out = out | (((2 * tot + W) // (2 * W)).astype(np.uint32) << np.uint32(sh))
    return out


def captured(r, w, h, lights, **kw):
    """configure, light and capture; the renderer is ready for relight()"""
    r.configure(w, h, shadows=True, light=lights[0], **kw)
    if len(lights) > 1:
        r.set_lights(lights)
    r.relight_capture()


def same(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} pixels differ"


# ---- the capture ----------------------------------------------------------------

@pytest.mark.parametrize("w,h,lights", [(128, 128, LIGHTS[:1]), (128, 128, LIGHTS[:3]), (128, 128, LIGHTS),
                                        (128, 128, SIXTEEN), (200, 136, LIGHTS[:3])],
                         ids=["128-K1", "128-K3", "128-K5", "128-K16", "200x136-K3"])
def test_capture_and_unit_weights(po, w, h, lights):
    K = len(lights)
    r = renderer()
    r.configure(w, h, shadows=True, light=lights[0])
    if K > 1:
        r.set_lights(lights)
    want_rec = r.aov().copy()
    r.render()
    frame = r.framebuffer().copy()          # the K-light frame of unchanged code
    r.relight_capture()
    rec = r.aov_records()
    assert np.array_equal(rec.view(np.uint32), want_rec.view(np.uint32)), "the capture's records are not rt_aov's"
    same(r.relight_base(), single(po, w, h, LIGHTS[0], shadows=False)[0])
    same(r.framebuffer(), frame)            # a capture writes no framebuffer
    r.relight([1] * K)
    assert r.kernel_ms() > 0
    got = r.framebuffer()
    same(got, frame)
    same(got, mean_frame(po, w, h, lights, min_mixed=100 if K > 1 else 0))
    # and the host's restatement on the buffers read back
    same(rt.relight_resolve(r.relight_base(), rec["depth_flags"], rec["light_mask"], [1] * K), got)


# ---- weights -----------------------------------------------------------------------

SUBSETS = [(LIGHTS[:3], [0]), (LIGHTS[:3], [1]), (LIGHTS[:3], [2]), (LIGHTS[:3], [0, 2]),
           (SIXTEEN, list(range(1, 16, 2)))]


@pytest.mark.parametrize("lights,on", SUBSETS, ids=["K3-0", "K3-1", "K3-2", "K3-02", "K16-odd"])
def test_subsets_by_zero_one_weights(po, lights, on):
    w = h = 128
    r = renderer()
    captured(r, w, h, lights)
    mean_frame(po, w, h, lights, min_mixed=100)   # the captured lights disagree on >= 100 pixels
    sub = [lights[i] for i in on]
    r.relight([1 if i in on else 0 for i in range(len(lights))])
    got = r.framebuffer()
    same(got, mean_frame(po, w, h, sub, min_mixed=100 if len(sub) > 1 else 0))
    if len(sub) == 1:   # the light alone sees pixels another captured light does not, or the reverse
        others = [single(po, w, h, L)[0] for L in lights if L != sub[0]]
        assert max(int((o != got).sum()) for o in others) >= 100
    r.set_lights(sub)   # (ends the capture)
    r.render()
    same(r.framebuffer(), got)


@pytest.mark.parametrize("lights,weights", [(LIGHTS[:3], [255, 64, 1]), (SIXTEEN, RAMP)], ids=["K3", "K16-ramp"])
def test_weighted(po, lights, weights):
    w = h = 128
    r = renderer()
    captured(r, w, h, lights)
    r.relight(weights)
    got = r.framebuffer()
    want = weighted_frame(po, w, h, lights, weights)
    same(got, want)
    unit = mean_frame(po, w, h, lights, min_mixed=100)
    assert int((want != unit).sum()) >= 100, "the weights change too few pixels to show"
    same(rt.relight_resolve(r.relight_base(), r.aov_records()["depth_flags"], r.aov_records()["light_mask"], weights),
         got)


def test_one_light(po):
    r = renderer()
    r.configure(128, 128, shadows=True, light=LIGHTS[1])
    r.relight_capture()
    r.relight([7])
    same(r.framebuffer(), single(po, 128, 128, LIGHTS[1])[0])
    r.set_light(LIGHTS[3])                  # a moved light: its own capture
    with pytest.raises(rt.RtError, match=r"\(-2\)"):
        r.relight([7])
    r.relight_capture()
    r.relight([200])
    same(r.framebuffer(), single(po, 128, 128, LIGHTS[3])[0])


# ---- compact and sharded framebuffers -----------------------------------------------

def test_two_shards_and_compact(po):
    w = h = 128
    lights, weights = LIGHTS[:3], [255, 64, 1]
    want = weighted_frame(po, w, h, lights, weights)
    r = renderer()
    parts = []
    for i in range(2):
        captured(r, w, h, lights, shard_index=i, shard_count=2)
        r.relight(weights)
        fb = r.framebuffer()
        assert fb.shape == (r.stats()["local_tiles"] * 1024,)
        parts.append(fb.copy())
    same(rt.deinterleave_tiles(parts, w, h), want)
    captured(r, w, h, lights, compact=True)
    r.relight(weights)
    same(rt.deinterleave_tiles([r.framebuffer()], w, h), want)


def test_compact_partial_tiles(po):
    """tiles overhanging the image: their pixels outside it stay as a frame leaves them"""
    w, h = 200, 136
    lights = LIGHTS[:3]
    r = renderer()
    r.configure(w, h, shadows=True, light=lights[0], compact=True)
    r.set_lights(lights)
    r.render()
    frame = r.framebuffer().copy()
    r.relight_capture()
    r.relight([1, 1, 1])
    same(r.framebuffer(), frame)
    same(rt.deinterleave_tiles([r.framebuffer()], w, h), mean_frame(po, w, h, lights))
    r.relight([0, 0, 9])
    same(rt.deinterleave_tiles([r.framebuffer()], w, h), single(po, w, h, lights[2])[0])


# ---- state ----------------------------------------------------------------------------

def _refused(fn, *a):
    with pytest.raises(rt.RtError, match=r"\(-2\)"):
        fn(*a)


def test_state(po):
    w = h = 128
    lights = LIGHTS[:3]
    s = rt.Scene.load(scene_path("tekkaman"))
    r = rt.Renderer(s)
    with pytest.raises(rt.RtError):
        r.relight_capture()                                 # before any configure
    r.configure(w, h, shadows=True, light=lights[0])
    _refused(r.relight, [1])                                # before a capture
    with pytest.raises(rt.RtError):
        r.relight_base()
    r.set_lights(lights)
    _refused(r.relight, [1, 1, 1])                          # still none
    r.relight_capture()
    _refused(r.relight, [1, 1])                             # a wrong n
    _refused(r.relight, [1, 1, 1, 1])
    _refused(r.relight, [0, 0, 0])                          # every weight 0
    _refused(r.relight, [0, 0, 0], False)
    with pytest.raises(rt.RtError):
        r.relight([1, 256, 1])
    r.relight([0, 1, 0])                                    # the refusals left the capture alone
    same(r.framebuffer(), single(po, w, h, lights[1])[0])
    # each of these ends the session
    r.set_light(lights[1])
    _refused(r.relight, [1, 1, 1])
    _refused(r.relight, [1])
    r.relight_capture()
    r.relight([3])
    same(r.framebuffer(), single(po, w, h, lights[1])[0])
    r.set_lights(lights[:2])
    _refused(r.relight, [1])
    _refused(r.relight, [1, 1])
    r.relight_capture()
    r.relight([1, 1])
    same(r.framebuffer(), mean_frame(po, w, h, lights[:2]))
    r.configure(w, h, shadows=True, light=lights[0])
    _refused(r.relight, [1, 1])
    _refused(r.relight, [1])
    with pytest.raises(rt.RtError):
        r.relight_base()                                    # the configure released the buffers
    r.close()
    s.close()


def test_render_between_capture_and_relight(po):
    w = h = 128
    lights = LIGHTS[:3]
    r = renderer()
    captured(r, w, h, lights)
    rec = r.aov_records().copy()
    base = r.relight_base().copy()
    r.render()
    r.start()
    r.start()
    r.wait()
    same(r.framebuffer(), mean_frame(po, w, h, lights))
    assert np.array_equal(r.aov_records().view(np.uint32), rec.view(np.uint32))
    same(r.relight_base(), base)
    r.relight([255, 64, 1])
    same(r.framebuffer(), weighted_frame(po, w, h, lights, [255, 64, 1]))
    # one light: frames flip between two framebuffers; the relight goes to the one in use
    r.configure(w, h, shadows=True, light=lights[2], counters=False)
    r.relight_capture()
    r.start()
    r.relight([1], wait=False)
    r.start()
    r.relight([5], wait=False)
    r.wait()
    same(r.framebuffer(), single(po, w, h, lights[2])[0])


def test_back_to_back(po):
    w = h = 128
    lights = LIGHTS[:3]
    r = renderer()
    captured(r, w, h, lights)
    r.relight([1, 0, 0], wait=False)
    r.relight([0, 0, 1], wait=False)
    r.relight([255, 64, 1], wait=False)
    r.wait()
    same(r.framebuffer(), weighted_frame(po, w, h, lights, [255, 64, 1]))
    assert r.kernel_ms() > 0


# ---- refusals of the capture -----------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(path=True), dict(flat=True), dict(raster=True, shadows=False),
                                dict(instrumented=True), dict(shadows=False)],
                         ids=["path", "flat", "raster", "instrumented", "no-shadows"])
def test_capture_refused(po, kw):
    r = renderer(key="/refusals")
    r.configure(128, 128, **dict(dict(shadows=True), **kw))
    _refused(r.relight_capture)
    _refused(r.relight_capture, False)
    _refused(r.relight, [1])
    r.render()                                              # the renderer still renders its frame
    if "instrumented" in kw:
        same(r.framebuffer(), single(po, 128, 128, LIGHTS[0])[0])
    if kw == dict(shadows=False):
        same(r.framebuffer(), single(po, 128, 128, LIGHTS[0], shadows=False)[0])


def test_capture_refused_ordered_tail(po):
    sv = rt.Scene.load(scene_path("vase"), om_layers=True)
    assert sv.om_split()[1] > 0
    ro = rt.Renderer(sv)
    ro.configure(128, 128, shadows=True)
    ro.render()
    want = ro.framebuffer().copy()
    _refused(ro.relight_capture)
    _refused(ro.relight, [1])
    ro.render()
    same(ro.framebuffer(), want)
    ro.close()
    sv.close()


# ---- the CLI -------------------------------------------------------------------------------

def _rtapp(*args):
    return subprocess.run([os.path.join(_lib.LIB_DIR, "rtapp"), "-t", scene_path("tekkaman"), "-w128", "-h128", *args],
                          capture_output=True, text=True, timeout=300)


def test_rtapp_relights(po, tmp_path):
    from PIL import Image
    out = tmp_path / "out.png"
    lights = LIGHTS[:3]
    arg = [f"{x:g},{y:g},{w:g}" for x, y, w in lights]
    p = _rtapp("-S", "-L", arg[0], "-M", arg[1], "-M", arg[2], "-W", "1,0,1", "-o", str(out))
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Relight: 3 lights, weights 1,0,1" in p.stdout, p.stdout
    got = np.array(Image.open(out).convert("RGBA"))
    want = po.argb_to_rgba_image(mean_frame(po, 128, 128, [lights[0], lights[2]]))
    assert po.compare_images(got, want, tol=0) == 0
    # the weight count is the light count, and -W needs -S: a usage error, nothing rendered
    for bad in (["-S", "-L", arg[0], "-M", arg[1], "-W", "1,0,1"], ["-S", "-L", arg[0], "-W", "1,300"],
                ["-L", arg[0], "-W", "1"]):
        p = _rtapp(*bad, "-o", "null")
        assert p.returncode != 0 and "Error: -W" in p.stdout and "Relight:" not in p.stdout, p.stdout
