"""GPU test (MI355X) of the shadow-list rounds of image rt_kernel with their
record loads issued in one batch (kernels/rt_trace.h slist_scan under
RT_SLIST_BATCH): the knob changes when a round's six rows
are loaded, never what is tested, so every frame and every ray counter must
stay the oracle's.

Tekkaman at 40x24 (blocks overhang the image's edge) and at 64x64 under the
default light (0, 60, 80), a light off to the side (30, -20, 95) and one inside
the model (0, 0, 0.5), and one set_light next to the model (5, 5, 99.5) under
set_list_policy(0) -- lists that exceed their capacity and are refilled:

* each case rendered synchronously and as four overlapped frames, with
  RT_FUSED_CHUNK 1 (the scan in place behind the shade) and 0 (the queue and
  both drains): the three scan sites of the image -- every frame equals the
  oracle's bit for bit;
* the plain image's shadow_rays and occluded equal the oracle's.

test_cases_hold_every_kind asserts from the oracle's counters that the cases
hold lit and occluded rays, and from the oracle's lists (each shadow ray's cell
restated here from the oracle's pid and t arrays, checked against its ray count)
that rays reach cells of odd and of even length -- an odd list ends on the
padding record a round reads past it -- and cells of three rounds and more.
No test asserts a time, none looks at the image's code."""
import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402

LIGHTS = ((0.0, 60.0, 80.0), (30.0, -20.0, 95.0), (0.0, 0.0, 0.5))
NEXT_TO_MODEL = (5.0, 5.0, 99.5)  # tests/test_gpu_light.py: its lists exceed the capacity
SIZES = ((40, 24), (64, 64))
CASES = [(w, h, L) for w, h in SIZES for L in LIGHTS]
KNOBS = ("RT_FUSED_CHUNK", "RT_BG_TIER", "RT_LANE_CHUNKS", "RT_BG_COST", "RT_BG_LAYERS", "RT_BG_STALE")

_state, _ref = {}, {}


@pytest.fixture(scope="module")
def renderer():
    s = rt.Scene.load(scene_path("tekkaman"))
    r = rt.Renderer(s)
    _state["scene"] = s
    yield r
    r.close()
    s.close()
    _state.clear()


def _oscene(po):
    if "osc" not in _state:
        _state["osc"] = po.OracleScene(po.cgltrace.load(scene_path("tekkaman")))
    return _state["osc"]


def _oracle(po, w, h, light):
    """(colour, pid, t, counters) of the oracle's frame, once per case, left unchanged"""
    key = (w, h, light)
    if key not in _ref:
        s = _state["scene"]
        c, pid, t, k = po.rt_render(_oscene(po), po.rt_params(w, h, shadows=True, light=light, nthreads=8),
                                    bvh=s.bvh() + (s.bvh4(),))
        for a in (c, pid, t):
            a.setflags(write=False)
        _ref[key] = (c, pid, t, k)
    return _ref[key]


def _sync_and_overlapped(r, ref):
    r.render()
    assert np.array_equal(r.framebuffer(), ref)
    for _ in range(4):
        r.start()
    r.wait()
    assert np.array_equal(r.framebuffer(), ref)
    assert np.array_equal(r.framebuffer_prev(), ref)


def _configure(r, m, w, h, light, fused, **kw):
    for k in KNOBS:
        m.delenv(k, raising=False)
    m.setenv("RT_FUSED_CHUNK", "1" if fused else "0")
    r.configure(w, h, shadows=True, light=light, **kw)
    assert r.setup_stats()["fused_chunk"] == (1 if fused else 0)
    assert r.setup_stats()["slist_on"] == 1


@pytest.mark.parametrize("w,h,light", CASES)
def test_frames_and_counters_equal_oracle(oracle_lib, renderer, monkeypatch, w, h, light):
    r = renderer
    ref, _, _, k = _oracle(oracle_lib, w, h, light)
    for fused in (True, False):
        with monkeypatch.context() as m:
            _configure(r, m, w, h, light, fused, counters=False)
            _sync_and_overlapped(r, ref)
            # the plain image's ray counters
            _configure(r, m, w, h, light, fused)
            r.render()
            st = r.stats()
            assert np.array_equal(r.framebuffer(), ref)
            for key in ("shadow_rays", "occluded"):
                assert st[key] == k[key], (key, fused)


@pytest.mark.parametrize("w,h", SIZES)
def test_set_light_next_to_the_model_refilled_lists(oracle_lib, renderer, monkeypatch, w, h):
    r = renderer
    ref, _, _, k = _oracle(oracle_lib, w, h, NEXT_TO_MODEL)
    for fused in (True, False):
        with monkeypatch.context() as m:
            r.set_list_policy(0)
            try:
                for counters in (False, True):
                    _configure(r, m, w, h, LIGHTS[0], fused, counters=counters)
                    r.set_light(NEXT_TO_MODEL)
                    ss = r.setup_stats()  # the status read settles the lists: refilled at their exact size
                    assert ss["slist_on"] == 1 and ss["slist_stale"] == 0, ss
                    if not counters:
                        _sync_and_overlapped(r, ref)
                        continue
                    r.render()  # the plain image's ray counters
                    st = r.stats()
                    assert np.array_equal(r.framebuffer(), ref)
                    for key in ("shadow_rays", "occluded"):
                        assert st[key] == k[key], (key, fused)
            finally:
                r.set_list_policy(8)  # (rt_renderer_set_list_policy's default)


def _ray_cells(po, w, h, light, pid, t):
    """The light-space cell of every shadow ray of the oracle's frame (oracle/rt.c rt_row, sl_cell_of,
    restated in float32; the fused multiply-adds through float64, whose product is exact)."""
    sc = po.cgltrace.load(scene_path("tekkaman"))
    layer = np.zeros(sc.num_prims + 1, bool)
    for dc in sc.drawcalls:
        if not dc.states["depth_test"]:
            layer[dc.prim_offset:dc.prim_offset + dc.prim_count] = True
    p = np.array(pid, np.int64)
    f32 = np.float32
    with np.errstate(all="ignore"):
        ray = (p >= 0) & ~layer[np.clip(p, 0, sc.num_prims)] & (t > 0) & np.isfinite(t)
        ys, xs = np.nonzero(ray)
        sx, sy = f32(2.0) / f32(w), f32(2.0) / f32(h)
        dx = ((xs + 0.5) * np.float64(sx) - 1.0).astype(f32)
        dy = ((ys + 0.5) * np.float64(sy) - 1.0).astype(f32)
        tt = (t[ys, xs] * f32(0.999755859375)).astype(f32)
        so = np.stack([dx * tt, dy * tt, tt], 1).astype(f32)
        u = -(np.array(light, f32)[None, :] - so).astype(f32)
    a = np.abs(u)
    k = np.zeros(len(u), np.int64)
    m = a[:, 0].copy()
    for j in (1, 2):
        up = a[:, j] > m
        k[up] = j
        m[up] = a[up, j]
    rows = np.arange(len(u))
    ax = np.array([[1, 2], [0, 2], [0, 1]])
    f = 2 * k + (u[rows, k] < 0)
    hn = f32(po.SL_N * 0.5)
    cx = np.clip(np.floor((u[rows, ax[k, 0]] / m + f32(1.0)) * hn).astype(np.int64), 0, po.SL_N - 1)
    cy = np.clip(np.floor((u[rows, ax[k, 1]] / m + f32(1.0)) * hn).astype(np.int64), 0, po.SL_N - 1)
    return (f * po.SL_N + cy) * po.SL_N + cx


def test_cases_hold_every_kind(oracle_lib, renderer):
    po = oracle_lib
    lit = occluded = odd = even = long_ = 0
    for w, h, light in CASES + [(w, h, NEXT_TO_MODEL) for w, h in SIZES]:
        _, pid, t, k = _oracle(po, w, h, light)
        lit += k["shadow_rays"] - k["occluded"]
        occluded += k["occluded"]
        cells = _ray_cells(po, w, h, light, pid, t)
        assert len(cells) == k["shadow_rays"]  # the restatement finds the oracle's rays
        idx, _ = po.shadow_lists(_oscene(po), light)
        n = idx[cells, 1].astype(np.int64)
        odd += int(((n & 1) == 1).sum())
        even += int(((n > 0) & ((n & 1) == 0)).sum())
        long_ += int((n >= 5).sum())
    print(f"rays lit {lit}, occluded {occluded}; rays in cells of odd length {odd}, of even length {even}, "
          f"of three rounds and more {long_}")
    assert lit > 0 and occluded > 0 and odd > 0 and even > 0 and long_ > 0
    # 64x64 under the default light alone holds lit and occluded rays
    _, _, _, k = _oracle(po, 64, 64, LIGHTS[0])
    assert 0 < k["occluded"] < k["shadow_rays"]
