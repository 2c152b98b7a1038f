"""GPU test (MI355X) of the key-specialised shading (gfx_device.h shade_keyed,
rt_trace.h shade_wave): every golden scene the RT path accepts rendered at
64^2 -- tekkaman and box through the specialised instantiations, carnival
(point filter), scene and triangle (untextured) through the generic shade() --
textured synthetic scenes (synth_tex_scene.py) whose bilinear drawcalls differ
from a specialised key only in the wraps, the format, or format and stride,
and a synthetic scene whose one untextured drawcall takes the generic
fallback; frame and counters, the instrumented image's included, against the
oracle."""
import numpy as np
import pytest

from conftest import scene_path
from test_shade_keys import load, rt_accepts, scene_names

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402

SIZE = 64
ACCEPTED = [n for n in scene_names() if rt_accepts(load(n))]


@pytest.fixture(scope="module")
def synth_path(tmp_path_factory):
    from synth_scene import make_scene
    return make_scene(str(tmp_path_factory.mktemp("keys") / "synth60.cgltrace.gz"), 60, seed=7, size=0.15)


def _check(po, path):
    s = rt.Scene.load(path)
    r = rt.Renderer(s)
    try:
        osc = po.OracleScene(po.cgltrace.load(path))
        r.configure(SIZE, SIZE, shadows=True)
        r.render()
        fb, st = r.framebuffer(), r.stats()
        c, _, _, k = po.rt_render(osc, po.rt_params(SIZE, SIZE, shadows=True))
        assert np.array_equal(fb, c), f"{int((fb != c).sum())} pixels differ"
        for key in ("primary_rays", "shadow_rays", "geometry_hits", "occluded"):
            assert st[key] == k[key], key
        # the instrumented image: the same frame, and the traversal / shading
        # counters of the oracle's walk of the renderer's tree
        r.configure(SIZE, SIZE, shadows=True, instrumented=True)
        r.render()
        assert np.array_equal(r.framebuffer(), c)
        st = r.stats()
        _, _, _, k = po.rt_render(osc, po.rt_params(SIZE, SIZE, shadows=True),
                                  bvh=s.bvh() + ((s.bvh4(),) if r.bvh4 else ()))
        for key in ("node_visits", "tri_tests", "layer_tests", "shaded", "texel_bytes", "shadow_rays",
                    "occluded"):
            assert st[key] == k[key], key
    finally:
        r.close()
        s.close()


@pytest.mark.parametrize("name", ACCEPTED)
def test_golden_scene_frame_and_counters(oracle_lib, name):
    _check(oracle_lib, scene_path(name))


@pytest.mark.parametrize("variant,fields", [("clamp", {2, 3}), ("a8l8", {4}), ("argb8888", {4, 5})])
def test_textured_scene_off_a_specialised_key_takes_the_generic_fallback(oracle_lib, tmp_path_factory,
                                                                          variant, fields):
    """A textured bilinear drawcall that differs from a specialised key only
    in its wraps (CLAMP), its format (A8L8) or its format and stride
    (A8R8G8B8) -- key fields (flags, filter, wrapu, wrapv, format, stride) at
    the indices in `fields` -- must not be shaded as that key: the oracle's
    frame of the variant differs from the base scene's, and the GPU's equals
    the variant's."""
    from synth_tex_scene import make_tex_scene
    from test_shade_keys import drawcall_key, specialised_keys
    po = oracle_lib
    path = make_tex_scene(str(tmp_path_factory.mktemp("keys") / f"box_{variant}.cgltrace.gz"), variant)
    sc = po.cgltrace.load(path)
    keys = {drawcall_key(sc, dc) for dc in sc.drawcalls}
    spec = specialised_keys()
    assert len(keys) == 1 and not (keys & spec)
    key = next(iter(keys))
    assert any({i for i in range(6) if key[i] != s[i]} == fields for s in spec), (key, spec)
    base, _, _, _ = po.rt_render(po.OracleScene(po.cgltrace.load(scene_path("box"))),
                                 po.rt_params(SIZE, SIZE, shadows=True))
    mine, _, _, _ = po.rt_render(po.OracleScene(sc), po.rt_params(SIZE, SIZE, shadows=True))
    assert int((base != mine).sum()) > 0, "the variant renders the base scene's frame: it checks nothing"
    _check(po, path)


def test_synth_scene_takes_the_generic_fallback(oracle_lib, synth_path):
    from test_shade_keys import RT_DC_TEX, drawcall_key, specialised_keys
    sc = oracle_lib.cgltrace.load(synth_path)
    keys = {drawcall_key(sc, dc) for dc in sc.drawcalls}
    assert keys and not (keys & specialised_keys()) and not any(k[0] & RT_DC_TEX for k in keys)
    _check(oracle_lib, synth_path)
