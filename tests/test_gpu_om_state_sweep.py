"""Scene-level sweep of the output-merger states the host translates from the
trace (app/setup.cpp ToVXCompare / ToVXStencilOp / ToVXBlend -> rt_omstate_t):
every compare function as depth and as stencil function, every stencil
operation as pass and as fail operation, every blend factor as source and as
destination, every colour mask -- on the layered synthetic scene whose frames
tell them apart (test_om_state_sweep_cpu.py), through the raster pipeline
(raster_kernel) and through the ordered tail of the RT path (rt_om), plain
and with shadows.  Each frame equals the composed oracle frame bit for bit;
the raster pipeline's depth/stencil plane too.  vase's blend and colour-mask
sweeps are the real-scene leg."""
import numpy as np
import pytest

import om_scenes as om

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402


@pytest.fixture(scope="module")
def sweep_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("om_sweep_gpu")


def _check(path, size):
    exp_c, exp_ds, _ = om.composed(path, size, size, False)
    exp_shadow, _, _ = om.composed(path, size, size, True)
    s = rt.Scene.load(path, om_layers=True)
    try:
        for kw, exp, what in ((dict(shadows=False, raster=True), exp_c, "raster"),
                              (dict(shadows=False), exp_c, "ordered tail, plain"),
                              (dict(shadows=True), exp_shadow, "ordered tail, shadows")):
            r = rt.Renderer(s)
            try:
                r.configure(size, size, **kw)
                r.render()
                assert int((r.framebuffer() != exp).sum()) == 0, what
                if kw.get("raster"):
                    assert int((r.depthbuffer() != exp_ds).sum()) == 0, what + " depth/stencil"
            finally:
                r.close()
    finally:
        s.close()


@pytest.mark.parametrize("family,value", om.LAYER_CASES, ids=[f"{f}-{v}" for f, v in om.LAYER_CASES])
def test_layer_scene_state(oracle_lib, sweep_dir, family, value):
    _check(om.layer_scene(sweep_dir, family, value), 32)


@pytest.mark.parametrize("tag,drawcall,value", om.VASE_CASES,
                         ids=[f"{t}@{d}-{v}" for t, d, v in om.VASE_CASES])
def test_vase_state(oracle_lib, sweep_dir, tag, drawcall, value):
    _check(om.swept_vase(sweep_dir, tag, drawcall, value), 64)
