"""Blended, stencil and masked drawcalls on the ray-tracing path: a scene
loaded with om_layers=True traces its head (the drawcalls the RT path can
trace) and folds its ordered tail over the head's pixels through the output
merger (kernels/rt_om_kernel.hip).  The frames are held, bit for bit, to the
composed checker of tests/om_scenes.py (the oracle's ray tracer / raster
pipeline for the head, its raster pipeline for the tail on top), to the
product's own raster pipeline, and through the CLI to the reference's golden
images."""
import os
import subprocess
import sys

import numpy as np
import pytest

import om_scenes as om
from conftest import GOLDEN, scene_path

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, rt  # noqa: E402

CASES = [(n, s) for n in om.SCENES for s in (32, 128)]


@pytest.mark.parametrize("name,size", CASES)
def test_plain_frame(oracle_lib, name, size):
    p = scene_path(name)
    exp, _, _ = om.composed(p, size, size, False)
    fb, _ = om.gpu_frame(p, size, size, False)
    assert int((fb != exp).sum()) == 0
    # ... and the product's raster pipeline on the same scene
    s = rt.Scene.load(p, om_layers=True)
    r = rt.Renderer(s)
    r.configure(size, size, shadows=False, raster=True)
    r.render()
    assert np.array_equal(r.framebuffer(), fb)
    r.close()


@pytest.mark.parametrize("name,size", CASES)
def test_cli_renders_on_the_rt_path(tmp_path, name, size):
    out = str(tmp_path / "o.png")
    p = subprocess.run([os.path.join(_lib.LIB_DIR, "rtapp"), "-O", "-t" + scene_path(name), f"-w{size}",
                        f"-h{size}", "-o", out, "-r" + f"{GOLDEN}/draw3d/{name}_ref_{size}.png"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "PASSED!" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    assert "rendering through the draw3d raster pipeline" not in p.stdout
    assert "Ordered tail: drawcalls %d-" % om.SPLITS[name][0] in p.stdout


@pytest.mark.parametrize("name,size", CASES)
def test_shadow_frame_and_counters(oracle_lib, name, size):
    p = scene_path(name)
    exp, _, cnt = om.composed(p, size, size, True)
    plain, _, _ = om.composed(p, size, size, False)
    fb, st = om.gpu_frame(p, size, size, True, counters=True)
    assert int((fb != exp).sum()) == 0
    gpu_plain, _ = om.gpu_frame(p, size, size, False)
    ndiff = int((exp != plain).sum())
    assert ndiff > 0 and int((fb != gpu_plain).sum()) == ndiff
    for key in ("primary_rays", "shadow_rays", "geometry_hits", "occluded"):
        assert st[key] == cnt[key], key


@pytest.mark.parametrize("shadows", (False, True))
@pytest.mark.parametrize("name", ("vase", "mouse"))
def test_same_frame_without_lists(oracle_lib, tmp_path, name, shadows):
    """RT_BLOCK_LISTS=0 RT_SHADOW_LISTS=0 (a child process): the head by the
    packet walks of the tree, the same frame."""
    p = scene_path(name)
    exp, _, _ = om.composed(p, 128, 128, shadows)
    out = str(tmp_path / "fb.npy")
    env = dict(os.environ, RT_BLOCK_LISTS="0", RT_SHADOW_LISTS="0")
    c = subprocess.run([sys.executable, om.__file__, p, "128", str(int(shadows)), out], env=env,
                       capture_output=True, text=True, timeout=120)
    assert c.returncode == 0, c.stdout[-2000:] + c.stderr[-2000:]
    assert int((np.load(out) != exp).sum()) == 0


@pytest.mark.parametrize("shadows", (False, True))
@pytest.mark.parametrize("name", ("vase", "evilskull"))
def test_same_frame_with_host_setup(oracle_lib, name, shadows):
    p = scene_path(name)
    exp, _, _ = om.composed(p, 128, 128, shadows)
    fb, _ = om.gpu_frame(p, 128, 128, shadows, host_setup=True)
    assert int((fb != exp).sum()) == 0


@pytest.mark.parametrize("shadows", (False, True))
def test_vase_200_partial_tiles(oracle_lib, shadows):
    """200 = 6 * 32 + 8: overhanging edge tiles, blocks outside the image."""
    p = scene_path("vase")
    exp, _, _ = om.composed(p, 200, 200, shadows)
    fb, _ = om.gpu_frame(p, 200, 200, shadows)
    assert int((fb != exp).sum()) == 0


def test_two_shards(oracle_lib):
    p = scene_path("evilskull")
    whole, _ = om.gpu_frame(p, 128, 128, True)
    s = rt.Scene.load(p, om_layers=True)
    r = rt.Renderer(s)
    shards = []
    for i in range(2):
        r.configure(128, 128, shadows=True, shard_index=i, shard_count=2, counters=False)
        r.render()
        shards.append(r.framebuffer().copy())
    r.close()
    assert np.array_equal(rt.deinterleave_tiles(shards, 128, 128), whole)
    assert np.array_equal(whole, om.composed(p, 128, 128, True)[0])


def test_exported_tail_lists_are_the_host_builder_s(oracle_lib):
    p = scene_path("vase")
    s = rt.Scene.load(p, om_layers=True)
    r = rt.Renderer(s)
    r.configure(128, 128, shadows=False)
    idx, ent = s.setup_olists(128, 128)
    assert np.array_equal(r.records("oidx"), idx)
    assert np.array_equal(r.records("olist")[:len(ent), 0], ent)
    r.close()


@pytest.fixture(scope="module")
def vase_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("om_vase_gpu")


@pytest.mark.parametrize("shadows", (False, True))
@pytest.mark.parametrize("which", ("mask", "stencil", "blend", "all"))
def test_synthetic_states(oracle_lib, vase_dir, which, shadows):
    """A partial colour mask, a stencil test some fragments pass and some
    fail, non-alpha blend factors: states no golden scene has."""
    p = om.mutated_vase(vase_dir, which)
    exp, _, _ = om.composed(p, 64, 64, shadows)
    fb, _ = om.gpu_frame(p, 64, 64, shadows)
    assert int((fb != exp).sum()) == 0


@pytest.mark.parametrize("kw", ({"path": True}, {"flat": True}, {"bvh_walk": True}, {"instrumented": True},
                                {"bvh_width": 2}), ids=("path", "flat", "bvh_walk", "instrumented", "bvh2"))
def test_rejected_modes(kw):
    """Modes without an output-merger image, and a head whose tree is not the
    binary16 BVH4 (the generic deep images' case), are refused with -2."""
    s = rt.Scene.load(scene_path("vase"), om_layers=True)
    r = rt.Renderer(s)
    with pytest.raises(rt.RtError, match=r"\(-2\).*RT_RENDER_RASTER"):
        r.configure(64, 64, shadows=False, **kw)
    r.configure(64, 64, shadows=False)      # the renderer is still usable
    r.close()


def test_without_the_flag_the_rt_path_still_refuses():
    s = rt.Scene.load(scene_path("vase"))
    r = rt.Renderer(s)
    with pytest.raises(rt.RtError, match=r"\(-2\).*RT_RENDER_RASTER"):
        r.configure(64, 64, shadows=False)
    r.close()
