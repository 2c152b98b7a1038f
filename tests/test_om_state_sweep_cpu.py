"""The layered synthetic scene of the output-merger state sweeps
(tests/synth_scene.py make_layer_scene, tests/om_scenes.py LAYER_FAMILIES)
must tell the swept states apart before the GPU test
(test_gpu_om_state_sweep.py) can mean anything: within every family the
composed oracle frames -- colour and depth/stencil -- are pairwise distinct.
The golden scenes do not manage that: they have no depth ties and nothing
fails their stencil tests."""
import itertools

import numpy as np
import pytest

import om_scenes as om

SIZE = 32


@pytest.fixture(scope="module")
def layer_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("om_layers_cpu")


def _frames(directory, family):
    values = list(om.LAYER_FAMILIES[family][0])
    return values, [om.composed(om.layer_scene(directory, family, v), SIZE, SIZE, False)[:2]
                    for v in values]


def test_scene_shape(oracle_lib, layer_dir):
    """the head is drawcall 0 alone; the counting drawcall leaves 0 to 3+
    layers behind (stencil 0xff down to 0xfc or lower); the tail meets depth
    ties, nearer and farther fragments"""
    p = om.layer_scene(layer_dir, "depth_func", 3)
    full = om.load_full(p)
    assert len(full.drawcalls) == 4 and om.first_tail_drawcall(full) == 1
    # count overdraw of the counting drawcall with depth ALWAYS: every fragment decrements
    from synth_scene import make_layer_scene
    q = make_layer_scene(str(layer_dir / "count.cgltrace"),
                         [dict(om.LAYER_COUNTING, depth_func=7), dict(depth_test=1, depth_func=0),
                          dict(depth_test=1, depth_func=0)])
    _, ds, _ = om.composed(q, 64, 64, False)
    layers = 0xFF - (ds >> 24)
    assert layers.min() == 0 and layers.max() >= 3
    # EQUAL, LESS and GREATER each pass somewhere and fail somewhere
    # (in the colour plane: an EQUAL pass writes the depth that is there)
    never = om.composed(om.layer_scene(layer_dir, "depth_func", 0), SIZE, SIZE, False)[0]
    always = om.composed(om.layer_scene(layer_dir, "depth_func", 7), SIZE, SIZE, False)[0]
    for f in (1, 2, 4):
        d = om.composed(om.layer_scene(layer_dir, "depth_func", f), SIZE, SIZE, False)[0]
        assert (d != never).any() and (d != always).any(), f


@pytest.mark.parametrize("family", list(om.LAYER_FAMILIES))
def test_family_frames_are_pairwise_distinct(oracle_lib, layer_dir, family):
    values, frames = _frames(layer_dir, family)
    same = [(values[i], values[j]) for (i, a), (j, b) in itertools.combinations(enumerate(frames), 2)
            if np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])]
    assert same == []       # no indistinguishable pair in any family
    # the colour plane alone (all the om_layers path exposes) separates them too,
    # but for fail ops KEEP and ZERO: they differ where the EQUAL 0xfe test failed,
    # on 0xff / 0xfd against 0x00, and the read-back drawcall rejects all three
    same_colour = [(values[i], values[j])
                   for (i, a), (j, b) in itertools.combinations(enumerate(frames), 2)
                   if np.array_equal(a[0], b[0])]
    assert same_colour == ([(0, 4)] if family == "fail_op" else [])


@pytest.mark.parametrize("tag,drawcall,values", om.VASE_SWEEPS, ids=[s[0] for s in om.VASE_SWEEPS])
def test_vase_sweeps_are_pairwise_distinct(oracle_lib, layer_dir, tag, drawcall, values):
    frames = [om.composed(om.swept_vase(layer_dir, tag, drawcall, v), 64, 64, False)[0] for v in values]
    for (i, a), (j, b) in itertools.combinations(enumerate(frames), 2):
        assert not np.array_equal(a, b), (i, j)


def test_product_reads_the_layered_scene_as_the_oracle_does(oracle_lib, layer_dir):
    from skybox_rt_amd import rt
    p = om.layer_scene(layer_dir, "stencil_func", 5)
    ref = om.load_full(p)
    s = rt.Scene.load(p, om_layers=True)
    try:
        assert np.array_equal(s.prims().view(np.uint32), ref.prim_verts.view(np.uint32))
        assert s.info()["num_drawcalls"] == 4
        first, tail_prims = s.om_split()[:2]
        assert (first, tail_prims) == (1, ref.num_prims - ref.drawcalls[0].prim_count)
    finally:
        s.close()
