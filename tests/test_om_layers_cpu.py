"""The ordered tail on the CPU (no GPU): the scene split of
rt.Scene.load(om_layers=True), the composed checker the GPU tests hold the
frames to (tests/om_scenes.py) against the oracle's raster pipeline and the
reference's golden images, the host-built per-block tail lists, and the
synthetic-state variants of vase."""
import numpy as np
import pytest
from PIL import Image

import om_scenes as om
from conftest import GOLDEN, scene_path

from skybox_rt_amd import rt


# ---- split -------------------------------------------------------------------
@pytest.mark.parametrize("name", om.SCENES)
def test_split_of_the_tailed_scenes(oracle_lib, name):
    s = rt.Scene.load(scene_path(name), om_layers=True)
    assert s.om_split() == om.SPLITS[name]
    full = om.load_full(scene_path(name))
    k = om.first_tail_drawcall(full)
    assert k == om.SPLITS[name][0]                      # the rule restated in Python
    assert sum(dc.prim_count for dc in full.drawcalls[k:]) == om.SPLITS[name][1]
    # geometry / layers describe the head only
    info = s.info()
    head = full.drawcalls[:k]
    assert info["num_geometry"] == sum(dc.prim_count for dc in head if dc.states["depth_test"])
    assert info["num_layer"] == sum(dc.prim_count for dc in head if not dc.states["depth_test"])
    assert info["num_prims"] == full.num_prims and info["num_drawcalls"] == len(full.drawcalls)


@pytest.mark.parametrize("name", ("tekkaman", "box"))
def test_scenes_without_a_tail_load_the_same_either_way(name):
    a, b = rt.Scene.load(scene_path(name), om_layers=True), rt.Scene.load(scene_path(name))
    n = a.info()["num_drawcalls"]
    assert a.om_split() == (n, 0) and b.om_split() == (n, 0)
    ia, ib = a.info(), b.info()
    for key in ("num_geometry", "num_layer", "bvh_nodes", "bvh_tris", "bvh4_nodes", "bvh4_stack"):
        assert ia[key] == ib[key], key
    idx, ent = a.setup_olists(64, 64)
    assert len(ent) == 0 and not idx[:, 1].any()


def test_loading_without_the_flag_is_unchanged():
    """vase without om_layers: every depth-tested primitive is geometry and the
    tree is built over all of them (the figures from before the flag existed), no tail."""
    s = rt.Scene.load(scene_path("vase"))
    info = s.info()
    assert (info["num_geometry"], info["bvh_nodes"], info["num_layer"]) == (1579, 480, 64)
    assert s.om_split() == (6, 0)


# ---- the checker ---------------------------------------------------------------
@pytest.mark.parametrize("name", om.SCENES)
def test_checker_without_shadows_is_the_raster_frame(oracle_lib, name):
    p = scene_path(name)
    c, d, _ = om.composed(p, 32, 32, False)
    rc, rd = om.raster_full(p, 32, 32)
    assert np.array_equal(c, rc) and np.array_equal(d, rd)


@pytest.mark.parametrize("size", (32, 128))
@pytest.mark.parametrize("name", om.SCENES)
def test_checker_without_shadows_is_the_golden_image(oracle_lib, name, size):
    """Exact, as test_oracle_goldens.py holds the raster oracle to every one of
    these images (mouse at 128^2 included: the composition bins at 32x32)."""
    po = oracle_lib
    c, _, _ = om.composed(scene_path(name), size, size, False)
    ref = np.array(Image.open(f"{GOLDEN}/draw3d/{name}_ref_{size}.png").convert("RGBA"))
    assert po.compare_images(po.argb_to_rgba_image(c), ref, tol=0) == 0


# pixels the tail changes / pixels of the head the shadows change, default light (CPU oracle)
TABLE = {("vase", 32): (152, 1), ("vase", 128): (2503, 22), ("mouse", 32): (18, 13),
         ("mouse", 128): (298, 200), ("evilskull", 32): (373, 24), ("evilskull", 128): (6033, 421),
         ("polybump", 32): (35, 10), ("polybump", 128): (564, 178)}


@pytest.mark.parametrize("name,size", sorted(TABLE))
def test_checker_exercises_tail_and_shadows(oracle_lib, name, size):
    po = oracle_lib
    p = scene_path(name)
    full = om.load_full(p)
    head = po.OracleScene(po.cgltrace.select_drawcalls(full, range(om.first_tail_drawcall(full))))
    plain, _, _ = om.composed(p, size, size, False)
    shadow, _, cnt = om.composed(p, size, size, True)
    head_only, _, _ = po.raster_render(head, size, size)
    head_shadow = po.rt_render(head, po.rt_params(size, size, shadows=True))[0]
    # the table counts the shadows' pixels on the head, before the fold (an
    # opaque tail fragment may cover some of them)
    assert (int((plain != head_only).sum()), int((head_shadow != head_only).sum())) == TABLE[(name, size)]
    assert 0 < int((shadow != plain).sum()) <= TABLE[(name, size)][1]
    assert cnt["shadow_rays"] > 0 and cnt["occluded"] > 0


# ---- the per-block lists ---------------------------------------------------------
@pytest.mark.parametrize("size", (32, 128))
@pytest.mark.parametrize("name", ("vase", "evilskull"))
def test_tail_lists(oracle_lib, name, size):
    po = oracle_lib
    p = scene_path(name)
    s = rt.Scene.load(p, om_layers=True)
    idx, ent = s.setup_olists(size, size)
    full = om.load_full(p)
    osc = po.OracleScene(full)
    k = om.first_tail_drawcall(full)
    first = full.drawcalls[k].prim_offset
    tail = np.arange(first, full.num_prims)
    assert len(tail) == om.SPLITS[name][1]
    vis = po.vis_prims(osc, size, size)            # the oracle's covered-pixel rectangles
    prims = s.setup_prims(size, size)              # edge functions (words 0-8)
    tiles_x = (size + 31) // 32
    nblk = tiles_x * ((size + 31) // 32) * 16
    assert idx.shape == (nblk, 2) and int(idx[:, 1].sum()) == len(ent)
    # per block: the pids whose rectangle reaches it / that cover a pixel of it
    reach = [set() for _ in range(nblk)]
    cover = [set() for _ in range(nblk)]
    for g in tail:
        rx, ry = int(vis[g, 0]), int(vis[g, 1])
        x0, x1, y0, y1 = rx & 0xFFFF, rx >> 16, ry & 0xFFFF, ry >> 16
        if x0 > x1 or y0 > y1:
            continue
        m = po.edge_cover(prims[g, :9], x0, y0, x1 - x0 + 1, y1 - y0 + 1)
        for by in range(y0 >> 3, (y1 >> 3) + 1):
            for bx in range(x0 >> 3, (x1 >> 3) + 1):
                b = ((by >> 2) * tiles_x + (bx >> 2)) * 16 + (by & 3) * 4 + (bx & 3)
                reach[b].add(int(g))
                sub = m[max(by * 8, y0) - y0:min(by * 8 + 7, y1) - y0 + 1,
                        max(bx * 8, x0) - x0:min(bx * 8 + 7, x1) - x0 + 1]
                if sub.any():
                    cover[b].add(int(g))
    assert any(cover)
    for b in range(nblk):
        l = ent[idx[b, 0]:idx[b, 0] + idx[b, 1]].astype(np.int64)
        assert np.all(np.diff(l) > 0), b                       # strictly ascending
        assert np.all((l >= first) & (l < full.num_prims)), b  # tail primitives only
        assert cover[b] <= set(l.tolist()) <= reach[b], b


# ---- synthetic states --------------------------------------------------------------
@pytest.fixture(scope="module")
def vase_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("om_vase")


@pytest.mark.parametrize("which", ("mask", "stencil", "blend", "all"))
def test_mutated_vase_loads_and_changes_the_frame(oracle_lib, vase_dir, which):
    p = om.mutated_vase(vase_dir, which)
    s = rt.Scene.load(p, om_layers=True)
    assert s.om_split() == om.SPLITS["vase"]        # the tail starts where it did
    base, _ = om.raster_full(scene_path("vase"), 64, 64)
    c, d = om.raster_full(p, 64, 64)
    assert int((c != base).sum()) > 0
    # the composition is the raster frame for these states too
    cc, cd, _ = om.composed(p, 64, 64, False)
    assert np.array_equal(cc, c) and np.array_equal(cd, d)
    if which in ("stencil", "all"):
        st = d >> 24
        assert st.min() != st.max()                 # some fragments passed (zeroed), some pixels untouched
