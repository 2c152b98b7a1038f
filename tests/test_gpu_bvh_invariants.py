"""Both device builders -- the binned SAH of kernels/bvh_sah.hip, the tree a
renderer starts with, and the LBVH of kernels/bvh_build.hip (build_bvh()) -- on
the inputs of tests/bvh_cases.py: every size at which a builder changes its
path, duplicates, zero extents, a dynamic range of 2^12, trees at and past the
traversal stacks' depth.  For every case the exported arrays pass
tests/bvh_reference.py (what a tree means: exact containment, every triangle
once, the reported depth, node count and BVH4 stack need; for the LBVH the
Morton leaf order), equal their CPU twin's bit for bit (app/bvh.cpp;
oracle/lbvh.c), and closest-hit and any-hit queries over them answer as the
oracle's brute force does for every one of 2 048 rays.  Then rebuilds in turn
on one renderer, the deep images at a stack need of exactly 32, the fall-back
to the BVH2 above it, and the refusals past RT_STACK_DEEP."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bvh_cases as bc  # noqa: E402
import bvh_reference as br  # noqa: E402
from query_reference import bits  # noqa: E402

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402
from test_gpu_bvh_sah import _host_renderer  # noqa: E402

N = bc.N_RAYS
GUARD_RAYS = 128          # 256 words behind the hits of N rays
UNUSED = rt.RT_BVH_STACK4_UNUSED


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bvh_gpu")


def exports(r):
    nodes, tris = r.export_bvh()
    return nodes, tris, r.export_bvh4(), r.export_bvh4h()


def same_arrays(got, want, what):
    """(nodes, tris, nodes4, rt_node4h_t records) bit for bit; on a difference the first differing record"""
    for g, w, part in zip(got, want, ("nodes", "tris", "nodes4", "nodes4h")):
        assert g.shape == w.shape, (what, part, g.shape, w.shape)
        g2, w2 = np.ascontiguousarray(g).reshape(len(g), -1), np.ascontiguousarray(w).reshape(len(w), -1)
        gb, wb = (g2.view(np.uint32), w2.view(np.uint32)) if g2.dtype != np.uint8 else (g2, w2)
        bad = np.flatnonzero((gb != wb).any(1))
        assert len(bad) == 0, (what, part, len(bad), int(bad[0]), g2[bad[0]].tolist(), w2[bad[0]].tolist())


def same_hits(got, want_pid, want_t, what):
    pid, t = got
    assert pid.dtype == np.int32 and t.dtype == np.float32 and len(pid) == len(t) == len(want_pid)   # no ray left out
    bad = np.flatnonzero((pid != want_pid) | (bits(t) != bits(want_t)))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), pid[bad[:4]].tolist(), np.asarray(want_pid)[bad[:4]].tolist(),
                           t[bad[:4]].tolist(), np.asarray(want_t)[bad[:4]].tolist())


def traces(r, c, po, what):
    """closest == brute force in pid and t bits; any == the oracle's verdict with a pid the ray
    meets at the t returned; the 256 words behind the N rays' hits keep an earlier launch's"""
    rays, tri9 = c["rays"], c["tri9"]
    bp, bt, bo = c["brute"]
    fill = r.trace_rays(np.concatenate([rays[::-1], rays[:GUARD_RAYS]]), "closest")
    assert len(fill[0]) == N + GUARD_RAYS and (fill[0][N:] >= 0).any()

    def guard():
        after = r.query_hits(N + GUARD_RAYS)
        same_hits((after[0][N:], after[1][N:]), fill[0][N:], fill[1][N:], (what, "guard words"))

    same_hits(r.trace_rays(rays, "closest"), bp, bt, (what, "closest"))
    guard()
    pid, t = r.trace_rays(rays, "any")
    assert len(pid) == N and np.array_equal(pid >= 0, bo.astype(bool)), (what, "any", int(((pid >= 0) != bo.astype(bool)).sum()))
    h = np.flatnonzero(pid >= 0)
    p = pid[h]
    assert (p < len(tri9)).all()
    met, mt = po.mt(rays[h, 0:3], rays[h, 3:6], tri9[p, 0:3], tri9[p, 3:6], tri9[p, 6:9], rays[h, 6])
    assert met.all(), (what, "any names a triangle the ray misses", h[met == 0][:8].tolist())
    assert np.array_equal(bits(t[h]), bits(mt)) and (t[h] < rays[h, 7]).all() and not bits(t[pid < 0]).any()
    guard()


def open_case(name, scene_dir, po):
    """-> (case, scene, the default renderer: its device SAH tree, a small frame, N + 128 rays reserved)"""
    c = bc.case(name, scene_dir, po, rt)
    s = rt.Scene.load(c["path"])
    r = rt.Renderer(s)
    return c, s, r


def ready(r):
    r.configure(32, 32, shadows=False)
    r.query_reserve(N + GUARD_RAYS)


def check_sah(r, c, st, what):
    """the device SAH tree in `r`: valid, its stats the validator's, its arrays the host builder's"""
    nodes, tris, n4, h4, depth, stack = c["trees"]["sah"]
    got = exports(r)
    d2, d4, need = br.check_all(*got, c["corners"])
    assert st["method"] == 1
    assert (st["depth"], st["depth4"]) == (d2, d4) and st["nodes"] == br.walk2(got[0], got[1], c["corners"])["reached"] == len(got[0])
    assert st["nodes4"] == len(got[2]) and st["stack4"] == (need if need <= bc.STACK_DEEP else UNUSED)
    same_arrays(got, (nodes, tris, n4, h4), (what, "host builder"))
    assert (d2, need) == (depth, stack)
    return got


def check_lbvh(r, c, st, what):
    """the device LBVH in `r`: valid, in Morton order, its stats the validator's, its arrays the oracle's"""
    ln, lt, l4, lh, ldepth, lstack = c["trees"]["lbvh"]
    got = exports(r)
    d2, d4, need = br.check_all(*got, c["corners"], morton=True)
    assert st["method"] == 0 and st["launches"] == 19
    assert st["depth"] == d2 and st["nodes"] == st["nodes4"] == len(got[0]) == len(got[2]) == max(len(c["corners"]) - 1, 1)
    assert st["stack4"] == (need if need <= bc.STACK_DEEP else UNUSED)
    same_arrays(got, (ln, lt, l4, lh), (what, "oracle LBVH"))
    assert (d2, need) == (ldepth, lstack)
    return got


@pytest.mark.parametrize("name", bc.WITHIN)
def test_device_trees(po, scene_dir, name):
    c, s, r = open_case(name, scene_dir, po)
    st = r.bvh_stats()
    assert r.gpu_bvh and r.gpu_bvh4
    got = check_sah(r, c, st, name)
    host = _host_renderer(s)                                       # app/bvh.cpp's tree as a renderer holds it
    same_arrays(got, exports(host), (name, "host renderer"))
    host.close()
    ready(r)
    traces(r, c, po, (name, "sah"))
    if name.startswith("same"):
        assert set(np.unique(r.trace_rays(c["rays"], "closest")[0]).tolist()) <= {-1, 0}     # the lowest pid wins
    lst = r.build_bvh()
    assert r.gpu_bvh4 and r.bvh4 and r.bvh4_f16
    check_lbvh(r, c, lst, name)
    assert r.bvh_stats() == lst
    if name == bc.ladder_name(bc.LADDER_STACK32):
        assert (lst["depth"], lst["stack4"]) == (22, bc.STACK_DEEP)     # the deep images, at their stack's last entry
    traces(r, c, po, (name, "lbvh"))
    print(f"{name}: {len(c['corners'])} triangles; SAH depth {st['depth']} stack {st['stack4']} "
          f"{st['launches']} launches; LBVH depth {lst['depth']} stack {lst['stack4']}; "
          f"{int((c['brute'][0] >= 0).sum())} of {N} rays hit")
    r.close()
    s.close()


@pytest.mark.parametrize("name", ["same300", "rand1025", bc.ladder_name(bc.LADDER_STACK32), "rand3", "same4"])
def test_rebuilds_in_turn_repeat_the_arrays(po, scene_dir, name):
    """sah, lbvh, sah, lbvh on one renderer: scratch, counters and bounds start afresh each time
    (rand3, same4: the one-node trees, whose arrays hold records no phase reaches -- a rebuild gets
    them in memory the build before it has used)"""
    c, s, r = open_case(name, scene_dir, po)
    ready(r)
    for turn in range(2):
        check_sah(r, c, r.build_bvh("sah"), (name, "sah", turn))
        check_lbvh(r, c, r.build_bvh(), (name, "lbvh", turn))
    traces(r, c, po, (name, "after the rebuilds"))
    r.close()
    s.close()


def refused(fn, *a, match="", code="(-2)", **kw):
    with pytest.raises(rt.RtError) as e:
        fn(*a, **kw)
    assert code in str(e.value) and match in str(e.value), str(e.value)


def test_lbvh_stack_need_above_32_falls_back_to_the_bvh2(po, scene_dir):
    """ladder(21, 8, 8): LBVH depth 23, BVH4 stack need 33.  The build succeeds without a BVH4 in
    use, caller's rays are refused, and a primary+shadow frame -- by the lists, and with every ray
    walking the BVH2 (bvh_walk) -- is the oracle's brute-force frame.  The frame is of the case's
    in-view copy (bvh_cases.in_view), whose LBVH has the same depth and stack need."""
    name = bc.ladder_name(bc.LADDER_STACK_OVER)
    for view in (False, True):
        c = bc.view_case(name, scene_dir, po, rt) if view else bc.case(name, scene_dir, po, rt)
        assert c["trees"]["lbvh"][4] <= bc.STACK_DEEP < c["trees"]["lbvh"][5]
        s = rt.Scene.load(c["path"])
        r = rt.Renderer(s)
        check_sah(r, c, r.bvh_stats(), name)
        ready(r)
        lst = r.build_bvh()
        assert lst["stack4"] == UNUSED and not r.gpu_bvh4 and not r.bvh4
        check_lbvh(r, c, lst, name)
        refused(r.trace_rays, c["rays"], match="binary16 BVH4")
        refused(r.trace_rays, c["rays"], "any", match="binary16 BVH4")
        if view:
            light = rt.DEFAULT_LIGHT
            osc = po.OracleScene(po.cgltrace.load(c["path"]))
            want, _, _, k = po.rt_render(osc, po.rt_params(64, 64, shadows=True, light=light, nthreads=8))
            assert k["shadow_rays"] > 0 and 0 < k["occluded"] < k["shadow_rays"]
            for walk in (False, True):
                r.configure(64, 64, shadows=True, light=light, bvh_walk=walk)
                assert not r.bvh4
                r.render()
                fb, fst = r.framebuffer(), r.stats()
                assert np.array_equal(fb, want), (walk, int((fb != want).sum()))
                assert fst["shadow_rays"] == k["shadow_rays"] and fst["occluded"] == k["occluded"], (walk, fst, k)
        r.close()
        s.close()


def test_sah_stack_need_above_32_falls_back_and_host_tree_is_refused(po, scene_dir):
    """ladder(30, 2048, 1): the SAH tree is 16 deep and its BVH4 needs 33 stack entries"""
    name = bc.ladder_name(bc.LADDER_SAH_STACK)
    c, s, r = open_case(name, scene_dir, po)
    assert c["trees"]["sah"][4:] == (16, bc.STACK_DEEP + 1)
    st = r.bvh_stats()
    assert st["stack4"] == UNUSED and r.gpu_bvh and not r.gpu_bvh4
    check_sah(r, c, st, name)
    ready(r)
    assert not r.bvh4
    refused(r.trace_rays, c["rays"], match="binary16 BVH4")
    refused(_host_renderer, s, match="BVH too deep", code="(-1)")
    r.close()
    s.close()


def test_lbvh_deeper_than_32_is_refused_and_the_tree_stays(po, scene_dir):
    """ladder(30, 32, 1): the LBVH is 33 deep.  The refusal is the host's, after the build's
    launches have run (phase_emit and phase_collapse walk parent[] and keep no table of fixed
    depth): the renderer keeps its SAH tree."""
    name = bc.ladder_name(bc.LADDER_LBVH_DEEP)
    c, s, r = open_case(name, scene_dir, po)
    assert c["trees"]["lbvh"][4] == bc.STACK_DEEP + 1
    st = r.bvh_stats()
    before = check_sah(r, c, st, name)
    ready(r)
    traces(r, c, po, (name, "before"))
    refused(r.build_bvh, match="deeper than the traversal stack", code="(-1)")
    assert r.bvh_stats() == st and r.gpu_bvh4
    same_arrays(exports(r), before, (name, "after the refusal"))
    traces(r, c, po, (name, "after"))
    r.close()
    s.close()
