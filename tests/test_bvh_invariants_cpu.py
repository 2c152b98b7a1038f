"""The host SAH builder (app/bvh.cpp) and the oracle's LBVH (oracle/lbvh.c) held
to what a tree means (tests/bvh_reference.py) on the inputs of tests/bvh_cases.py:
sizes at every threshold of the device builders, duplicates, zero extents, a
dynamic range of 2^12, and trees as deep as the traversal stacks allow and
deeper.  Both are the twins the device builders are compared with bit for bit
(tests/test_gpu_bvh_invariants.py); here each is valid by itself, the LBVH's
leaf order is the Morton order, and the oracle's BVH2 and BVH4 walks over both
trees return brute force's answers for every ray."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("SKYBOX_RT_NO_TORCH", "1")

import bvh_cases as bc  # noqa: E402
import bvh_reference as br  # noqa: E402
from query_reference import bits  # noqa: E402

from skybox_rt_amd import _lib, rt  # noqa: E402

N = bc.N_RAYS


@pytest.fixture(scope="session", autouse=True)
def native_built():
    if _lib.missing():
        _lib.build()
    assert not _lib.missing()


@pytest.fixture(scope="module")
def po(oracle_lib):
    return oracle_lib


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bvh_cases")


def same(got, want, what):
    """(pid, t, occluded) of every ray equal, t bit for bit"""
    for g, w, field in zip(got, want, ("pid", "t", "occluded")):
        assert len(g) == len(w) == len(want[0])                           # no ray is left out
        bad = np.flatnonzero(bits(g) != bits(w)) if field == "t" else np.flatnonzero(np.asarray(g) != np.asarray(w))
        assert len(bad) == 0, (what, field, len(bad), bad[:8].tolist())


@pytest.mark.parametrize("name", bc.NAMES)
def test_trees_are_valid_and_walks_equal_brute_force(po, scene_dir, name):
    c = bc.case(name, scene_dir, po, rt)
    corners, info = c["corners"], c["info"]
    bp, bt, bo = c["brute"]
    hits = int((bp >= 0).sum())
    print(f"{name}: {len(corners)} triangles, {hits} of {N} rays hit")
    assert hits >= N // 8 and N - hits >= N // 16
    for kind in ("sah", "lbvh"):
        nodes, tris, n4, h4, depth, stack = c["trees"][kind]
        d2, d4, st = br.check_all(nodes, tris, n4, h4, corners, depth=depth, stack4=stack, morton=kind == "lbvh")
        print(f"  {kind}: depth {d2}, BVH4 depth {d4}, stack need {st}")
        if kind == "sah":
            assert d4 == info["bvh4_depth"] and br.walk2(nodes, tris, corners)["reached"] == info["bvh_nodes"] == len(nodes)
            assert len(n4) == info["bvh4_nodes"]
        else:
            assert len(nodes) == len(n4) == max(len(corners) - 1, 1)
        zero = np.zeros(N, np.uint8)
        same(po.trace_rays(c["tri9"], c["rays"], c["none"], zero, bvh=(nodes, tris), mode=1), (bp, bt, bo), (name, kind, "BVH2"))
        same(po.trace_rays(c["tri9"], c["rays"], c["none"], zero, bvh=(nodes, tris, n4), mode=2), (bp, bt, bo), (name, kind, "BVH4"))


def test_duplicates_answer_the_lowest_pid(po, scene_dir):
    c = bc.case("same300", scene_dir, po, rt)
    bp = c["brute"][0]
    assert set(np.unique(bp).tolist()) == {-1, 0}


@pytest.mark.parametrize("spec", sorted(bc.LADDER_FACTS))
def test_depth_cases_reach_their_depths(po, scene_dir, spec):
    c = bc.case(bc.ladder_name(spec), scene_dir, po, rt)
    sah, lbvh = c["trees"]["sah"], c["trees"]["lbvh"]
    assert (c["info"]["bvh_depth"], c["info"]["bvh4_stack"], lbvh[4], lbvh[5]) == bc.LADDER_FACTS[spec]
    assert (sah[4], sah[5]) == bc.LADDER_FACTS[spec][:2]


def test_depth_cases_sit_at_the_limits(po, scene_dir):
    """the properties the GPU tests rely on, from the host builder and the oracle alone"""
    deep = bc.STACK_DEEP
    t = {s: bc.case(bc.ladder_name(s), scene_dir, po, rt)["trees"] for s in bc.LADDERS}
    assert t[bc.LADDER_STACK32]["lbvh"][4:] == (22, 32)                       # loads the deep images at exactly 32
    bits_, cc, m = bc.LADDER_STACK_OVER
    over, below = t[bc.LADDER_STACK_OVER]["lbvh"], bc.case(bc.ladder_name((bits_ - 1, cc, m)), scene_dir, po, rt)["trees"]["lbvh"]
    assert over[4] <= deep < over[5] and below[5] <= deep                     # the smallest such `bits`
    assert max(t[bc.LADDER_STACK_OVER]["sah"][4:]) <= deep
    assert t[bc.LADDER_LBVH_DEEP]["lbvh"][4] == deep + 1 and max(t[bc.LADDER_LBVH_DEEP]["sah"][4:]) <= deep
    assert t[bc.LADDER_SAH_STACK]["sah"][4] <= deep and t[bc.LADDER_SAH_STACK]["sah"][5] == deep + 1
    for name in bc.WITHIN:
        tr = bc.case(name, scene_dir, po, rt)["trees"]
        assert max(tr["sah"][4:] + tr["lbvh"][4:]) <= deep, name


def test_in_view_copy_keeps_the_tree_and_casts_shadow_rays(po, scene_dir):
    """the frame of the case whose LBVH needs more than 32 stack entries: its in-view copy has the
    same LBVH shape, and the oracle's brute-force frame at 64 x 64 has shadow rays, some occluded"""
    name = bc.ladder_name(bc.LADDER_STACK_OVER)
    c, v = bc.case(name, scene_dir, po, rt), bc.view_case(name, scene_dir, po, rt)
    assert v["trees"]["lbvh"][4:] == c["trees"]["lbvh"][4:] and max(v["trees"]["sah"][4:]) <= bc.STACK_DEEP
    assert np.array_equal(v["trees"]["lbvh"][1][:, 3].view(np.int32), c["trees"]["lbvh"][1][:, 3].view(np.int32))
    for kind in ("sah", "lbvh"):
        nodes, tris, n4, h4, depth, stack = v["trees"][kind]
        br.check_all(nodes, tris, n4, h4, v["corners"], depth=depth, stack4=stack, morton=kind == "lbvh")
    osc = po.OracleScene(po.cgltrace.load(v["path"]))
    _, _, _, k = po.rt_render(osc, po.rt_params(64, 64, shadows=True, nthreads=8))
    print(f"{name} in view: {k['shadow_rays']} shadow rays, {k['occluded']} occluded")
    assert k["shadow_rays"] > 0 and 0 < k["occluded"] < k["shadow_rays"]
    ln, lt = v["trees"]["lbvh"][:2]
    _, _, _, k2 = po.rt_render(osc, po.rt_params(64, 64, shadows=True, nthreads=8, vis_lists=False, shadow_lists=False),
                               bvh=(ln, lt))
    assert (k2["shadow_rays"], k2["occluded"]) == (k["shadow_rays"], k["occluded"])


def test_lattice_case_equals_the_exact_model(po, scene_dir):
    c = bc.case("lat1025", scene_dir, po, rt)
    rays, skip, mp, mt, mo = bc.lattice_table(c)
    n = len(rays)
    zero = np.zeros(n, np.uint8)
    want = (mp, mt, mo.astype(np.uint8))
    same(po.trace_rays(c["tri9"], rays, skip, zero), want, "brute force")
    for kind in ("sah", "lbvh"):
        nodes, tris, n4 = c["trees"][kind][:3]
        same(po.trace_rays(c["tri9"], rays, skip, zero, bvh=(nodes, tris), mode=1), want, (kind, "BVH2"))
        same(po.trace_rays(c["tri9"], rays, skip, zero, bvh=(nodes, tris, n4), mode=2), want, (kind, "BVH4"))
    print(f"lat1025, lattice rays: {int((mp >= 0).sum())} of {n} hit")
    assert (mp >= 0).sum() >= n // 8 and (mp < 0).sum() >= n // 16


@pytest.mark.parametrize("name", ["rand1025", "rand2049", "lat1025"])
def test_sah_tree_costs_no_more_than_the_median_tree(po, scene_dir, name):
    """Measured: 0.794 (rand1025), 0.792 (rand2049), 0.881 (lat1025) of the median tree's cost."""
    c = bc.case(name, scene_dir, po, rt)
    mn, mt = br.median_tree(c["corners"])
    assert br.check_bvh2(mn, mt, c["corners"]) >= 1
    sah, med = br.sah_cost(c["trees"]["sah"][0]), br.sah_cost(mn)
    print(f"{name}: SAH cost {sah:.3f}, median tree {med:.3f}, ratio {sah / med:.4f}")
    assert sah <= med


def test_validator_rejects_every_mutation():
    done = br.check_sensitivity()
    for what in ("leaf plane one ulp inward", "BVH4 plane one binary16 quantum inward", "triangle dropped",
                 "leaf referenced twice", "records swapped across leaves", "stack bound one too high",
                 "stack bound one too low", "no binary16 value", "equal-code triangles swapped"):
        assert any(what in d for d in done), what


def test_morton_order_is_stable_and_clamped():
    """the rule by hand: centres 0 and 1023 fix the range; centre k lands in cell k (k / 1023 *
    1024 = k + k / 1023 < k + 1), the top centre is clamped from 1024 to 1023; x is the highest
    bit of a triple; equal codes keep index order"""
    pos = np.array([[0, 0, 0], [1023, 1023, 1023], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1], [512, 0, 0]], np.float64)
    corners = (pos[:, None, :] + bc._CELL[None]).astype(np.float32)
    assert br.morton_codes(corners).tolist() == [0, (1 << 30) - 1, 4, 2, 1, 1, 4 << 27]
    assert br.morton_order(corners).tolist() == [0, 4, 5, 3, 2, 6, 1]
    flat = corners.copy()
    flat[:, :, 1] = 7.0                                                   # zero extent on y: its bits are 0
    assert br.morton_codes(flat).tolist() == [0, ((1 << 30) - 1) & ~0x12492492, 4, 0, 1, 1, 4 << 27]
