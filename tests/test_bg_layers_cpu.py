"""CPU test of the background-layer table (rt_common.h rt_bglayer_t) as the
host restates it (app/setup.cpp BgLayers, through rt_scene_bg_layers), against
the oracle's per-pixel pid: for every 8x8-block chunk the table says which one
screen-layer primitive covers all 64 pixels (pid + 1 and its drawcall),
0xffffffff when no layer covers any, 0 otherwise.

Scenes: tekkaman, the sparse synthetic scene (no layers: every entry of a
block inside the image is 0xffffffff) and the small layered scene of
synth_bg_scene.py (blocks crossed by layer edges).  Sizes 40x24, 44x28 (blocks
overhang the image), 96x64 and 256^2.

Over the blocks that show no geometry pixel (the background; a block with a
geometry pixel never reaches the background tier, its entry is not read):
* a non-zero entry equals all 64 oracle pids, its drawcall that primitive's;
* a zero entry stands only where the 64 pids differ or a pixel lies outside
  the image -- so the table cannot hide behind zeros: the count of non-zero
  entries is the oracle's count of uniform full background blocks (tekkaman
  at 256^2: 833 of 858);
* a shuffled tile order and a first chunk behind the start give the same
  records in the order's places."""
import os

import numpy as np
import pytest

from conftest import scene_path
from skybox_rt_amd import rt

SCENES = ("tekkaman", "sparse", "layered")
SIZES = [(40, 24), (44, 28), (96, 64), (256, 256)]
NONE = 0xFFFFFFFF

_pids = {}


def scene_file(name, tmp_root):
    if name == "tekkaman":
        return scene_path(name)
    p = os.path.join(str(tmp_root), f"bg_layers_{name}.cgltrace" + (".gz" if name == "sparse" else ""))
    if not os.path.exists(p):
        if name == "sparse":
            from synth_scene import make_scene
            make_scene(p, 3, seed=5, size=0.04, spread=0.02)
        else:
            from synth_bg_scene import make_bg_scene
            make_bg_scene(p)
    return p


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bg_layers")


def oracle_pids(po, name, scene_dir, w, h):
    """(per-pixel pid int32[h, w], layer pids, drawcall of every pid), once per case, left unchanged"""
    key = (name, w, h)
    if key not in _pids:
        sc = po.cgltrace.load(scene_file(name, scene_dir))
        _, pid, _, _ = po.rt_render(po.OracleScene(sc), po.rt_params(w, h, shadows=False, nthreads=8))
        pid = np.array(pid, np.int64)
        pid.setflags(write=False)
        pdc = np.zeros(sc.num_prims, np.int64)
        layers = set()
        for d, dc in enumerate(sc.drawcalls):
            pdc[dc.prim_offset:dc.prim_offset + dc.prim_count] = d
            if not dc.states["depth_test"]:
                layers.update(range(dc.prim_offset, dc.prim_offset + dc.prim_count))
        _pids[key] = (pid, frozenset(layers), pdc)
    return _pids[key]


def expected(pid, layers, pdc, w, h, order=None, first_chunk=0):
    """per chunk from first_chunk on: (word 0, word 1) the table must hold, or None for a block
    with a geometry pixel; and the number of uniform full background blocks / of background blocks"""
    tx = (w + 31) // 32
    tiles = tx * ((h + 31) // 32)
    order = np.arange(tiles) if order is None else order
    out, uniform, background = [], 0, 0
    for c in range(first_chunk, 16 * tiles):
        t, blk = int(order[c >> 4]), c & 15
        x0, y0 = (t % tx) * 32 + (blk & 3) * 8, (t // tx) * 32 + (blk >> 2) * 8
        blkp = pid[y0:min(y0 + 8, h), x0:min(x0 + 8, w)]
        vals = set(blkp.ravel().tolist())
        if any(v >= 0 and v not in layers for v in vals):
            out.append(None)
            continue
        full = x0 + 8 <= w and y0 + 8 <= h
        background += full
        if full and len(vals) == 1:
            v = vals.pop()
            out.append((NONE, 0) if v < 0 else (v + 1, int(pdc[v])))
            uniform += 1
        else:
            out.append((0, 0))
    return out, uniform, background


def check_table(tab, exp):
    assert len(tab) == len(exp)
    nonzero = 0
    for i, (t, e) in enumerate(zip(tab.tolist(), exp)):
        if e is not None:
            assert tuple(t) == e, f"chunk {i}: table {t}, oracle {e}"
            nonzero += t[0] != 0
    return nonzero


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", SCENES)
def test_host_table_equals_the_oracle_pids(oracle_lib, scene_dir, name, w, h):
    pid, layers, pdc = oracle_pids(oracle_lib, name, scene_dir, w, h)
    s = rt.Scene.load(scene_file(name, scene_dir))
    try:
        tab = s.bg_layers(w, h)
        exp, uniform, background = expected(pid, layers, pdc, w, h)
        assert check_table(tab, exp) == uniform
        if name == "tekkaman" and (w, h) == (256, 256):
            assert (uniform, background) == (833, 858)
        if name == "sparse":
            assert not layers and all(e in (None, (NONE, 0), (0, 0)) for e in exp) and uniform > 0
        if name == "layered" and w >= 96:
            assert set(np.unique(pid[pid >= 0]).tolist()) >= {0, 1, 2}  # every layer shows,
            assert uniform < background                                 # layer edges cross blocks,
            assert {e[0] for e in exp if e} >= {0, 1, 2}                # mixed, and each of the pair alone
        # another order, a later first chunk: the same records where the order puts them
        tiles = ((w + 31) // 32) * ((h + 31) // 32)
        order = np.random.default_rng(w * h).permutation(tiles).astype(np.uint32)
        first = 16 * (tiles // 2) + 5
        tab2 = s.bg_layers(w, h, order=order, first_chunk=first)
        exp2, _, _ = expected(pid, layers, pdc, w, h, order, first)
        check_table(tab2, exp2)
        assert len(tab2) == 16 * tiles - first
    finally:
        s.close()
