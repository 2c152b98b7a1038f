"""What the block-list trim tests share (test_blist_trim_cpu.py, test_gpu_blist_trim.py): the cases,
and per case the trimmed lists as the oracle defines them -- computed once and not written to.

A block's trimmed list: the entries of the oracle's candidate list (oracle/rt.c orc_vis_block_lists)
whose primitive is the raster's depth-test winner (oracle orc_raster_render's per-pixel pid) at one of
the block's 64 pixels inside the image, in the list's order."""
import functools

import numpy as np

from conftest import scene_path

# scene, width, height, entries, kept, non-empty blocks, blocks that keep any, the longest trimmed list
CASES = [("tekkaman", 40, 24, 225, 86, 9, 9, 38),      # edge tiles overhang the image
         ("tekkaman", 128, 128, 1141, 426, 52, 51, 20),
         ("box", 128, 128, 150, 87, 80, 68, 2),
         ("scene", 128, 128, 1416, 1143, 172, 170, 30)]
IDS = [f"{c[0]}-{c[1]}x{c[2]}" for c in CASES]
PAD = np.array([0, 0xFFFFFFFF, 0xFFFEFFFE, 0xFFFFFFFF], np.uint32)


@functools.lru_cache(maxsize=None)
def oscene(name):
    from oracle import py_oracle as po
    return po.OracleScene(po.cgltrace.load(scene_path(name)))


@functools.lru_cache(maxsize=None)
def geometry(name):
    """pids of the geometry primitives, ascending: the primitives of the depth-tested drawcalls."""
    from oracle import py_oracle as po
    sc = po.cgltrace.load(scene_path(name))
    g = [np.arange(dc.prim_offset, dc.prim_offset + dc.prim_count) for dc in sc.drawcalls
         if dc.states["depth_test"]]
    out = np.concatenate(g).astype(np.int64) if g else np.zeros(0, np.int64)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _raster_pids(name, w, h):
    from oracle import py_oracle as po
    return po.raster_render(oscene(name), w, h)[2]


@functools.lru_cache(maxsize=None)
def expected(name, w, h, index=0, count=1):
    """(oidx, oent, tidx, trimmed): the oracle's lists of shard `index` of `count`, the trimmed
    headers (first, kept) and per block the kept entries (uint32[kept, 4])."""
    from oracle import py_oracle as po
    oidx, oent = po.vis_block_lists(oscene(name), w, h, index, count)
    pids, geom = _raster_pids(name, w, h), geometry(name)
    tiles_x = (w + 31) // 32
    tidx = oidx.copy()
    trimmed = []
    for lb, (first, n) in enumerate(oidx):
        gt = index + (lb >> 4) * count
        x0 = (gt % tiles_x) * 32 + (lb & 3) * 8
        y0 = (gt // tiles_x) * 32 + ((lb >> 2) & 3) * 8
        win = set(np.unique(pids[y0:min(y0 + 8, h), x0:min(x0 + 8, w)]).tolist())
        ent = oent[first:first + n]
        keep = np.array([int(geom[k]) in win for k in ent[:, 0]], bool)
        trimmed.append(ent[keep])
        tidx[lb, 1] = int(keep.sum())
    for a in (oidx, oent, tidx):
        a.setflags(write=False)
    return oidx, oent, tidx, tuple(trimmed)


def check_trim(btidx, btrim, name, w, h, index=0, count=1):
    """btidx / btrim (with the padding entries) against expected(); returns (kept, blocks, longest)."""
    oidx, oent, tidx, trimmed = expected(name, w, h, index, count)
    assert btidx.shape == tidx.shape and btrim.shape == (len(oent) + 3, 4), (btidx.shape, btrim.shape)
    assert np.array_equal(btidx[:, 0], oidx[:, 0]), "a list's offset moved"
    bad = np.nonzero(btidx[:, 1] != tidx[:, 1])[0]
    assert bad.size == 0, f"{bad.size} kept counts differ, first blocks {bad[:8]}: {btidx[bad[:8], 1]} != {tidx[bad[:8], 1]}"
    for lb, (first, n) in enumerate(tidx):
        assert np.array_equal(btrim[first:first + n], trimmed[lb]), f"block {lb}: kept entries differ"
    # every slot a scan can load -- a list's own slots behind its kept entries, the lists after it,
    # the padding entries -- names a geometry record
    assert int(btrim[:, 0].max()) < len(geometry(name))
    assert (btrim[-3:] == PAD).all()
    kept = btidx[:, 1]
    return int(kept.sum()), int((kept > 0).sum()), int(kept.max()) if len(kept) else 0
