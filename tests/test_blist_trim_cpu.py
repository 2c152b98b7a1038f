"""The block lists trimmed to their winners, on the host alone (app/setup.cpp TrimBlockLists through
rt_scene_block_trim), against the oracle: per 8x8 block the entries of the oracle's
candidate list whose primitive is the raster's winner at one of the block's pixels, in order.

* every block's trimmed list, its unchanged offset and its kept count (blist_trim_cases.check_trim);
* every slot of the trimmed array, the padding entries included, names a geometry record;
* the untrimmed arrays of the same call equal the oracle's lists;
* the totals of each case as counted on the CPU when the trim was proposed;
* tekkaman 128^2 in 3 shards: every shard, and the shards' totals summed are the whole frame's."""
import numpy as np
import pytest

from blist_trim_cases import CASES, IDS, check_trim, expected
from conftest import scene_path

from skybox_rt_amd import rt  # noqa: E402


@pytest.fixture(scope="module")
def scenes(oracle_lib):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = rt.Scene.load(scene_path(name))
        return cache[name]
    yield get
    for s in cache.values():
        s.close()


@pytest.mark.parametrize("name,w,h,entries,kept,blocks,kblocks,longest", CASES, ids=IDS)
def test_host_trim_equals_oracle_winners(scenes, name, w, h, entries, kept, blocks, kblocks, longest):
    bidx, blist, btidx, btrim = scenes(name).block_trim(w, h)
    oidx, oent, _, _ = expected(name, w, h)
    assert np.array_equal(bidx, oidx) and np.array_equal(blist[:-3], oent)
    got = check_trim(btidx, btrim, name, w, h)
    print(f"{name} {w}x{h}: entries {len(oent)} -> kept {got[0]}, non-empty blocks "
          f"{int((oidx[:, 1] > 0).sum())} -> {got[1]}, longest trimmed list {got[2]}")
    assert (len(oent), int((oidx[:, 1] > 0).sum())) == (entries, blocks)
    assert got == (kept, kblocks, longest)


def test_host_trim_shards(scenes):
    name, w, h, entries, kept, blocks, kblocks, _ = CASES[1]
    tot = np.zeros(4, np.int64)
    for index in range(3):
        bidx, blist, btidx, btrim = scenes(name).block_trim(w, h, index, 3)
        oidx, oent, _, _ = expected(name, w, h, index, 3)
        assert np.array_equal(bidx, oidx) and np.array_equal(blist[:-3], oent)
        k, b, _ = check_trim(btidx, btrim, name, w, h, index, 3)
        tot += (len(oent), k, int((oidx[:, 1] > 0).sum()), b)
    assert tuple(tot) == (entries, kept, blocks, kblocks)
