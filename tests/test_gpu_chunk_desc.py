"""GPU test (MI355X) of the chunk descriptor table (rt_common.h rt_cdesc_t):
the table the device setup builds (rt_setup.hip RTS_CDESC) equals the host
restatement (app/setup.cpp ChunkDescs) record for record, and the frame
rt_kernel renders through it equals the oracle's -- at 8x8 (one chunk), 40x24
(edge tiles overhang, not a multiple of 32) and 96x64 on `triangle`, and on
`tekkaman` at 128^2; with shard_count 1 and 3 (every shard_index) and the
compact buffer layout on and off; and moving the light leaves the table's
bytes as they were."""
import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

from skybox_rt_amd import rt  # noqa: E402

TILE = 32
CASES = [("triangle", 8, 8), ("triangle", 40, 24), ("triangle", 96, 64), ("tekkaman", 128, 128)]

_scenes, _oracle = {}, {}


def _renderer(name):
    if name not in _scenes:
        s = rt.Scene.load(scene_path(name))
        _scenes[name] = (s, rt.Renderer(s))
    return _scenes[name][1]


def _oracle_frame(po, name, w, h):
    """the oracle's frame, computed once per (scene, size) and left unchanged"""
    key = (name, w, h)
    if key not in _oracle:
        c, _, _, k = po.rt_render(po.OracleScene(po.cgltrace.load(scene_path(name))),
                                  po.rt_params(w, h, shadows=True))
        c.setflags(write=False)
        _oracle[key] = (c, k)
    return _oracle[key]


def _shard_pixels(fb, w, h, si, sc):
    """(y, x, colour) of a compact shard buffer's pixels that lie in the image"""
    tiles_x = (w + TILE - 1) // TILE
    tiles = fb.reshape(-1, TILE, TILE)
    ys, xs, cs = [], [], []
    for lt in range(tiles.shape[0]):
        gt = si + lt * sc
        tx, ty = gt % tiles_x, gt // tiles_x
        yy, xx = np.mgrid[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
        ok = (yy < h) & (xx < w)
        ys.append(yy[ok]); xs.append(xx[ok]); cs.append(tiles[lt][ok])
    return np.concatenate(ys), np.concatenate(xs), np.concatenate(cs)


@pytest.mark.parametrize("name,w,h", CASES)
@pytest.mark.parametrize("sc,compact", [(1, False), (1, True), (3, True)])
def test_device_table_equals_host_restatement_and_frame_equals_oracle(oracle_lib, name, w, h, sc, compact):
    r = _renderer(name)
    ref, k = _oracle_frame(oracle_lib, name, w, h)
    seen = np.zeros((h, w), bool)
    for si in range(sc):
        r.configure(w, h, shadows=True, shard_index=si, shard_count=sc, compact=compact)
        st = r.stats()
        if st["local_tiles"] == 0:  # more shards than tiles: this shard renders nothing
            continue
        dev, host = r.records("cdesc"), r.records("cdesc_host")
        assert dev.shape == host.shape == (st["local_tiles"] * 16, 4)
        assert np.array_equal(dev, host), f"{int((dev != host).any(axis=1).sum())} records differ"
        # pixel rows per record: the image width, or a tile's 32 in the compact layout
        assert np.all(dev[:, 3] >> 16 == (TILE if (compact or sc > 1) else w))
        r.render()
        fb = r.framebuffer()
        if compact or sc > 1:
            y, x, c = _shard_pixels(fb, w, h, si, sc)
            assert np.array_equal(c, ref[y, x]), f"shard {si}: {int((c != ref[y, x]).sum())} pixels differ"
            seen[y, x] = True
        else:
            assert np.array_equal(fb, ref), f"{int((fb != ref).sum())} pixels differ"
            seen[:] = True
            s2 = r.stats()
            assert s2["shadow_rays"] == k["shadow_rays"] and s2["occluded"] == k["occluded"]
    assert seen.all(), "the shards together cover the image"


@pytest.mark.parametrize("name,w,h", [("triangle", 40, 24), ("tekkaman", 128, 128)])
def test_moving_the_light_leaves_the_table_untouched(oracle_lib, name, w, h):
    po = oracle_lib
    r = _renderer(name)
    r.configure(w, h, shadows=True)
    before = r.records("cdesc").tobytes()
    light = (10.0, 40.0, 60.0)
    r.set_light(light)
    r.render()
    assert r.records("cdesc").tobytes() == before
    c, _, _, _ = po.rt_render(po.OracleScene(po.cgltrace.load(scene_path(name))),
                              po.rt_params(w, h, shadows=True, light=light))
    assert np.array_equal(r.framebuffer(), c)


def test_no_table_falls_back_to_the_task_map(oracle_lib, monkeypatch):
    """env RT_CHUNK_DESC=0: no table is built and the image works the task map
    out itself -- the same frame"""
    monkeypatch.setenv("RT_CHUNK_DESC", "0")
    r = _renderer("tekkaman")
    r.configure(128, 128, shadows=True)
    with pytest.raises(rt.RtError):
        r.records("cdesc")
    r.render()
    ref, _ = _oracle_frame(oracle_lib, "tekkaman", 128, 128)
    assert np.array_equal(r.framebuffer(), ref)
