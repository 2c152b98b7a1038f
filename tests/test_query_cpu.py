"""Ray queries without a GPU: the record sizes of include/vx_rt.h, the host's
rt_query_key against the numpy restatement of its definition (tests/
query_reference.py) on the walk scenes' rays and on a hand-worked table, and the
Python layer's argument checks, which come before any call into the library."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_reference as qr  # noqa: E402
import ray_known_answers as ka  # noqa: E402

from skybox_rt_amd import rt  # noqa: E402


def test_record_sizes():
    class Ray(ctypes.Structure):
        _fields_ = [("o", ctypes.c_float * 3), ("tmin", ctypes.c_float), ("d", ctypes.c_float * 3),
                    ("tmax", ctypes.c_float)]

    class Hit(ctypes.Structure):
        _fields_ = [("pid", ctypes.c_int32), ("t", ctypes.c_float)]

    assert ctypes.sizeof(Ray) == 32 and ctypes.sizeof(Hit) == 8
    assert rt.RAY_DTYPE.itemsize == 32 and rt.HIT_DTYPE.itemsize == 8
    assert [rt.RAY_DTYPE.fields[n][1] for n in ("o", "tmin", "d", "tmax")] == [0, 12, 16, 28]
    assert [rt.HIT_DTYPE.fields[n][1] for n in ("pid", "t")] == [0, 4]
    # the library reads a ray as that record: o, tmin, d, tmax -- a direction along -x shows its sign bit,
    # an origin of -1 does not
    rec = np.zeros(1, rt.RAY_DTYPE)
    rec["o"], rec["d"], rec["tmax"] = (-1, 0, 0), (-1, 0, 0), 1.0
    h = rt.lib()
    box = (ctypes.c_float * 6)(0, 0, 0, 128, 128, 128)
    assert h.rt_query_key(rec.ctypes.data, box) == 0x8000000F


def test_hand_worked_keys():
    rays, boxes, keys = qr.hand_rays()
    assert len(rays) >= 12
    for i, (r, b, k) in enumerate(zip(rays, boxes, keys)):
        got = rt.query_key(r, b)
        model = int(qr.key_numpy(r[None], b)[0])
        assert got == int(k) and model == int(k), (i, r.tolist(), b.tolist(), hex(got), hex(model), hex(int(k)))
    assert list(qr.malformed(rays)) == [int(k) == qr.MISS_KEY for k in keys]


@pytest.fixture(scope="module")
def scene_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("query_cpu")


@pytest.mark.parametrize("name", ka.WALK_SCENES)
def test_key_equals_numpy_on_walk_rays(oracle_lib, scene_dir, name):
    case = ka.walk_case(name, scene_dir, oracle_lib, rt)
    rays = case["rays"]
    assert rays.shape == (4096, 8)
    t9 = case["tri9"]
    corners = np.stack([t9[:, 0:3], t9[:, 0:3] + t9[:, 3:6], t9[:, 0:3] + t9[:, 6:9]], 1)
    for box in (qr.corner_box(corners), np.array(qr.U, np.float32)):
        got = rt.query_key(rays, box)
        want = qr.key_numpy(rays, box)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (name, len(bad), rays[bad[0]].tolist(), hex(int(got[bad[0]])), hex(int(want[bad[0]])))
        print(f"{name}: {len(np.unique(got))} distinct keys over {len(rays)} rays")
        assert len(np.unique(got)) > 64   # the key separates unrelated rays


def test_python_layer_rejects_before_any_device_call(monkeypatch):
    def no_lib():
        raise AssertionError("the library was called")

    monkeypatch.setattr(rt, "lib", no_lib)
    r = object.__new__(rt.Renderer)
    r._h = None
    r._query_keep = []
    ok = np.zeros((4, 8), np.float32)
    ok[:, 3] = 1.0
    bad_rays = [np.zeros((4, 7), np.float32), np.zeros((8,), np.float32), np.zeros((4, 8), np.float64),
                np.zeros((0, 8), np.float32), np.zeros((2, 4, 8), np.float32), [[0.0] * 8]]
    for rays in bad_rays:
        with pytest.raises(rt.RtError, match="rays are"):
            r.trace_rays(rays)
        with pytest.raises(rt.RtError, match="rays are"):
            r.query_keys(rays)
    for mode in ("nearest", "", None, 0):
        with pytest.raises(rt.RtError, match="mode is one of"):
            r.trace_rays(ok, mode=mode)
    for skip in (np.zeros(4, np.int64), np.zeros(3, np.int32), np.zeros((4, 1), np.int32), [0, 0, 0, 0]):
        with pytest.raises(rt.RtError, match="skip is"):
            r.trace_rays(ok, skip=skip)
    with pytest.raises(rt.RtError, match="8 floats"):
        rt.query_key(np.zeros(7, np.float32), qr.U)
    r._h = None
