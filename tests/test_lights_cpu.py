"""Several lights (vx_rt.h rt_renderer_set_lights): the exported entry points
and the host restatement of the device resolve, rt_lights_resolve -- the same
text the kernel compiles (kernels/rt_common.h rt_lights_mix: a multiplication
by a reciprocal in place of the division) -- against a numpy restatement of
the definition, over its whole domain.  No GPU."""
import ctypes as C
import os

import numpy as np

from skybox_rt_amd import _lib


def _h():
    h = C.CDLL(os.path.join(_lib.LIB_DIR, "librtapp.so"))
    h.rt_lights_resolve.argtypes = [C.c_uint32] * 3
    h.rt_lights_resolve.restype = C.c_uint32
    h.rt_accum_resolve.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
    h.rt_accum_resolve.restype = C.c_uint32
    return h


def test_entry_points_exported():
    h = C.CDLL(os.path.join(_lib.LIB_DIR, "librtapp.so"))
    for name in ("rt_renderer_set_lights", "rt_renderer_lights_info", "rt_renderer_export_light_lists",
                 "rt_lights_resolve"):
        assert hasattr(h, name), name
    for img in ("rt_lights.vxbin", "rt_lights_stats.vxbin"):
        assert img in _lib.REQUIRED


def test_resolve_equals_the_definition_everywhere():
    """Every c in 0..255, k in 1..16, o in 0..k, in each channel (the other two
    held at values of their own), under four alphas: (2 * sum + k) // (2 * k)
    with sum = (k - o) * c + o * (c >> 1), and rt_accum_resolve on the sums."""
    h = _h()
    c = np.arange(256, dtype=np.uint64)
    for k in range(1, 17):
        for o in range(k + 1):
            want = (2 * ((k - o) * c + o * (c >> np.uint64(1))) + k) // (2 * k)
            for alpha in (0x00, 0x01, 0x80, 0xFF):
                for sh in (16, 8, 0):
                    others = {16: (8, 0), 8: (16, 0), 0: (16, 8)}[sh]
                    for v in range(256):
                        # the other channels: v's complement and a fixed odd value
                        a, b = 255 - v, 0x5B
                        argb = (alpha << 24) | (v << sh) | (a << others[0]) | (b << others[1])
                        got = h.rt_lights_resolve(argb, o, k)
                        assert got >> 24 == alpha
                        assert (got >> sh) & 0xFF == int(want[v]), (v, k, o, sh)
                        assert (got >> others[0]) & 0xFF == int(want[a]) and (got >> others[1]) & 0xFF == int(want[b])
                        if alpha == 0x80 and sh == 16:
                            ch = [(argb >> s) & 0xFF for s in (16, 8, 0)]
                            rec = (C.c_uint32 * 4)(*[(k - o) * x + o * (x >> 1) for x in ch], k)
                            assert got == h.rt_accum_resolve(rec, argb)


def test_resolve_edges():
    h = _h()
    rng = np.random.default_rng(7)
    for argb in [0, 0xFFFFFFFF, 0x80010203, 0x7FFEFDFC] + [int(x) for x in rng.integers(0, 1 << 32, 64)]:
        for k in range(1, 17):
            assert h.rt_lights_resolve(argb, 0, k) == argb                        # every light sees it
        # one light that does not: shadow_attenuate, c >> 1 per channel under c's alpha
        assert h.rt_lights_resolve(argb, 1, 1) == (argb & 0xFF000000) | ((argb >> 1) & 0x007F7F7F)
