"""CPU-side tests of progressive accumulation (vx_rt.h rt_renderer_accum_begin;
no GPU calls): librtapp.so exports the new entry points, and rt_accum_resolve
-- the host restatement of the resolve the pt_accum image ends every launch
with -- equals a numpy restatement of (2 * sum + n) // (2 * n) per channel
under the alpha it is given."""
import ctypes as C
import os

import numpy as np
import pytest

os.environ.setdefault("SKYBOX_RT_NO_TORCH", "1")

from skybox_rt_amd import _lib  # noqa: E402

SYMBOLS = ("rt_renderer_accum_begin", "rt_renderer_accum_reset", "rt_render_accumulate_start",
           "rt_render_accumulate", "rt_renderer_accum_samples", "rt_read_accum", "rt_accum_resolve")
NS = (1, 2, 3, 7, 32, 1 << 24)


@pytest.fixture(scope="module")
def h():
    if _lib.missing():
        _lib.build()
    assert not _lib.missing()
    return C.CDLL(os.path.join(_lib.LIB_DIR, "librtapp.so"))


def test_librtapp_exports_the_accumulation_entry_points(h):
    for n in SYMBOLS:
        assert hasattr(h, n), f"librtapp.so does not export {n}"
    assert "pt_accum.vxbin" in _lib.REQUIRED


def _sums(n):
    """0, 255 n, and for n <= 7 every sum there is (all the .5 boundaries and
    both their neighbours among them); for larger n the boundaries q n + n / 2
    of a spread of quotients q with their neighbours."""
    if n <= 7:
        return list(range(0, 255 * n + 1))
    out = {0, 1, 255 * n - 1, 255 * n}
    for q in (0, 1, 2, 127, 128, 253, 254):
        for half in ((n - 1) // 2, n // 2, (n + 1) // 2):
            for d in (-1, 0, 1):
                s = q * n + half + d
                if 0 <= s <= 255 * n:
                    out.add(s)
    return sorted(out)


def _model(sums, n, alpha):
    s = np.asarray(sums, np.uint64)
    m = (2 * s + np.uint64(n)) // np.uint64(2 * n)
    assert int(m.max()) <= 255
    return (np.uint64(alpha & 0xFF000000) | (m[:, 0] << np.uint64(16)) | (m[:, 1] << np.uint64(8))
            | m[:, 2]).astype(np.uint32)


@pytest.mark.parametrize("n", NS)
def test_resolve_equals_the_numpy_restatement(h, n):
    h.rt_accum_resolve.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
    h.rt_accum_resolve.restype = C.c_uint32
    sums = _sums(n)
    # every listed sum in each channel, against two other channels that move too
    recs = np.array([(s, sums[(i * 7 + 3) % len(sums)], sums[-1 - i]) for i, s in enumerate(sums)]
                    + [(sums[-1 - i], s, sums[(i * 5 + 1) % len(sums)]) for i, s in enumerate(sums)]
                    + [(sums[(i * 3 + 2) % len(sums)], sums[-1 - i], s) for i, s in enumerate(sums)], np.uint64)
    for alpha in (0xFF000000, 0x00000000, 0x80FFFFFF, 0x12345678):
        want = _model(recs, n, alpha)
        got = np.empty(len(recs), np.uint32)
        for i, (r, g, b) in enumerate(recs):
            rec = (C.c_uint32 * 4)(int(r), int(g), int(b), n)
            got[i] = h.rt_accum_resolve(rec, alpha)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (n, hex(alpha), recs[bad[0]].tolist(), hex(int(got[bad[0]])), hex(int(want[bad[0]])))


def test_one_sample_resolves_to_itself(h):
    h.rt_accum_resolve.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
    h.rt_accum_resolve.restype = C.c_uint32
    for px in (0xFF000000, 0xFFFFFFFF, 0xFF123456, 0x7F80FF01):
        rec = (C.c_uint32 * 4)((px >> 16) & 0xFF, (px >> 8) & 0xFF, px & 0xFF, 1)
        assert h.rt_accum_resolve(rec, px) == px
    # k samples of one colour: that colour for any n
    for n in NS:
        rec = (C.c_uint32 * 4)(0x12 * n, 0xFE * n, 0x01 * n, n)
        assert h.rt_accum_resolve(rec, 0xFF000000) == 0xFF12FE01
