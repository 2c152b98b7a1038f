"""om.vxbin driven at the DCR level through the Vortex C ABI: the state sweep
of tests/om_sweep.py on the device, against the independent model of the
unit (tests/om_reference.py) and the oracle (orc_om_app), bit for bit on the
colour and the depth/stencil plane; and the edges only the device has --
partial waves, waves that span two rows, pitches wider than the row, planes
at an offset inside their allocation, and every byte outside the frame left
alone.  One device and one kernel upload for the module."""
import os
import struct

import numpy as np
import pytest

import om_reference as R
import om_sweep as S
from om_known_answers import KNOWN_ANSWERS

pytestmark = pytest.mark.gpu

from skybox_rt_amd import _lib, vortex  # noqa: E402

ALLOC = 256 * 256 * 4 + 8192
GUARD = 256


class Rig:
    def __init__(self):
        self.dev = vortex.Device()
        self.kernel = self.dev.upload_kernel_file(os.path.join(_lib.LIB_DIR, "om.vxbin"))
        self.cb = self.dev.mem_alloc(ALLOC)
        self.zb = self.dev.mem_alloc(ALLOC)
        self.args = self.dev.mem_alloc(64)
        assert self.cb.address % 64 == 0 and self.zb.address % 64 == 0
        self.fill = np.random.default_rng(5).integers(0, 256, ALLOC, dtype=np.uint8)

    def close(self):
        self.dev.close()

    def _image(self, plane, off, pitch):
        h, w = plane.shape
        assert off % 64 == 0 and pitch % 4 == 0 and pitch >= 4 * w
        size = off + pitch * h + GUARD
        assert size <= ALLOC
        img = self.fill[:size].copy()
        rows = np.lib.stride_tricks.as_strided(img[off:], (h, 4 * w), (pitch, 1))
        inside = np.zeros(size, bool)
        np.lib.stride_tricks.as_strided(inside[off:], (h, 4 * w), (pitch, 1))[:] = True
        rows[:] = np.ascontiguousarray(plane, np.uint32).view(np.uint8).reshape(h, 4 * w)
        return img, inside

    @staticmethod
    def _plane(img, off, pitch, h, w):
        rows = np.lib.stride_tricks.as_strided(img[off:], (h, 4 * w), (pitch, 1))
        return np.ascontiguousarray(rows).view(np.uint32).reshape(h, w)

    def launch(self, dcr, backface, blend_enable, num_tasks, rgb, depth, cbuf, zbuf,
               c_off=0, z_off=0, c_pitch=None, z_pitch=None):
        """-> (colour, depth/stencil, colour bytes unchanged, depth/stencil
        bytes unchanged); asserts that no byte outside the W x H words of
        either plane changed"""
        h, w = cbuf.shape
        c_pitch, z_pitch = c_pitch or 4 * w, z_pitch or 4 * w
        cimg, cin = self._image(cbuf, c_off, c_pitch)
        zimg, zin = self._image(zbuf, z_off, z_pitch)
        self.cb.write(cimg.tobytes())
        self.zb.write(zimg.tobytes())
        words = [int(v) for v in dcr]
        words[R.CBUF_ADDR], words[R.CBUF_PITCH] = (self.cb.address + c_off) // 64, c_pitch
        words[R.ZBUF_ADDR], words[R.ZBUF_PITCH] = (self.zb.address + z_off) // 64, z_pitch
        for i, v in enumerate(words):
            self.dev.dcr_write(R.OM_STATE_BEGIN + i, v)
        # om_arg_t: num_tasks, width, height, color, depth, backface, blend_enable, use_sw
        self.args.write(struct.pack("<5I3Bx", num_tasks, w, h, rgb & 0xFFFFFFFF, depth & 0xFFFFFFFF,
                                    int(bool(backface)), int(bool(blend_enable)), 0))
        self.dev.start(self.kernel, self.args)
        self.dev.ready_wait()
        cout = np.frombuffer(self.cb.read(len(cimg)), np.uint8)
        zout = np.frombuffer(self.zb.read(len(zimg)), np.uint8)
        assert np.array_equal(cout[~cin], cimg[~cin]), "colour bytes outside the frame changed"
        assert np.array_equal(zout[~zin], zimg[~zin]), "depth/stencil bytes outside the frame changed"
        return (self._plane(cout, c_off, c_pitch, h, w), self._plane(zout, z_off, z_pitch, h, w),
                np.array_equal(cout, cimg), np.array_equal(zout, zimg))

    def run_case(self, case):
        c, z = S.frame(case.family)
        return self.launch(case.dcr, case.backface, case.blend_enable, c.shape[0], case.rgb,
                           case.depth, c, z)[:2]


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


def _check_cases(rig, po, cases):
    bad = []
    for case in cases:
        gc, gz = rig.run_case(case)
        rc, rz = S.reference(case)
        oc, oz = S.oracle(po, case)
        n = int((gc != rc).sum()) + int((gz != rz).sum()) + int((gc != oc).sum()) + int((gz != oz).sum())
        if n:
            bad.append((case.name, n))
    assert bad == []


# ---- the sweep ----
_BLEND = S.blend_cases()


@pytest.mark.parametrize("part", range(7))
def test_blend_arithmetic_sweep(rig, oracle_lib, part):
    cases = _BLEND[part::7]
    assert len(cases) == 40
    _check_cases(rig, oracle_lib, cases)


def test_logic_op_sweep(rig, oracle_lib):
    _check_cases(rig, oracle_lib, S.logic_cases())


@pytest.mark.parametrize("backface,depth_func", S.DS_GROUPS,
                         ids=[f"{'back' if b else 'front'}_d{f}" for b, f in S.DS_GROUPS])
def test_depth_stencil_sweep(rig, oracle_lib, backface, depth_func):
    _check_cases(rig, oracle_lib, S.ds_cases(backface, depth_func))


# ---- the hand table ----
def test_known_answers(rig):
    """a 1 x 256 frame, every row a task: row -alpha & 0xff carries the
    entry's source alpha"""
    for name, kw, back, src, depth, c0, z0, c1, z1 in KNOWN_ANSWERS:
        c, z, _, _ = rig.launch(R.make_dcr(**kw), back, True, 256, src & 0xFFFFFF, depth,
                                np.full((256, 1), c0, np.uint32), np.full((256, 1), z0, np.uint32))
        row = -(src >> 24) & 0xFF
        assert (hex(int(c[row, 0])), hex(int(z[row, 0]))) == (hex(c1), hex(z1)), name


# ---- edges only the device has ----
# everything on at once: depth LEQUAL with depth writes, a masked stencil test
# whose three slots all occur, alpha blending, a partial colour mask
EDGE_DCR = R.make_dcr(cmask=0x7, depth_func=R.LEQUAL, depth_wm=1, stencil_func=(R.LESS, R.NEVER),
                      zpass=(R.INCR_WRAP, R.KEEP), zfail=(R.INVERT, R.ZERO), fail=(R.DECR, R.REPLACE),
                      ref=(0x70, 0x11), mask=(0xF0, 0x0F), swm=(0x3F, 0xC0),
                      func=(R.F_SRC_A, R.F_ONE, R.F_ONE_MINUS_SRC_A, R.F_DST_A))
EDGE_RGB, EDGE_DEPTH = 0x2E8B57, 0xA5400000


def _edge_frame(w, h, seed):
    """random colours and stencil bytes, depths at and around the incoming one"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(np.uint32)
    d = (EDGE_DEPTH & 0xFFFFFF) + rng.integers(-1, 2, (h, w))
    z = ((rng.integers(0, 256, (h, w)) << 24) | d).astype(np.uint32)
    return c, z


def _check_edge(rig, po, w, h, num_tasks=None, dcr=EDGE_DCR, backface=False, **where):
    c0, z0 = _edge_frame(w, h, 100 * w + h)
    nt = num_tasks or h
    gc, gz, c_same, z_same = rig.launch(dcr, backface, True, nt, EDGE_RGB, EDGE_DEPTH, c0, z0, **where)
    rc, rz = R.om_reference(dcr, backface, R.alpha_ramp(h, nt, EDGE_RGB), EDGE_DEPTH, c0, z0)
    oc, oz = S.oracle_app(po, dcr, backface, True, nt, EDGE_RGB, EDGE_DEPTH, c0, z0)
    assert np.array_equal(rc, oc) and np.array_equal(rz, oz)
    assert int((gc != rc).sum()) == 0 and int((gz != rz).sum()) == 0
    return c0, z0, gc, gz, c_same, z_same


@pytest.mark.parametrize("h", (1, 5))
@pytest.mark.parametrize("w", (1, 63, 64, 65, 67))
def test_partial_waves_and_rows(rig, oracle_lib, w, h):
    c0, z0, gc, gz, _, _ = _check_edge(rig, oracle_lib, w, h)
    if w >= 63:         # the state does something: to depth/stencil always, to colour
        assert (gz != z0).any()         # once a row has a non-zero alpha (row 0 has alpha 0)
        assert (gc != c0).any() == (h > 1)


def test_pitch_wider_than_the_row(rig, oracle_lib):
    _check_edge(rig, oracle_lib, 67, 5, c_pitch=320, z_pitch=320)


def test_planes_at_offsets_with_different_pitches(rig, oracle_lib):
    _check_edge(rig, oracle_lib, 67, 5, c_off=192, z_off=4096 + 64, c_pitch=320, z_pitch=384)
    _check_edge(rig, oracle_lib, 65, 5, backface=True, c_off=64, z_off=128, c_pitch=512, z_pitch=260)


def test_colour_mask_zero_leaves_the_colour_allocation_alone(rig, oracle_lib):
    dcr = EDGE_DCR.copy()
    dcr[R.CBUF_WRITEMASK] = 0
    c0, z0, gc, gz, c_same, _ = _check_edge(rig, oracle_lib, 67, 5, dcr=dcr, c_pitch=320)
    assert c_same and (gz != z0).any()


def test_never_applies_only_the_fail_op(rig, oracle_lib):
    dcr = R.make_dcr(depth_func=R.LEQUAL, depth_wm=1, stencil_func=(R.NEVER, R.ALWAYS),
                     zpass=(R.ZERO, R.KEEP), zfail=(R.REPLACE, R.KEEP), fail=(R.INCR_WRAP, R.KEEP),
                     ref=(0x55, 0), mask=(0xFF, 0xFF), swm=(0xFF, 0),
                     func=(R.F_SRC_A, R.F_ONE, R.F_ONE_MINUS_SRC_A, R.F_DST_A))
    c0, z0, gc, gz, c_same, _ = _check_edge(rig, oracle_lib, 67, 5, dcr=dcr)
    assert c_same
    assert np.array_equal(gz & 0xFFFFFF, z0 & 0xFFFFFF)
    assert np.array_equal(gz >> 24, ((z0 >> 24) + 1) & 0xFF)
    # depth NEVER: the zfail slot, depth kept
    dcr = R.make_dcr(depth_func=R.NEVER, depth_wm=1, stencil_func=(R.ALWAYS, R.NEVER),
                     zpass=(R.ZERO, R.KEEP), zfail=(R.DECR_WRAP, R.KEEP), fail=(R.REPLACE, R.KEEP),
                     ref=(0x55, 0), mask=(0xFF, 0xFF), swm=(0xFF, 0))
    c0, z0, gc, gz, c_same, _ = _check_edge(rig, oracle_lib, 65, 5, dcr=dcr)
    assert c_same
    assert np.array_equal(gz & 0xFFFFFF, z0 & 0xFFFFFF)
    assert np.array_equal(gz >> 24, ((z0 >> 24) - 1) & 0xFF)


@pytest.mark.parametrize("num_tasks", (1, 7, 37, 111))
def test_alpha_ramp_partitions(rig, oracle_lib, num_tasks):
    dcr = R.make_dcr(func=(R.F_SRC_A, R.F_SRC_A, R.F_ONE_MINUS_SRC_A, R.F_ONE_MINUS_SRC_A))
    c0, _, gc, _, _, _ = _check_edge(rig, oracle_lib, 16, 37, num_tasks=num_tasks, dcr=dcr)
    if num_tasks > 1:       # one task: alpha 0 everywhere, the destination survives
        assert (gc != c0).any()
    else:
        assert np.array_equal(gc, c0)
