"""The output merger's state sweep, shared by test_om_unit_cpu.py (oracle
against tests/om_reference.py) and test_gpu_om_unit.py (om.vxbin against
both).  Imports neither the product nor, until a case is run, the oracle.

A case is one launch of the OM regression app at the DCR level: a frame of
W x H pixels with known colour and depth/stencil contents, the 18 OM DCR
words, the face, and the app's arguments.  num_tasks = H, so a blending
case's source alpha in row y is (y * 255) & 0xff = -y & 0xff.

Families (the frames are built once and never written):
  blend   256 x 256, blend_enable, destination x * 0x01010101: every (source
          alpha, destination channel) pair occurs once per state
  logic   256 x 256, random destination colours
  ds      256 x 8, stencil byte = x, depth by row around the incoming depth
          (the tie, +-1, +-2, 0, 0xffffff, the far half), colour mask 0xA
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

import om_reference as R

BLEND_RGB = 0xE05A17            # source r, g, b all different, none 0 or 0xff
BLEND_CONST = 0x40C81E7B        # four different bytes
DS_DEPTH = 0x5A123456           # the high byte is not part of the depth
DS_REF = DS_DEPTH & 0xFFFFFF
DS_COLOR = 0x3C96D2
DS_ROWS = (DS_REF - 2, DS_REF - 1, DS_REF, DS_REF + 1, DS_REF + 2, 0, 0xFFFFFF, DS_REF ^ 0x800000)
# (stencil write mask, stencil mask, depth write mask)
DS_MASKS = ((0xFF, 0xFF, 1), (0x0F, 0xF0, 0), (0x00, 0x3C, 1))
DS_REFS = (0x6B, 0x94)          # front / back reference value
# (zpass, zfail, fail) triples: every operation occurs once in every slot
DS_TRIPLES = tuple((i, (i + 3) % 8, (i + 5) % 8) for i in range(8))


@dataclass
class Case:
    name: str
    family: str
    dcr: np.ndarray
    backface: bool = False
    blend_enable: bool = False
    rgb: int = 0xFFFFFF
    depth: int = 0


def _frame(family):
    if family == "blend":
        x = np.arange(256, dtype=np.uint32)
        c = np.broadcast_to(x * np.uint32(0x01010101), (256, 256)).copy()
        z = np.zeros((256, 256), np.uint32)
    elif family == "logic":
        rng = np.random.default_rng(20)
        c = rng.integers(0, 1 << 32, (256, 256), dtype=np.uint64).astype(np.uint32)
        z = np.zeros((256, 256), np.uint32)
    else:
        rng = np.random.default_rng(21)
        c = rng.integers(0, 1 << 32, (8, 256), dtype=np.uint64).astype(np.uint32)
        x = np.arange(256, dtype=np.uint32)[None, :]
        z = (x << np.uint32(24)) | np.asarray(DS_ROWS, np.uint32)[:, None]
    c.setflags(write=False)
    z.setflags(write=False)
    return c, z


_FRAMES = {}


def frame(family):
    """(colour, depth/stencil) uint32[H, W] before the launch; read-only"""
    if family not in _FRAMES:
        _FRAMES[family] = _frame(family)
    return _FRAMES[family]


def blend_cases():
    out = []

    def add(name, mode, func):
        out.append(Case(name, "blend", R.make_dcr(mode=mode, func=func, const=BLEND_CONST),
                        blend_enable=True, rgb=BLEND_RGB))

    for m in (R.ADD, R.SUB, R.REV_SUB):
        for f in range(15):
            for g in (R.F_ZERO, R.F_ONE_MINUS_SRC_A, R.F_DST_RGB):
                add(f"m{m}_src{f}_dst{g}", (m, m), (f, f, g, g))
            for g in (R.F_ONE, R.F_SRC_A, R.F_ONE_MINUS_DST_RGB):
                add(f"m{m}_dst{f}_src{g}", (m, m), (g, g, f, f))
    add("min", (R.MIN, R.MIN), (R.F_ONE, R.F_ONE, R.F_ZERO, R.F_ZERO))
    add("max", (R.MAX, R.MAX), (R.F_SRC_A, R.F_DST_A, R.F_CONST_RGB, R.F_ALPHA_SAT))
    # four different BLEND_FUNC bytes, different rgb and alpha modes
    for i, (mode, func) in enumerate((
            ((R.ADD, R.SUB), (R.F_SRC_A, R.F_ONE, R.F_ONE_MINUS_SRC_A, R.F_DST_A)),
            ((R.SUB, R.ADD), (R.F_ONE, R.F_CONST_A, R.F_SRC_RGB, R.F_ONE_MINUS_DST_A)),
            ((R.REV_SUB, R.ADD), (R.F_CONST_RGB, R.F_ONE_MINUS_SRC_RGB, R.F_ONE, R.F_SRC_A)),
            ((R.ADD, R.REV_SUB), (R.F_ALPHA_SAT, R.F_ZERO, R.F_ONE_MINUS_CONST_A, R.F_ONE)),
            ((R.MIN, R.ADD), (R.F_ZERO, R.F_DST_RGB, R.F_ONE, R.F_ONE_MINUS_CONST_RGB)),
            ((R.ADD, R.MAX), (R.F_DST_A, R.F_ONE, R.F_ONE_MINUS_DST_RGB, R.F_ZERO)),
            ((R.MAX, R.SUB), (R.F_ONE, R.F_ONE_MINUS_DST_A, R.F_ZERO, R.F_SRC_RGB)),
            ((R.SUB, R.REV_SUB), (R.F_ONE_MINUS_SRC_A, R.F_DST_RGB, R.F_CONST_A, R.F_ONE)))):
        assert len(set(func)) == 4 and mode[0] != mode[1]
        add(f"mixed{i}", mode, func)
    return out


def logic_cases():
    out = []
    for cmask in (0xF, 0x5, 0x0):
        for op in range(16):
            out.append(Case(f"op{op}_mask{cmask:x}", "logic",
                            R.make_dcr(cmask=cmask, mode=(R.LOGICOP, R.LOGICOP), logic_op=op),
                            blend_enable=True, rgb=0xA5C33C))
    # LOGICOP in one half of the mode word only
    out.append(Case("rgb_half", "logic",
                    R.make_dcr(mode=(R.LOGICOP, R.ADD), logic_op=9, const=BLEND_CONST,
                               func=(R.F_ZERO, R.F_SRC_A, R.F_ZERO, R.F_ONE_MINUS_SRC_A)),
                    blend_enable=True, rgb=0xA5C33C))
    out.append(Case("alpha_half", "logic",
                    R.make_dcr(cmask=0xB, mode=(R.REV_SUB, R.LOGICOP), logic_op=2, const=BLEND_CONST,
                               func=(R.F_SRC_A, R.F_ZERO, R.F_ONE, R.F_ZERO)),
                    blend_enable=True, rgb=0xA5C33C))
    return out


def ds_case(backface, depth_func, stencil_func, triple, masks):
    """One depth/stencil state.  The other face's half of every stencil word
    holds different values, so a wrong shift shows."""
    swm, mask, dwm = masks
    me, other = (1, 0) if backface else (0, 1)

    def pair(mine, theirs):
        p = [0, 0]
        p[me], p[other] = mine, theirs
        return tuple(p)

    zp, zf, fl = triple
    dcr = R.make_dcr(cmask=0xA, depth_func=depth_func, depth_wm=dwm,
                     stencil_func=pair(stencil_func, (stencil_func + 3) % 8),
                     zpass=pair(zp, (zp + 1) % 8), zfail=pair(zf, (zf + 2) % 8),
                     fail=pair(fl, (fl + 5) % 8), ref=pair(DS_REFS[me], DS_REFS[other]),
                     mask=pair(mask, mask ^ 0x5A), swm=pair(swm, swm ^ 0xA5))
    name = f"{'back' if backface else 'front'}_d{depth_func}_s{stencil_func}_op{zp}{zf}{fl}_wm{swm:02x}"
    return Case(name, "ds", dcr, backface=bool(backface), rgb=DS_COLOR, depth=DS_DEPTH)


def ds_cases(backface, depth_func):
    """the 8 stencil functions x 8 triples x 3 mask sets of one face and
    depth function: 192 states"""
    return [ds_case(backface, depth_func, sf, t, m)
            for sf in range(8) for t in DS_TRIPLES for m in DS_MASKS]


DS_GROUPS = [(b, f) for b in (0, 1) for f in range(8)]


def source_color(case):
    """uint32[H, 1]: the app's colour of every row, num_tasks = H"""
    h = frame(case.family)[0].shape[0]
    return R.alpha_ramp(h, h, case.rgb, case.blend_enable)


def reference(case, variant=None):
    c, z = frame(case.family)
    return R.om_reference(case.dcr, case.backface, source_color(case), case.depth, c, z,
                          variant=variant)


def oracle_app(po, dcr, backface, blend_enable, num_tasks, rgb, depth, cbuf, zbuf):
    """orc_om_app (oracle/gfx.c) on copies of cbuf / zbuf -> (colour, depth/stencil)"""
    L = po.lib()
    L.orc_om_app.argtypes = [C.c_uint32] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    h, w = cbuf.shape
    c = np.ascontiguousarray(cbuf, np.uint32).copy()
    z = np.ascontiguousarray(zbuf, np.uint32).copy()
    d = np.ascontiguousarray(dcr, np.uint32)
    rc = L.orc_om_app(w, h, num_tasks, rgb & 0xFFFFFFFF, depth & 0xFFFFFFFF, int(backface),
                      int(blend_enable), d.ctypes.data, c.ctypes.data, z.ctypes.data)
    assert rc == 0, rc
    return c, z


def oracle(po, case):
    c, z = frame(case.family)
    return oracle_app(po, case.dcr, case.backface, case.blend_enable, c.shape[0], case.rgb,
                      case.depth, c, z)
