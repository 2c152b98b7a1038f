"""The output merger (OM) unit in plain numpy: an independent model of what
gfx::om_write (kernels/gfx_device.h) and orc_om_write (oracle/gfx.c) restate.

Written from the unit's definition -- DepthTencil::configure / ::test,
Blender::configure / ::blend, DoCompare, DoStencilOp, DoLogicOp, DoBlendFunc,
DoBlendMode (sim/common/graphics.cpp:320-636) and OutputMerger::configure /
::read / ::write (sim/simx/om_unit.cpp:28-136) -- over whole arrays, int64 per
channel.  It calls neither the oracle nor the product, and shares no table
with them: the tests hold both to it.

    om_reference(dcr18, backface, src_color, depth, cbuf, zbuf) -> (cbuf', zbuf')

dcr18[i] is the DCR word VX_DCR_OM_STATE_BEGIN + i (words 0, 1, 3, 4 -- the
buffer addresses and pitches -- are not read).  src_color / depth broadcast
against cbuf / zbuf, so the regression app's per-row alpha ramp (alpha_ramp)
fits.  State values outside the unit's enums raise ValueError.

`variant` is for the discrimination checks only: a deliberately wrong unit
("trunc": x // 255 for the rounding division, "no_round": no +0x80,
"no_clamp": no 0xFF00 clamp, "face_swap": the other face's half words).
"""
import numpy as np

# DCR word indices (VX_types.h VX_DCR_OM_*, relative to VX_DCR_OM_STATE_BEGIN)
CBUF_ADDR, CBUF_PITCH, CBUF_WRITEMASK, ZBUF_ADDR, ZBUF_PITCH = 0, 1, 2, 3, 4
DEPTH_FUNC, DEPTH_WRITEMASK = 5, 6
STENCIL_FUNC, STENCIL_ZPASS, STENCIL_ZFAIL, STENCIL_FAIL = 7, 8, 9, 10
STENCIL_REF, STENCIL_MASK, STENCIL_WRITEMASK = 11, 12, 13
BLEND_MODE, BLEND_FUNC, BLEND_CONST, LOGIC_OP = 14, 15, 16, 17
OM_STATE_BEGIN = 0x022      # VX_DCR_OM_STATE_BEGIN

# compare functions (VX_OM_DEPTH_FUNC_*)
ALWAYS, NEVER, LESS, LEQUAL, EQUAL, GEQUAL, GREATER, NOTEQUAL = range(8)
# stencil operations (VX_OM_STENCIL_OP_*)
KEEP, ZERO, REPLACE, INCR, DECR, INVERT, INCR_WRAP, DECR_WRAP = range(8)
# blend modes (VX_OM_BLEND_MODE_*)
ADD, SUB, REV_SUB, MIN, MAX, LOGICOP = range(6)
# blend factors (VX_OM_BLEND_FUNC_*)
(F_ZERO, F_ONE, F_SRC_RGB, F_ONE_MINUS_SRC_RGB, F_DST_RGB, F_ONE_MINUS_DST_RGB, F_SRC_A,
 F_ONE_MINUS_SRC_A, F_DST_A, F_ONE_MINUS_DST_A, F_CONST_RGB, F_ONE_MINUS_CONST_RGB, F_CONST_A,
 F_ONE_MINUS_CONST_A, F_ALPHA_SAT) = range(15)

DEPTH_BITS = 24
DEPTH_MASK = 0xFFFFFF
U32 = 0xFFFFFFFF


def make_dcr(cmask=0xF, depth_func=ALWAYS, depth_wm=0, stencil_func=(ALWAYS, ALWAYS),
             zpass=(KEEP, KEEP), zfail=(KEEP, KEEP), fail=(KEEP, KEEP), ref=(0, 0),
             mask=(0xFF, 0xFF), swm=(0, 0), mode=(ADD, ADD), func=(F_ONE, F_ONE, F_ZERO, F_ZERO),
             const=0, logic_op=0):
    """The 18 OM DCR words.  Pairs are (front, back); mode is (rgb, alpha);
    func is (src rgb, src alpha, dst rgb, dst alpha).  The defaults are the
    unit switched off: every test off, blending off, full colour mask."""
    pair = lambda p: (p[0] & 0xFFFF) | ((p[1] & 0xFFFF) << 16)
    d = np.zeros(18, np.uint32)
    d[CBUF_WRITEMASK] = cmask
    d[DEPTH_FUNC], d[DEPTH_WRITEMASK] = depth_func, depth_wm
    d[STENCIL_FUNC], d[STENCIL_ZPASS] = pair(stencil_func), pair(zpass)
    d[STENCIL_ZFAIL], d[STENCIL_FAIL] = pair(zfail), pair(fail)
    d[STENCIL_REF], d[STENCIL_MASK], d[STENCIL_WRITEMASK] = pair(ref), pair(mask), pair(swm)
    d[BLEND_MODE] = pair(mode)
    d[BLEND_FUNC] = func[0] | (func[1] << 8) | (func[2] << 16) | (func[3] << 24)
    d[BLEND_CONST], d[LOGIC_OP] = const, logic_op
    return d


def alpha_ramp(height, num_tasks, rgb, blend_enable=True):
    """The regression app's source colour of every row (om/kernel.cpp:16-38)
    as uint32[height, 1]: rows are dealt to num_tasks tasks of tile_h rows and
    a task's alpha is uint32(float32(task) * float32(255 / tile_h)); the
    colour word is (alpha << 24) | rgb in 32 bits, so alpha bits above 8 fall
    off.  Without blend_enable alpha is 0xff."""
    tile_h = (height + num_tasks - 1) // num_tasks
    task = np.arange(height, dtype=np.int64) // tile_h
    if blend_enable:
        step = np.float32(255.0) / np.float32(tile_h)
        alpha = (task.astype(np.float32) * step).astype(np.int64)
    else:
        alpha = np.full(height, 0xFF, np.int64)
    return (((alpha << 24) | (rgb & 0xFFFFFF)) & U32).astype(np.uint32).reshape(height, 1)


def _compare(func, a, b):
    lt, eq = a < b, a == b
    if func == ALWAYS:
        return np.ones_like(lt)
    if func == NEVER:
        return np.zeros_like(lt)
    if func == LESS:
        return lt
    if func == LEQUAL:
        return lt | eq
    if func == EQUAL:
        return eq
    if func == GEQUAL:
        return ~lt
    if func == GREATER:
        return ~(lt | eq)
    if func == NOTEQUAL:
        return ~eq
    raise ValueError(f"compare function {func}")


def _stencil_op(op, ref, val):
    """val: int64 stencil bytes; the result still carries what `<< 24` drops"""
    if op == KEEP:
        return val
    if op == ZERO:
        return np.zeros_like(val)
    if op == REPLACE:
        return np.full_like(val, ref)
    if op == INCR:
        return np.where(val < 0xFF, val + 1, val)
    if op == DECR:
        return np.where(val > 0, val - 1, val)
    if op == INVERT:
        return ~val
    if op == INCR_WRAP:
        return (val + 1) & 0xFF
    if op == DECR_WRAP:
        return (val - 1) & 0xFF
    raise ValueError(f"stencil operation {op}")


def _channels(word):
    w = np.asarray(word).astype(np.int64)
    return {"a": (w >> 24) & 0xFF, "r": (w >> 16) & 0xFF, "g": (w >> 8) & 0xFF, "b": w & 0xFF}


def _factor(f, ch, src, dst, cst):
    """blend factor f for channel ch ('a', 'r', 'g' or 'b')"""
    if f == F_ZERO:
        return np.int64(0)
    if f == F_ONE:
        return np.int64(0xFF)
    if f == F_SRC_RGB:
        return src[ch]
    if f == F_ONE_MINUS_SRC_RGB:
        return 0xFF - src[ch]
    if f == F_DST_RGB:
        return dst[ch]
    if f == F_ONE_MINUS_DST_RGB:
        return 0xFF - dst[ch]
    if f == F_SRC_A:
        return src["a"]
    if f == F_ONE_MINUS_SRC_A:
        return 0xFF - src["a"]
    if f == F_DST_A:
        return dst["a"]
    if f == F_ONE_MINUS_DST_A:
        return 0xFF - dst["a"]
    if f == F_CONST_RGB:
        return cst[ch]
    if f == F_CONST_A:
        return cst["a"]
    if f in (F_ONE_MINUS_CONST_RGB, F_ONE_MINUS_CONST_A):
        # the unit's ONE_MINUS_CONST_A is per channel too (graphics.cpp:463-469)
        return 0xFF - cst[ch]
    if f == F_ALPHA_SAT:
        return np.int64(0xFF) if ch == "a" else np.minimum(src["a"], 0xFF - dst["a"])
    raise ValueError(f"blend factor {f}")


_LOGIC = {      # DoLogicOp on the packed words (int64; the caller keeps 32 bits)
    0: lambda s, d: np.zeros_like(s), 1: lambda s, d: s & d, 2: lambda s, d: s & ~d,
    3: lambda s, d: s, 4: lambda s, d: ~s & d, 5: lambda s, d: d, 6: lambda s, d: s ^ d,
    7: lambda s, d: s | d, 8: lambda s, d: ~(s | d), 9: lambda s, d: ~(s ^ d),
    10: lambda s, d: ~d, 11: lambda s, d: s | ~d, 12: lambda s, d: ~s, 13: lambda s, d: ~s | d,
    14: lambda s, d: ~(s & d), 15: lambda s, d: np.full_like(s, -1),
}


def _div255(x, variant):
    if variant == "trunc":
        return x // 255
    return (x + (x >> 8)) >> 8


def _mode(mode, ch, fs, fd, src, dst, srcw, dstw, lop, variant):
    """one channel of DoBlendMode, as the byte ColorARGB keeps of it"""
    half = 0 if variant == "no_round" else 0x80
    s, d = src[ch], dst[ch]
    if mode == ADD:
        x = s * fs + d * fd + half
        if variant != "no_clamp":
            x = np.minimum(x, 0xFF00)
        out = _div255(x, variant)
    elif mode == SUB:
        out = _div255(np.maximum(s * fs - d * fd + half, 0), variant)
    elif mode == REV_SUB:
        out = _div255(np.maximum(d * fd - s * fs + half, 0), variant)
    elif mode == MIN:
        out = np.minimum(s, d)
    elif mode == MAX:
        out = np.maximum(s, d)
    elif mode == LOGICOP:
        if lop not in _LOGIC:
            raise ValueError(f"logic op {lop}")
        out = _channels(_LOGIC[lop](srcw, dstw) & U32)[ch]
    else:
        raise ValueError(f"blend mode {mode}")
    return out & 0xFF


def om_reference(dcr18, backface, src_color, depth, cbuf, zbuf, variant=None):
    dcr = [int(v) & U32 for v in dcr18]
    assert len(dcr) == 18
    cbuf = np.asarray(cbuf)
    zbuf = np.asarray(zbuf)
    assert cbuf.dtype == np.uint32 and zbuf.dtype == np.uint32 and cbuf.shape == zbuf.shape
    shape = cbuf.shape
    srcw = np.broadcast_to(np.asarray(src_color).astype(np.int64) & U32, shape)
    depth = np.broadcast_to(np.asarray(depth).astype(np.int64) & U32, shape)
    dst_c_mem = cbuf.astype(np.int64)
    dst_z_mem = zbuf.astype(np.int64)

    # ---- configure ----
    back = bool(backface) != (variant == "face_swap")
    half = (lambda w: w >> 16) if back else (lambda w: w & 0xFFFF)
    depth_func = dcr[DEPTH_FUNC]
    depth_wm = dcr[DEPTH_WRITEMASK] & 1
    s_func, s_zpass = half(dcr[STENCIL_FUNC]), half(dcr[STENCIL_ZPASS])
    s_zfail, s_fail = half(dcr[STENCIL_ZFAIL]), half(dcr[STENCIL_FAIL])
    s_ref, s_mask, s_wm = half(dcr[STENCIL_REF]), half(dcr[STENCIL_MASK]), half(dcr[STENCIL_WRITEMASK])
    depth_on = not (depth_func == ALWAYS and not depth_wm)
    stencil_on = not (s_func == ALWAYS and s_zpass == KEEP and s_zfail == KEEP)
    mode_rgb, mode_a = dcr[BLEND_MODE] & 0xFFFF, dcr[BLEND_MODE] >> 16
    f_src_rgb, f_src_a = dcr[BLEND_FUNC] & 0xFF, (dcr[BLEND_FUNC] >> 8) & 0xFF
    f_dst_rgb, f_dst_a = (dcr[BLEND_FUNC] >> 16) & 0xFF, (dcr[BLEND_FUNC] >> 24) & 0xFF
    blend_on = (mode_rgb, mode_a, f_src_rgb, f_src_a, f_dst_rgb, f_dst_a) != \
        (ADD, ADD, F_ONE, F_ONE, F_ZERO, F_ZERO)
    cmask4 = dcr[CBUF_WRITEMASK] & 0xF
    cmask = sum(0xFF << (8 * i) for i in range(4) if (cmask4 >> i) & 1)
    color_read, color_write = cmask4 != 0xF, cmask4 != 0

    # ---- read: an unread destination counts as 0 ----
    ds_read = depth_on or stencil_on
    dst_z = dst_z_mem if ds_read else np.zeros(shape, np.int64)
    dst_cw = dst_c_mem if (color_write and (color_read or blend_on)) else np.zeros(shape, np.int64)

    # ---- depth / stencil test ----
    passed = np.ones(shape, bool)
    new_z = np.zeros(shape, np.int64)
    if ds_read:
        depth_val, stencil_val = dst_z & DEPTH_MASK, dst_z >> DEPTH_BITS
        depth_ref = depth & DEPTH_MASK
        s_pass = _compare(s_func, np.broadcast_to(np.int64(s_ref & s_mask), shape),
                          stencil_val & s_mask)
        z_pass = _compare(depth_func, depth_ref, depth_val)
        passed = s_pass & z_pass
        res = np.where(s_pass,
                       np.where(z_pass, _stencil_op(s_zpass, s_ref, stencil_val),
                                _stencil_op(s_zfail, s_ref, stencil_val)),
                       _stencil_op(s_fail, s_ref, stencil_val))
        new_z = ((res << DEPTH_BITS) | depth_ref) & U32

    # ---- blend ----
    color = srcw
    if blend_on:
        src, dst, cst = _channels(srcw), _channels(dst_cw), _channels(dcr[BLEND_CONST])
        out = {}
        for ch in "argb":
            m, fs, fd = (mode_a, f_src_a, f_dst_a) if ch == "a" else (mode_rgb, f_src_rgb, f_dst_rgb)
            out[ch] = _mode(m, ch, _factor(fs, ch, src, dst, cst), _factor(fd, ch, src, dst, cst),
                            src, dst, srcw, dst_cw, dcr[LOGIC_OP], variant)
        color = (out["a"] << 24) | (out["r"] << 16) | (out["g"] << 8) | out["b"]

    # ---- write ----
    z_wm = np.where(passed & bool(depth_on and depth_wm), DEPTH_MASK, 0).astype(np.int64)
    if stencil_on:
        z_wm = z_wm | ((s_wm << DEPTH_BITS) & U32)
    out_z = np.where(z_wm != 0, (dst_z & ~z_wm) | (new_z & z_wm), dst_z_mem)
    if color_write:
        out_c = np.where(passed, (dst_cw & ~cmask) | (color & cmask), dst_c_mem)
    else:
        out_c = dst_c_mem
    return (out_c & U32).astype(np.uint32), (out_z & U32).astype(np.uint32)
