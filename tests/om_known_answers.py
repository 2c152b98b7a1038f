"""Hand-worked single-pixel known answers of the output merger, with the
arithmetic written out.  Worked from the unit's definition
(sim/common/graphics.cpp:320-636, sim/simx/om_unit.cpp:55-136), not from any
implementation's output; tests/om_reference.py, the oracle and the device all
have to reproduce them.

div255(x) = (x + (x >> 8)) >> 8; for x = 255 k + 128 it gives k.

An entry: (name, make_dcr keywords, backface, source colour, depth word,
colour before, depth/stencil before, colour after, depth/stencil after).
Depth/stencil words are stencil << 24 | depth.
"""
from om_reference import (ADD, ALWAYS, DECR, DECR_WRAP, EQUAL, F_ALPHA_SAT, F_ONE,
                          F_ONE_MINUS_CONST_A, F_ONE_MINUS_SRC_A, F_SRC_A, F_ZERO, GEQUAL, GREATER,
                          INCR, INCR_WRAP, INVERT, KEEP, LEQUAL, LESS, LOGICOP, MAX, MIN, NEVER,
                          NOTEQUAL, REPLACE, REV_SUB, SUB, ZERO)

_S, _D = 0x80C04010, 0x40208030     # the blend-mode entries' source and destination


def _ops(op, val, ref, exp):
    """stencil `op` in the zpass slot: EQUAL under mask 0x0F passes (val and
    ref share their low nibble), LESS passes (0x10 < 0x20); colour written,
    depth written, stencil = exp"""
    return (f"zpass_{op}_{val:02x}",
            dict(depth_func=LESS, depth_wm=1, stencil_func=(EQUAL, NEVER), zpass=(op, KEEP),
                 ref=(ref, 0), mask=(0x0F, 0), swm=(0xFF, 0)),
            False, 0x11223344, 0x000010, 0x55667788, (val << 24) | 0x000020,
            0x11223344, (exp << 24) | 0x000010)


def _tie(func, passes):
    """depth word 0xFF123456 against a stored 0x123456 (stencil byte 0xAB): the
    word's high byte is masked off, so the compare sees a tie.  A pass writes
    the colour and the (equal) depth; the stencil byte stays: stencil is off."""
    return (f"tie_{func}", dict(depth_func=func, depth_wm=1), False, 0x11223344, 0xFF123456,
            0x55667788, 0xAB123456, 0x11223344 if passes else 0x55667788, 0xAB123456)


KNOWN_ANSWERS = [
    # ---- blend modes ----
    # ADD, SRC_A / ONE_MINUS_SRC_A: src a=128 r=255 g=128 b=64, dst a=255 r=32 g=64 b=96;
    # factors 128 and 127 on every channel
    #   a: 128*128 + 255*127 + 128 = 48897; 48897 >> 8 = 191; (48897 + 191) >> 8 = 191 = 0xBF
    #   r: 255*128 +  32*127 + 128 = 36832; 36832 >> 8 = 143; (36832 + 143) >> 8 = 144 = 0x90
    #   g: 128*128 +  64*127 + 128 = 24640; 24640 >> 8 =  96; (24640 +  96) >> 8 =  96 = 0x60
    #   b:  64*128 +  96*127 + 128 = 20512; 20512 >> 8 =  80; (20512 +  80) >> 8 =  80 = 0x50
    ("add_src_alpha", dict(func=(F_SRC_A, F_SRC_A, F_ONE_MINUS_SRC_A, F_ONE_MINUS_SRC_A)),
     False, 0x80FF8040, 0, 0xFF204060, 0x12345678, 0xBF906050, 0x12345678),
    # ADD, ONE / ONE, the 0xFF00 clamp: src a=255 r=128 g=192 b=16, dst a=255 r=144 g=80 b=127
    #   a: 255*255 + 255*255 + 128 = 130178 -> 0xFF00 = 65280; (65280 + 255) >> 8 = 255
    #   r: (128 + 144) * 255 + 128 = 69488 -> 65280 -> 255
    #      (unclamped: 69488 >> 8 = 271; (69488 + 271) >> 8 = 272, kept byte 0x10)
    #   g: (192 + 80) * 255 + 128 = 69488 -> 255
    #   b: (16 + 127) * 255 + 128 = 36593; 36593 >> 8 = 142; (36593 + 142) >> 8 = 143 = 0x8F
    ("add_clamp", dict(func=(F_ONE, F_ONE, F_ONE, F_ONE)),
     False, 0xFF80C010, 0, 0xFF90507F, 0, 0xFFFFFF8F, 0),
    # SUB, ONE / ONE: src a=128 r=192 g=64 b=16, dst a=64 r=32 g=128 b=48
    #   a: (128 - 64) * 255 + 128 = 16448 -> 64 = 0x40
    #   r: (192 - 32) * 255 + 128 = 40928 -> 160 = 0xA0
    #   g: (64 - 128) * 255 + 128 < 0 -> 0;   b: (16 - 48) * 255 + 128 < 0 -> 0
    ("sub", dict(mode=(SUB, SUB), func=(F_ONE, F_ONE, F_ONE, F_ONE)),
     False, _S, 0, _D, 0, 0x40A00000, 0),
    # REV_SUB, same operands: a and r negative -> 0; g: (128 - 64) -> 0x40; b: (48 - 16) -> 0x20
    ("rev_sub", dict(mode=(REV_SUB, REV_SUB), func=(F_ONE, F_ONE, F_ONE, F_ONE)),
     False, _S, 0, _D, 0, 0x00004020, 0),
    # MIN / MAX ignore the (ZERO, ZERO) factors: per channel of 80 C0 40 10 and 40 20 80 30
    ("min", dict(mode=(MIN, MIN), func=(F_ZERO, F_ZERO, F_ZERO, F_ZERO)),
     False, _S, 0, _D, 0, 0x40204010, 0),
    ("max", dict(mode=(MAX, MAX), func=(F_ZERO, F_ZERO, F_ZERO, F_ZERO)),
     False, _S, 0, _D, 0, 0x80C08030, 0),
    # LOGICOP XOR on the packed words: 0x80C04010 ^ 0x40208030 = 0xC0E0C020
    ("logicop_xor", dict(mode=(LOGICOP, LOGICOP), logic_op=6), False, _S, 0, _D, 0, 0xC0E0C020, 0),
    # LOGICOP in the rgb half only, alpha ADD with ONE / ZERO: a = div255(128*255 + 128) = 0x80
    ("logicop_rgb_half", dict(mode=(LOGICOP, ADD), logic_op=6), False, _S, 0, _D, 0, 0x80E0C020, 0),
    # ---- factors ----
    # ONE_MINUS_CONST_A is per channel: const a=0x40 r=0x10 g=0x20 b=0x30 gives factors
    # BF EF DF CF (a true 1 - const alpha would be BF on all four); src all 255, dst factor
    # ZERO: channel = div255(255 * f + 128) = f
    ("one_minus_const_a", dict(func=(F_ONE_MINUS_CONST_A, F_ONE_MINUS_CONST_A, F_ZERO, F_ZERO),
                               const=0x40102030),
     False, 0xFFFFFFFF, 0, 0x01020304, 0, 0xBFEFDFCF, 0),
    # ALPHA_SAT: factor (0xFF, f, f, f), f = min(src a, 0xFF - dst a)
    #   src a=0x60=96, dst a=0xC0 -> f = min(96, 63) = 63: a = 96, rgb = div255(255*63 + 128) = 0x3F
    ("alpha_sat_dst_limits", dict(func=(F_ALPHA_SAT, F_ALPHA_SAT, F_ZERO, F_ZERO)),
     False, 0x60FFFFFF, 0, 0xC0000000, 0, 0x603F3F3F, 0),
    #   src a=0x20=32, dst a=0xC0 -> f = min(32, 63) = 32: a = 32, rgb = 0x20
    ("alpha_sat_src_limits", dict(func=(F_ALPHA_SAT, F_ALPHA_SAT, F_ZERO, F_ZERO)),
     False, 0x20FFFFFF, 0, 0xC0000000, 0, 0x20202020, 0),
    # ---- compare functions at a tie ----
    _tie(LESS, False), _tie(LEQUAL, True), _tie(EQUAL, True), _tie(NOTEQUAL, False),
    _tie(GEQUAL, True), _tie(GREATER, False), _tie(NEVER, False), _tie(ALWAYS, True),
    # LESS one below the stored depth: passes, depth written under the kept stencil byte
    ("less_passes", dict(depth_func=LESS, depth_wm=1), False, 0x11223344, 0xFF123455,
     0x55667788, 0xAB123456, 0x11223344, 0xAB123455),
    # ... and with the depth write mask off: colour only
    ("less_passes_no_depth_write", dict(depth_func=LESS, depth_wm=0), False, 0x11223344, 0x123455,
     0x55667788, 0xAB123456, 0x11223344, 0xAB123456),
    # ---- stencil operations (zpass slot) ----
    _ops(KEEP, 0xF1, 0x81, 0xF1), _ops(ZERO, 0xF1, 0x81, 0x00), _ops(REPLACE, 0xF1, 0x81, 0x81),
    _ops(INCR, 0xF1, 0x81, 0xF2), _ops(INCR, 0xFF, 0x8F, 0xFF),           # saturates
    _ops(DECR, 0xF1, 0x81, 0xF0), _ops(DECR, 0x00, 0x80, 0x00),           # saturates
    _ops(INVERT, 0xF1, 0x81, 0x0E),     # ~0xF1 = 0xFFFFFF0E, the high bits leave through << 24
    _ops(INCR_WRAP, 0xFF, 0x8F, 0x00), _ops(DECR_WRAP, 0x00, 0x80, 0xFF),
    # ---- the other two slots, write masks, the back face ----
    # zfail: stencil passes, LESS fails (0x30 > 0x20): INVERT applied, depth and colour kept
    ("zfail_invert", dict(depth_func=LESS, depth_wm=1, stencil_func=(EQUAL, NEVER),
                          zpass=(ZERO, KEEP), zfail=(INVERT, KEEP), fail=(REPLACE, KEEP),
                          ref=(0x81, 0), mask=(0x0F, 0), swm=(0xFF, 0)),
     False, 0x11223344, 0x000030, 0x55667788, 0xF1000020, 0x55667788, 0x0E000020),
    # fail: low nibbles differ (ref 0x82, val 0xF1): REPLACE applied though LESS would pass
    ("fail_replace", dict(depth_func=LESS, depth_wm=1, stencil_func=(EQUAL, NEVER),
                          zpass=(ZERO, KEEP), zfail=(INVERT, KEEP), fail=(REPLACE, KEEP),
                          ref=(0x82, 0), mask=(0x0F, 0), swm=(0xFF, 0)),
     False, 0x11223344, 0x000010, 0x55667788, 0xF1000020, 0x55667788, 0x82000020),
    # stencil write mask 0x0F: INVERT of 0xF6 = 0x09 lands in the low nibble only -> 0xF9
    ("stencil_writemask", dict(stencil_func=(ALWAYS, NEVER), zpass=(INVERT, KEEP), ref=(0, 0),
                               mask=(0xFF, 0), swm=(0x0F, 0)),
     False, 0x11223344, 0x000010, 0x55667788, 0xF6000020, 0x11223344, 0xF9000020),
    # back face: the high halves decide (GEQUAL: 0x40 >= 0x3F & 0x7F passes; zpass DECR_WRAP);
    # the front halves would fail (NEVER) and REPLACE
    ("back_face", dict(stencil_func=(NEVER, GEQUAL), zpass=(KEEP, DECR_WRAP), fail=(REPLACE, KEEP),
                       ref=(0x11, 0x40), mask=(0xFF, 0x7F), swm=(0x00, 0xFF)),
     True, 0x11223344, 0x000010, 0x55667788, 0x3F000020, 0x11223344, 0x3E000020),
    # GREATER on the stencil: ref & mask = 0x40 > val & mask = 0x3F passes, but depth GREATER
    # fails (0x10 < 0x20): zfail INCR, colour kept
    ("stencil_greater_depth_fails", dict(depth_func=GREATER, depth_wm=1,
                                         stencil_func=(GREATER, ALWAYS), zpass=(ZERO, KEEP),
                                         zfail=(INCR, KEEP), ref=(0x40, 0), mask=(0x7F, 0),
                                         swm=(0xFF, 0)),
     False, 0x11223344, 0x000010, 0x55667788, 0xBF000020, 0x55667788, 0xC0000020),
    # ---- colour mask ----
    # mask 0x5 (blue and red bytes), blending off: the destination is read and keeps a and g
    ("color_mask", dict(cmask=0x5), False, 0x11223344, 0, 0x55667788, 0xAB123456,
     0x55227744, 0xAB123456),
    # mask 0: nothing is written to colour; depth still is (LESS passes)
    ("color_mask_zero", dict(cmask=0x0, depth_func=LESS, depth_wm=1), False, 0x11223344, 0x000010,
     0x55667788, 0xAB000020, 0x55667788, 0xAB000010),
]
assert len({k[0] for k in KNOWN_ANSWERS}) == len(KNOWN_ANSWERS)
