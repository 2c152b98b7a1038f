"""Hand-worked known answers of the texture sampler, with the arithmetic
written out.  Worked from the meaning of the operations (coordinates are
fixed point with 23 fraction bits, ONE = 2^23 = 0x800000 is the texture's
side; sim/common/graphics.cpp:35-314 and tests/regression/tex/kernel.cpp are
the definition), not from any implementation's output: tests/tex_reference.py,
the oracle and the device all have to reproduce them.

lerp(a, b, f) = (p + (p >> 8)) >> 8 with p = a (255 - f) + b f + 128;
lerp(a, a, f) = a for every a and f (p = 255 a + 128).

WRAPS: (name, mode, coordinate, wrapped coordinate).
SAMPLES: (name, texture bytes, mipoff of the levels present, logw, logh,
format, filter, wrapu, wrapv, u, v, lod, frac, colour a<<24|r<<16|g<<8|b).
Filter 0 point, 1 bilinear (both at `lod`), 2 the blend of the bilinear
samples at `lod` and the next level by `frac`.
LODS: (name, logw, logh, dst width, dst height, lod, frac).
"""
from tex_reference import (A1R5G5B5, A4R4G4B4, A8, A8L8, A8R8G8B8, BILINEAR, CLAMP, INT32_MAX,
                           INT32_MIN, L8, MIRROR, ONE, POINT, R5G6B5, REPEAT, TRILINEAR)

# ---- wrap modes ---------------------------------------------------------------
# CLAMP is min(max(d, 0), ONE - 1); REPEAT the floor modulus; MIRROR reflects
# the odd periods: d = per * ONE + fr, fr in [0, ONE), and the result is
# ONE - 1 - fr when per is odd.
#   -1       = -1 * ONE + (ONE - 1)      per -1 (odd),  fr ONE - 1
#   ONE      =  1 * ONE + 0              per  1 (odd),  fr 0
#   ONE + 1  =  1 * ONE + 1              per  1 (odd),  fr 1
#   2 ONE - 1 = 1 * ONE + (ONE - 1)      per  1 (odd),  fr ONE - 1
#   -ONE - 1 = -2 * ONE + (ONE - 1)      per -2 (even), fr ONE - 1
WRAPS = [
    ("clamp_m1", CLAMP, -1, 0),                       # below 0
    ("clamp_one", CLAMP, ONE, ONE - 1),               # at and above ONE: the last coordinate
    ("clamp_one_p1", CLAMP, ONE + 1, ONE - 1),
    ("clamp_2one_m1", CLAMP, 2 * ONE - 1, ONE - 1),
    ("clamp_mone_m1", CLAMP, -ONE - 1, 0),
    ("repeat_m1", REPEAT, -1, ONE - 1),               # fr of the table above
    ("repeat_one", REPEAT, ONE, 0),
    ("repeat_one_p1", REPEAT, ONE + 1, 1),
    ("repeat_2one_m1", REPEAT, 2 * ONE - 1, ONE - 1),
    ("repeat_mone_m1", REPEAT, -ONE - 1, ONE - 1),
    ("mirror_m1", MIRROR, -1, 0),                     # odd:  ONE - 1 - (ONE - 1)
    ("mirror_one", MIRROR, ONE, ONE - 1),             # odd:  ONE - 1 - 0
    ("mirror_one_p1", MIRROR, ONE + 1, ONE - 2),      # odd:  ONE - 1 - 1
    ("mirror_2one_m1", MIRROR, 2 * ONE - 1, 0),       # odd:  ONE - 1 - (ONE - 1)
    ("mirror_mone_m1", MIRROR, -ONE - 1, ONE - 1),    # even: fr
]

_NOMIP = (0,)
# an 8x1 L8 ramp: texel x holds 0x11 x, so a point sample names its column:
# x = wrapped * 8 >> 23, colour 0xFF then 0x11 x in each of r, g, b
_RAMP8 = (0x00, 0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77)
# a 4x1 L8 row for the bilinear entries; one texel T = ONE / 4 = 0x200000,
# half a texel 0x100000.  Its height is 1: v = ONE / 2 gives v0 = 0 (y0 = 0,
# beta = 0) and every wrap of v1 = ONE lands in row 0 again.
_ROW4 = (10, 50, 90, 200)


def _point_on_ramp(name, mode, d, wrapped):
    """the wrap entry seen through a point sample of the ramp (v = 0, CLAMP):
    column wrapped * 8 >> 23 is 0 for wrapped < 0x100000 and 7 from 0x700000"""
    x = {0: 0, 1: 0, ONE - 2: 7, ONE - 1: 7}[wrapped]
    L = _RAMP8[x]
    return ("point_" + name, _RAMP8, _NOMIP, 3, 0, L8, POINT, mode, CLAMP, d, 0, 0, 0,
            0xFF000000 | (L << 16) | (L << 8) | L)


SAMPLES = [_point_on_ramp(*w) for w in WRAPS] + [
    # ---- one texel per format, decoded (1x1 texture, point filter) ----
    # A8R8G8B8: bytes 78 56 34 12 little-endian = 0x12345678, stored as is
    ("decode_a8r8g8b8", (0x78, 0x56, 0x34, 0x12), _NOMIP, 0, 0, A8R8G8B8, POINT, CLAMP, CLAMP, 0, 0,
     0, 0, 0x12345678),
    # R5G6B5: 0xB4A9 = 10110 100101 01001: r = 10110, g = 100101 (6 bits), b = 01001
    #   r: 10110 101 = 0xB5   g: 100101 10 = 0x96   b: 01001 010 = 0x4A   a: none = 0xFF
    ("decode_r5g6b5", (0xA9, 0xB4), _NOMIP, 0, 0, R5G6B5, POINT, CLAMP, CLAMP, 0, 0, 0, 0,
     0xFFB5964A),
    # A1R5G5B5: 0x9F11 = 1 00111 11000 10001: a = 1 -> 0xFF
    #   r: 00111 001 = 0x39   g: 11000 110 = 0xC6   b: 10001 100 = 0x8C
    ("decode_a1r5g5b5_a1", (0x11, 0x9F), _NOMIP, 0, 0, A1R5G5B5, POINT, CLAMP, CLAMP, 0, 0, 0, 0,
     0xFF39C68C),
    # the same colour fields with a = 0: 0x1F11 -> alpha 0x00
    ("decode_a1r5g5b5_a0", (0x11, 0x1F), _NOMIP, 0, 0, A1R5G5B5, POINT, CLAMP, CLAMP, 0, 0, 0, 0,
     0x0039C68C),
    # A4R4G4B4: 0xA3C5: every nibble doubled
    ("decode_a4r4g4b4", (0xC5, 0xA3), _NOMIP, 0, 0, A4R4G4B4, POINT, CLAMP, CLAMP, 0, 0, 0, 0,
     0xAA33CC55),
    # A8L8: 0x9D42: a = 0x9D, r = g = b = 0x42
    ("decode_a8l8", (0x42, 0x9D), _NOMIP, 0, 0, A8L8, POINT, CLAMP, CLAMP, 0, 0, 0, 0, 0x9D424242),
    # L8: r = g = b = 0x6B, no alpha = 0xFF;  A8: a = 0x6B, no colour = 0xFFFFFF
    ("decode_l8", (0x6B,), _NOMIP, 0, 0, L8, POINT, CLAMP, CLAMP, 0, 0, 0, 0, 0xFF6B6B6B),
    ("decode_a8", (0x6B,), _NOMIP, 0, 0, A8, POINT, CLAMP, CLAMP, 0, 0, 0, 0, 0x6BFFFFFF),

    # ---- bilinear ----
    # exactly on the centre of texel 1: u = 1.5 T = 0x300000
    #   u0 = 0x200000: x0 = 0x200000 * 4 >> 23 = 1, alpha = (0x200000 * 1024 >> 23) & 255 = 256 & 255 = 0
    #   u1 = 0x400000: x1 = 2;  lerp(50, 90, 0): p = 12750 + 128 = 12878, 12878 >> 8 = 50,
    #   (12878 + 50) >> 8 = 50;  alpha channel lerp(255, 255, 0): p = 65153, >> 8 = 254,
    #   (65153 + 254) >> 8 = 255
    ("bilinear_centre", _ROW4, _NOMIP, 2, 0, L8, BILINEAR, CLAMP, CLAMP, 0x300000, ONE // 2, 0, 0,
     0xFF323232),
    # alpha = 128 between 0 and 255: a 2x1 texture (0, 255), T = 0x400000, half 0x200000
    #   u = 0x400000: u0 = 0x200000: x0 = 0x200000 * 2 >> 23 = 0,
    #   alpha = (0x200000 * 512 >> 23) & 255 = 128;  u1 = 0x600000: x1 = 0xC00000 >> 23 = 1
    #   lerp(0, 255, 128): p = 0 * 127 + 255 * 128 + 128 = 32768; 32768 >> 8 = 128;
    #   (32768 + 128) >> 8 = 128 -> 0x80   (without the + 128: 32640 -> 127)
    ("bilinear_half", (0, 255), _NOMIP, 1, 0, L8, BILINEAR, CLAMP, CLAMP, 0x400000, ONE // 2, 0, 0,
     0xFF808080),
    # the right edge, u = 3.75 T = 0x780000 on the 4x1 row:
    #   u0 = 0x680000: x0 = 0x1A00000 >> 23 = 3, alpha = (0x680000 >> 13) & 255 = 0x340 & 255 = 64
    #   u1 = 0x880000 is past ONE:
    #   CLAMP:  ONE - 1 -> x1 = 3: lerp(200, 200, 64) = 200 = 0xC8
    #   REPEAT: 0x080000 -> x1 = 0x200000 >> 23 = 0: lerp(200, 10, 64):
    #           p = 200 * 191 + 10 * 64 + 128 = 38968; >> 8 = 152; (38968 + 152) >> 8 = 152 = 0x98
    #   MIRROR: period 1 (odd), fr 0x080000 -> 0x77FFFF -> x1 = 0x1DFFFFC >> 23 = 3: 200 = 0xC8
    ("bilinear_edge_clamp", _ROW4, _NOMIP, 2, 0, L8, BILINEAR, CLAMP, CLAMP, 0x780000, ONE // 2, 0,
     0, 0xFFC8C8C8),
    ("bilinear_edge_repeat", _ROW4, _NOMIP, 2, 0, L8, BILINEAR, REPEAT, REPEAT, 0x780000, ONE // 2,
     0, 0, 0xFF989898),
    ("bilinear_edge_mirror", _ROW4, _NOMIP, 2, 0, L8, BILINEAR, MIRROR, MIRROR, 0x780000, ONE // 2,
     0, 0, 0xFFC8C8C8),
    # a 1x1 level: all four taps are the one texel whatever the coordinates,
    # and lerp(a, a, f) = a
    ("bilinear_1x1", (0x78, 0x56, 0x34, 0x12), _NOMIP, 0, 0, A8R8G8B8, BILINEAR, REPEAT, MIRROR,
     0x123456, -5, 0, 0, 0x12345678),

    # ---- the int32 extremes under bilinear REPEAT (4x1 row, half texel 0x100000;
    #      v = 0: v0 = -0x400000 mod ONE = 0x400000, beta = 128, both rows are row 0) ----
    # u = INT32_MAX = 0x7FFFFFFF: u0 = 0x7FEFFFFF, mod ONE = 0x6FFFFF: x0 = 0x1BFFFFC >> 23 = 3,
    #   alpha = (0x6FFFFF >> 13) & 255 = 0x37F & 255 = 127
    #   u1 = 0x7FFFFFFF + 0x100000 wraps to the bit pattern 0x800FFFFF (negative); its
    #   floor modulus is its low 23 bits 0x0FFFFF: x1 = 0x3FFFFC >> 23 = 0
    #   lerp(200, 10, 127): p = 200 * 128 + 10 * 127 + 128 = 26998; >> 8 = 105;
    #   (26998 + 105) >> 8 = 105 = 0x69;  lerp(105, 105, 128) = 105
    ("bilinear_int32_max", _ROW4, _NOMIP, 2, 0, L8, BILINEAR, REPEAT, REPEAT, INT32_MAX, 0, 0, 0,
     0xFF696969),
    # u = INT32_MIN: u0 = -0x80000000 - 0x100000 wraps to 0x7FF00000, mod ONE = 0x700000:
    #   x0 = 0x1C00000 >> 23 = 3, alpha = (0x700000 >> 13) & 255 = 0x380 & 255 = 128
    #   u1 = -0x7FF00000, bit pattern 0x80100000, low 23 bits 0x100000: x1 = 0x400000 >> 23 = 0
    #   lerp(200, 10, 128): p = 200 * 127 + 10 * 128 + 128 = 26808; >> 8 = 104;
    #   (26808 + 104) >> 8 = 26912 >> 8 = 105 = 0x69
    ("bilinear_int32_min", _ROW4, _NOMIP, 2, 0, L8, BILINEAR, REPEAT, REPEAT, INT32_MIN, 0, 0, 0,
     0xFF696969),

    # ---- trilinear: a 2x1 L8 texture (40, 100) with its chain.  Level 1 is the box
    #      of level 0 (a side of 1 stays at index 0: rows 0, 0): (40 + 100 + 40 + 100) >> 2
    #      = 70; bytes 40 100 | 70, mipoff 0, 2 ----
    # frac = 255 at lod 0, u = centre of texel 0 = 0x200000:
    #   level 0 (half texel 0x200000): u0 = 0: x0 = 0, alpha = 0 -> 40
    #   level 1 (1x1): 70;  lerp(40, 70, 255): p = 40 * 0 + 70 * 255 + 128 = 17978; >> 8 = 70;
    #   (17978 + 70) >> 8 = 70 = 0x46: frac 255 is exactly the next level
    ("trilinear_frac255", (40, 100, 70), (0, 2), 1, 0, L8, TRILINEAR, CLAMP, CLAMP, 0x200000,
     ONE // 2, 0, 255, 0xFF464646),
    # past the chain: lod 1 is the last level, its partner lod 2 has mipoff 0 (never
    # written) and 1x1 dims: it reads byte 0 = 40.  lerp(70, 40, 128):
    #   p = 70 * 127 + 40 * 128 + 128 = 14138; >> 8 = 55; (14138 + 55) >> 8 = 55 = 0x37
    ("trilinear_past_chain", (40, 100, 70), (0, 2), 1, 0, L8, TRILINEAR, CLAMP, CLAMP, 0x200000,
     ONE // 2, 1, 128, 0xFF373737),
]

# ---- lod and blend fraction of a destination size --------------------------------
# j = trunc(max(W / dw, H / dh, 1) * 65536) in float32, converted to a signed 32-bit
# word by a saturating conversion; lod = floor(log2 j) - 16; frac = (j - 2^(lod+16)) >> (lod+8)
LODS = [
    ("lod_unit", 4, 4, 16, 16, 0, 0),          # ratio 1: j = 65536 = 2^16
    # 16 / 12 in float32 = 1.33333337...; * 65536 = 87381.33...: j = 87381, 2^16 <= j < 2^17:
    # lod 0, frac = (87381 - 65536) >> 8 = 21845 >> 8 = 85
    ("lod_third", 4, 4, 12, 12, 0, 85),
    ("lod_quarter", 5, 3, 8, 8, 2, 0),         # max(32 / 8, 8 / 8) = 4: j = 2^18
    # the kernel's j is a signed 32-bit fixed-point word built from a float
    # (kernel.cpp:119, a fcvt.w.s on the reference's cores: it saturates).  A ratio
    # of 2^15 asks for j = 2^31, which saturates to 2^31 - 1: floor(log2) = 30, lod 14,
    # frac = (2^31 - 1 - 2^30) >> 22 = (2^30 - 1) >> 22 = 255.  So the lod clamp at 15
    # can never bind; a model without the saturation answers (15, 0) here.
    ("lod_sat", 15, 0, 1, 1, 14, 255),
]
