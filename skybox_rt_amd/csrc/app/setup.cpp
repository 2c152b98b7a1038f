// setup.cpp -- see setup.h.  Compiled with -ffp-contract=off: the float
// operation order below is part of the bit-exact contract with the reference
// (every product is rounded before it is added, as on the reference's x86
// host build without FMA).
#include "setup.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rt {
namespace {

// cocogfx TFixed<F>(float) on the host: truncation toward zero; x86
// cvttss2si yields INT_MIN for values out of range.
int32_t FixedHost(float f, int frac) {
  const float x = f * (float)(1u << frac);
  if (!(x >= -2147483648.0f && x < 2147483648.0f)) return INT32_MIN;
  return (int32_t)x;
}

// cocogfx ClipToHDC / ClipToScreen with viewport (0, W, 0, H, near, far):
// framebuffer row 0 is NDC y = -1 (draw3d/main.cpp:385-386).
struct Viewport {
  float sx, cx, sy, cy, sz, cz;
};
Viewport MakeViewport(uint32_t w, uint32_t h, float n, float f) {
  const float l = 0.0f, r = (float)w, t = 0.0f, b = (float)h;
  return {(r - l) * 0.5f, (r + l) * 0.5f, (b - t) * 0.5f, (b + t) * 0.5f,
          (f - n) * 0.5f, (f + n) * 0.5f};
}

}  // namespace

uint32_t ToVXCompare(int32_t c) {  // gfxutil.cpp:296-311
  static const uint32_t m[8] = {VX_OM_DEPTH_FUNC_NEVER,    VX_OM_DEPTH_FUNC_LESS,
                                VX_OM_DEPTH_FUNC_EQUAL,    VX_OM_DEPTH_FUNC_LEQUAL,
                                VX_OM_DEPTH_FUNC_GREATER,  VX_OM_DEPTH_FUNC_NOTEQUAL,
                                VX_OM_DEPTH_FUNC_GEQUAL,   VX_OM_DEPTH_FUNC_ALWAYS};
  return (c >= 0 && c < 8) ? m[c] : VX_OM_DEPTH_FUNC_ALWAYS;
}

int32_t ToVXFormat(int32_t f) {  // gfxutil.cpp:280-294
  switch (f) {
  case 1: return VX_TEX_FORMAT_A8;
  case 2: return VX_TEX_FORMAT_L8;
  case 3: return VX_TEX_FORMAT_A8L8;
  case 4: return VX_TEX_FORMAT_R5G6B5;
  default: return VX_TEX_FORMAT_A8R8G8B8;  // 5 in the traces: 4 bytes per texel
  }
}

uint32_t FormatStride(int32_t vx_format) {
  switch (vx_format) {
  case VX_TEX_FORMAT_A8R8G8B8: return 4;
  case VX_TEX_FORMAT_L8:
  case VX_TEX_FORMAT_A8: return 1;
  default: return 2;
  }
}

int PrimSetup(const std::array<Vertex, 3>& v, uint32_t width, uint32_t height, float znear,
              float zfar, rt_prim_t* out) {
  std::memset(out, 0, sizeof(*out));
  const Viewport vp = MakeViewport(width, height, znear, zfar);
  float hx[3], hy[3], hw[3], sz[3];
  for (int i = 0; i < 3; ++i) {
    const float* p = v[i].pos;
    hx[i] = p[0] * vp.sx + p[3] * vp.cx;  // HDC = screen position * w
    hy[i] = p[1] * vp.sy + p[3] * vp.cy;
    hw[i] = p[3];
    const float rhw = 1.0f / p[3];
    sz[i] = (p[2] * rhw) * vp.sz + vp.cz;  // screen z
  }
  // EdgeEquation (gfxutil.cpp:35-75): e_i = q_j x q_k over (x, y, w)
  float e[3][3];
  for (int i = 0; i < 3; ++i) {
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    e[i][0] = (hy[j] * hw[k]) - (hy[k] * hw[j]);
    e[i][1] = (hx[k] * hw[j]) - (hx[j] * hw[k]);
    e[i][2] = (hx[j] * hy[k]) - (hx[k] * hy[j]);
  }
  const float det = e[0][2] * hw[0] + e[1][2] * hw[1] + e[2][2] * hw[2];
  if (det < 0)
    for (auto& row : e)
      for (float& x : row) x *= -1.0f;
  if (det == 0) return kSetupDegenerate;
  for (auto& row : e) row[2] += row[0] * 0.5f + row[1] * 0.5f;  // half-pixel offset
  // EdgeToFixed (gfxutil.cpp:79-96)
  float m = std::fabs(e[0][0]);
  const float c[5] = {std::fabs(e[1][0]), std::fabs(e[2][0]), std::fabs(e[0][1]),
                      std::fabs(e[1][1]), std::fabs(e[2][1])};
  for (float x : c) m = (x > m) ? x : m;
  const float scale = 1.0f / m;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) out->edges[i][j] = FixedHost(e[i][j] * scale, 16);
  // ATTRIBUTE_DELTA (gfxutil.cpp:204-207,224-230): z from screen z, rest raw
  float a[7][3];
  for (int i = 0; i < 3; ++i) {
    a[0][i] = sz[i];
    for (int k = 0; k < 4; ++k) a[1 + k][i] = v[i].color[k];
    a[5][i] = v[i].uv[0];
    a[6][i] = v[i].uv[1];
  }
  for (int k = 0; k < 7; ++k) {
    out->attribs[k][0] = FixedHost(a[k][0] - a[k][2], 24);
    out->attribs[k][1] = FixedHost(a[k][1] - a[k][2], 24);
    out->attribs[k][2] = FixedHost(a[k][2], 24);
  }
  return kSetupOk;
}

rt_dcstate_t DrawcallState(const DrawCall& dc, const Scene& scene) {
  rt_dcstate_t s;
  std::memset(&s, 0, sizeof(s));
  const States& st = dc.states;
  // kernel_arg flags (draw3d/main.cpp:336-344)
  bool depth = st.depth_test != 0, color = st.color_enabled != 0, tex = st.texture_enabled != 0;
  bool modulate = tex && st.texture_envmode == kCglEnvModeModulate;
  if (modulate && !color) modulate = false;
  if (tex && color && !modulate) color = false;
  auto it = scene.textures.find(dc.texture_id);
  if (tex && it == scene.textures.end()) tex = false;
  if (tex) {
    const Texture& t = it->second;
    uint32_t lw = 0, lh = 0;
    while ((1u << lw) < (uint32_t)t.width) ++lw;
    while ((1u << lh) < (uint32_t)t.height) ++lh;
    s.tex_logw = lw;
    s.tex_logh = lh;
    s.tex_format = (uint32_t)ToVXFormat(t.format);
    s.tex_stride = FormatStride((int32_t)s.tex_format);
    // quirks kept: magfilter tested twice, wrapV from addressU (main.cpp:304-308)
    s.tex_filter = (st.texture_magfilter != kCglFilterNearest) ? VX_TEX_FILTER_BILINEAR
                                                              : VX_TEX_FILTER_POINT;
    s.tex_wrapu = (st.texture_addressU == kCglAddressWrap) ? VX_TEX_WRAP_REPEAT : VX_TEX_WRAP_CLAMP;
    s.tex_wrapv = s.tex_wrapu;
  }
  s.flags = (depth ? RT_DC_DEPTH : 0u) | (color ? RT_DC_COLOR : 0u) | (tex ? RT_DC_TEX : 0u) |
            (modulate ? RT_DC_MODULATE : 0u);
  return s;
}

int PrimBBox(const std::array<Vertex, 3>& v, uint32_t width, uint32_t height, rt_bbox_t* out) {
  const Viewport vp = MakeViewport(width, height, 0.0f, 1.0f);
  float l = 0, r = 0, t = 0, b = 0;
  for (int i = 0; i < 3; ++i) {  // ClipToScreen x, y (oracle clip_to_screen)
    const float* p = v[i].pos;
    const float rhw = 1.0f / p[3];
    const float x = (p[0] * rhw) * vp.sx + vp.cx, y = (p[1] * rhw) * vp.sy + vp.cy;
    if (i == 0) {
      l = r = x;
      t = b = y;
    } else {
      l = std::fmin(l, x); r = std::fmax(r, x);
      t = std::fmin(t, y); b = std::fmax(b, y);
    }
  }
  int32_t L = (int32_t)std::floor(l), R = (int32_t)std::ceil(r);
  int32_t T = (int32_t)std::floor(t), B = (int32_t)std::ceil(b);
  L = L > 0 ? L : 0;
  R = R < (int32_t)width ? R : (int32_t)width;
  T = T > 0 ? T : 0;
  B = B < (int32_t)height ? B : (int32_t)height;
  if (R <= L || B <= T) {
    out->x = out->y = 0;
    return kSetupCulled;
  }
  out->x = (uint32_t)L | ((uint32_t)R << 16);
  out->y = (uint32_t)T | ((uint32_t)B << 16);
  return kSetupOk;
}

namespace {
uint32_t ToVXStencilOp(int32_t c) {  // gfxutil.cpp:313-326
  static const uint32_t m[6] = {VX_OM_STENCIL_OP_KEEP, VX_OM_STENCIL_OP_REPLACE,
                                VX_OM_STENCIL_OP_INCR, VX_OM_STENCIL_OP_DECR,
                                VX_OM_STENCIL_OP_ZERO, VX_OM_STENCIL_OP_INVERT};
  return (c >= 0 && c < 6) ? m[c] : VX_OM_STENCIL_OP_KEEP;
}
uint32_t ToVXBlend(int32_t c) {  // gfxutil.cpp:328-346
  static const uint32_t m[11] = {VX_OM_BLEND_FUNC_ZERO, VX_OM_BLEND_FUNC_ONE,
                                 VX_OM_BLEND_FUNC_SRC_RGB, VX_OM_BLEND_FUNC_ONE_MINUS_SRC_RGB,
                                 VX_OM_BLEND_FUNC_SRC_A, VX_OM_BLEND_FUNC_ONE_MINUS_SRC_A,
                                 VX_OM_BLEND_FUNC_DST_A, VX_OM_BLEND_FUNC_ONE_MINUS_DST_A,
                                 VX_OM_BLEND_FUNC_DST_RGB, VX_OM_BLEND_FUNC_ONE_MINUS_DST_RGB,
                                 VX_OM_BLEND_FUNC_ALPHA_SAT};
  return (c >= 0 && c < 11) ? m[c] : VX_OM_BLEND_FUNC_ONE;
}
}  // namespace

rt_omstate_t OmState(const DrawCall& dc) {
  // draw3d/main.cpp:223-284 DCR writes, then DepthTencil / Blender configure
  // (graphics.cpp:534-620) and OutputMerger::configure (gpu_sw.h:78-98)
  rt_omstate_t s;
  std::memset(&s, 0, sizeof(s));
  const States& st = dc.states;
  uint32_t depth_func = VX_OM_DEPTH_FUNC_ALWAYS, depth_wm = 0;
  if (st.depth_test) {
    depth_func = ToVXCompare(st.depth_func);
    depth_wm = (uint32_t)st.depth_writemask & 1u;
  }
  uint32_t sf = VX_OM_DEPTH_FUNC_ALWAYS, szp = VX_OM_STENCIL_OP_KEEP, szf = 0;
  uint32_t sfail = VX_OM_STENCIL_OP_KEEP, sref = 0, smask = VX_OM_STENCIL_MASK, swm = 0;
  if (st.stencil_test) {
    sf = ToVXCompare(st.stencil_func);
    szp = ToVXStencilOp(st.stencil_zfail);  // quirk: ZPASS written twice, ZFAIL never (:251-260)
    szf = 0;
    sfail = ToVXStencilOp(st.stencil_fail);
    sref = (uint32_t)st.stencil_ref;
    smask = (uint32_t)st.stencil_mask;
    swm = (uint32_t)st.stencil_writemask;
  }
  uint32_t blend_func = (VX_OM_BLEND_FUNC_ZERO << 24) | (VX_OM_BLEND_FUNC_ZERO << 16) |
                        (VX_OM_BLEND_FUNC_ONE << 8) | VX_OM_BLEND_FUNC_ONE;
  if (st.blend_enabled) {
    const uint32_t bs = ToVXBlend(st.blend_src), bd = ToVXBlend(st.blend_dst);
    blend_func = (bd << 24) | (bd << 16) | (bs << 8) | bs;
  }
  s.depth_func = depth_func;
  s.depth_writemask = depth_wm;
  s.depth_test_on = !((depth_func == VX_OM_DEPTH_FUNC_ALWAYS) && !depth_wm);
  s.stencil_func = sf & 0xffff;
  s.stencil_zpass = szp & 0xffff;
  s.stencil_zfail = szf & 0xffff;
  s.stencil_fail = sfail & 0xffff;
  s.stencil_ref = sref & 0xffff;
  s.stencil_mask = smask & 0xffff;
  s.stencil_writemask = swm & 0xffff;
  s.stencil_on = !((s.stencil_func == VX_OM_DEPTH_FUNC_ALWAYS) &&
                   (s.stencil_zpass == VX_OM_STENCIL_OP_KEEP) &&
                   (s.stencil_zfail == VX_OM_STENCIL_OP_KEEP));
  s.blend_mode_rgb = VX_OM_BLEND_MODE_ADD;
  s.blend_mode_a = VX_OM_BLEND_MODE_ADD;
  s.blend_src_rgb = blend_func & 0xff;
  s.blend_src_a = (blend_func >> 8) & 0xff;
  s.blend_dst_rgb = (blend_func >> 16) & 0xff;
  s.blend_dst_a = (blend_func >> 24) & 0xff;
  s.blend_const = 0;
  s.logic_op = 0;
  s.blend_on = !((s.blend_src_rgb == VX_OM_BLEND_FUNC_ONE) && (s.blend_src_a == VX_OM_BLEND_FUNC_ONE) &&
                 (s.blend_dst_rgb == VX_OM_BLEND_FUNC_ZERO) && (s.blend_dst_a == VX_OM_BLEND_FUNC_ZERO));
  const uint32_t wm = st.color_writemask & 0xf;
  s.cbuf_writemask = ((wm >> 0) & 1) * 0x000000ffu | ((wm >> 1) & 1) * 0x0000ff00u |
                     ((wm >> 2) & 1) * 0x00ff0000u | ((wm >> 3) & 1) * 0xff000000u;
  s.color_read = wm != 0xf;
  s.color_write = wm != 0x0;
  s.prim_offset = dc.prim_offset;
  s.prim_count = dc.prim_count;
  return s;
}

std::vector<rt_cdesc_t> ChunkDescs(uint32_t width, uint32_t tiles_x, uint32_t shard_index,
                                   uint32_t shard_count, bool compact, uint32_t pos0,
                                   uint32_t local_tiles, const uint32_t* order, const uint32_t* bidx) {
  std::vector<rt_cdesc_t> out;
  for (uint32_t pos = pos0; pos < local_tiles; ++pos) {
    const uint32_t lt = order ? order[pos] : pos;
    const uint32_t gt = shard_index + lt * shard_count;
    const uint32_t tx = gt % tiles_x, ty = gt / tiles_x;
    for (uint32_t blk = 0; blk < 16; ++blk) {
      const uint32_t x0 = tx * 32u + (blk & 3u) * 8u, y0 = ty * 32u + (blk >> 2) * 8u;
      rt_cdesc_t d;
      d.origin = x0 | (y0 << 16);
      d.out = compact ? (lt << 10) | ((y0 & 31u) << 5) | (x0 & 31u) : y0 * width + x0;
      d.first = bidx ? bidx[2 * (lt * 16u + blk)] : 0u;
      d.count = (bidx ? bidx[2 * (lt * 16u + blk) + 1] : 0u) | ((compact ? 32u : width) << 16);
      out.push_back(d);
    }
  }
  return out;
}

std::vector<rt_bglayer_t> BgLayers(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t local_tiles,
                                   const uint32_t* order, uint32_t first_chunk, const rt_vtri_t* layers,
                                   uint32_t num_layers, const rt_prim_t* prims, uint32_t num_prims) {
  std::vector<rt_bglayer_t> out;
  for (uint32_t c = first_chunk; c < local_tiles * 16u; ++c) {
    const uint32_t gt = order ? order[c >> 4] : c >> 4, blk = c & 15u;
    const uint32_t x0 = (gt % tiles_x) * 32u + (blk & 3u) * 8u, y0 = (gt / tiles_x) * 32u + (blk >> 2) * 8u;
    rt_bglayer_t d{0u, 0u};
    if (x0 + 8u <= width && y0 + 8u <= height) {
      int32_t top[64];
      for (int32_t& t : top) t = -1;
      for (uint32_t k = num_layers; k-- > 0;)  // drawing order: the later layer overwrites
        for (uint32_t p = 0; p < 64u; ++p)
          if (rt_layer_covers(layers[k].edges, layers[k].rx, layers[k].ry, x0 + (p & 7u), y0 + (p >> 3)))
            top[p] = layers[k].pid;
      bool same = true;
      for (uint32_t p = 1; p < 64u; ++p) same = same && top[p] == top[0];
      if (same && top[0] < 0) {
        d.pid1 = RT_BGLAYER_NONE;
      } else if (same && (uint32_t)top[0] < num_prims) {
        d.pid1 = (uint32_t)top[0] + 1u;
        d.dc = prims[top[0]].dc;
      }
    }
    out.push_back(d);
  }
  return out;
}

namespace {
// gfx_device.h fx_from_float_dev / fx_to_float / interp and rt_trace.h vis_depth on the host: the
// shader's depth word from the three edge values (fp32, no contraction, IEEE division)
int32_t FxFromFloatDev(float f, int frac) {
  const float x = f * (float)(1u << frac);
  if (x != x || x >= 2147483648.0f) return INT32_MAX;  // fcvt.w.s: NaN and overflow saturate high
  if (x <= -2147483648.0f) return INT32_MIN;
  return (int32_t)x;
}
int32_t Imadd24(int32_t a, int32_t b, int32_t c) {
  const int32_t p = (int32_t)(((int64_t)a * (int64_t)b) >> 24);
  return (int32_t)((uint32_t)p + (uint32_t)c);
}
uint32_t VisDepth(int32_t E0, int32_t E1, int32_t E2, const int32_t z[3]) {
  const float k = 1.0f / (float)(1u << 24);
  const float f0 = (float)E0 * k, f1 = (float)E1 * k, f2 = (float)E2 * k;
  const float r = 1.0f / (f0 + f1 + f2);
  const int32_t dx = FxFromFloatDev(r * f0, 24), dy = FxFromFloatDev(r * f1, 24);
  return (uint32_t)Imadd24(z[1], dy, Imadd24(z[0], dx, z[2])) & VX_OM_DEPTH_MASK;
}
int32_t EdgeEval(const int32_t* e, uint32_t x, uint32_t y) {
  return (int32_t)((uint32_t)e[0] * x + (uint32_t)e[1] * y + (uint32_t)e[2]);
}
bool RectIn(uint32_t r, uint32_t p) { return p >= (r & 0xffffu) && p <= (r >> 16); }
}  // namespace

void TrimBlockLists(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t shard_index,
                    uint32_t shard_count, uint32_t local_tiles, bool tie_high, const uint32_t* bidx,
                    const rt_bentry_t* blist, uint64_t entries, const rt_vtri_t* vgeom,
                    std::vector<uint32_t>* btidx, std::vector<rt_bentry_t>* btrim, uint64_t* kept,
                    uint32_t* blocks) {
  btrim->assign(blist, blist + entries + RT_BLIST_PAD);
  btidx->assign(2 * (size_t)local_tiles * 16u, 0u);
  *kept = 0;
  *blocks = 0;
  std::vector<uint8_t> wins;
  for (uint32_t lb = 0; lb < local_tiles * 16u; ++lb) {
    const uint32_t first = bidx[2 * lb], count = bidx[2 * lb + 1];
    const uint32_t gt = shard_index + (lb >> 4) * shard_count, blk = lb & 15u;
    const uint32_t x0 = (gt % tiles_x) * 32u + (blk & 3u) * 8u, y0 = (gt / tiles_x) * 32u + (blk >> 2) * 8u;
    wins.assign(count, 0);
    for (uint32_t p = 0; p < 64u; ++p) {
      const uint32_t px = x0 + (p & 7u), py = y0 + (p >> 3);
      if (px >= width || py >= height) continue;  // edge tiles overhang the image
      // rt_trace.h vis_test over the whole list; (bz, bpid) start at the cleared depth buffer
      uint32_t bz = VX_OM_DEPTH_MASK;
      int32_t bpid = -1, best = -1;
      for (uint32_t i = 0; i < count; ++i) {
        const rt_vtri_t& t = vgeom[blist[first + i].k];
        if (!RectIn(t.rx, px) || !RectIn(t.ry, py) || t.zmin > bz) continue;
        const int32_t E0 = EdgeEval(t.edges, px, py), E1 = EdgeEval(t.edges + 3, px, py),
                      E2 = EdgeEval(t.edges + 6, px, py);
        if (E0 < 0 || E1 < 0 || E2 < 0) continue;
        const uint32_t z = VisDepth(E0, E1, E2, t.z);
        if (z < bz || (z == bz && (tie_high ? t.pid > bpid : (bpid >= 0 && t.pid < bpid)))) {
          bz = z;
          bpid = t.pid;
          best = (int32_t)i;
        }
      }
      if (best >= 0) wins[best] = 1;
    }
    uint32_t n = 0;
    for (uint32_t i = 0; i < count; ++i)
      if (wins[i]) (*btrim)[first + n++] = blist[first + i];
    (*btidx)[2 * lb] = first;
    (*btidx)[2 * lb + 1] = n;
    *kept += n;
    *blocks += n ? 1u : 0u;
  }
}

}  // namespace rt
