// rt_common.h -- data layout shared by the RT host app and the HIP kernel.
//
// Everything the kernel reads lives in the driver's HBM arena and is addressed
// by the device addresses the app got from vx_mem_alloc (see DESIGN.md
// "Data layout in HBM"):
//   nodes   [num_nodes]  rt_node_t   64 B  BVH2 node = both children's boxes
//   tris    [num_tris]   rt_tri_t    48 B  clip-space v0,e1,e2 + pid (leaf order)
//   vnodes  [num nodes]  rt_vnode_t  64 B  primary visibility per traversed node
//   vtris   [num_tris]   rt_vtri_t   64 B  primary visibility per leaf record
//   vlayers [num_layer]  rt_vtri_t   64 B  screen layers, highest pid first
//   vgeom   [num_geom]   rt_vtri_t   64 B  geometry, ascending pid (flat mode)
//   prims   [num_prims]  rt_prim_t  128 B  fixed-point shading record
//   dcs     [num_dc]     rt_dcstate_t 64 B per-drawcall shading state
//   ptris   [num_prims]  rt_tri_t    48 B  clip-space triangle by pid
//   geom    [num_geom]   rt_tri_t    48 B  geometry triangles, ascending pid (flat)
//   ovtris  [tail prims] rt_vtri_t   64 B  the ordered tail's primitives, ascending pid (rt_om)
//   oidx / olist         u32              per-block lists of tail pids (rt_om)
//   cbuf    W*H*4 (linear, row 0 = NDC y=-1) or tiles*1024*4 (compact shard)
#pragma once

#include <stdint.h>

// one wave per workgroup: the dispatcher places (and retires) single waves,
// so a long wave never holds three finished partners' slots (64 vs 256
// threads: -7 % kernel time on tekkaman 1024^2)
#ifndef RT_BLOCK_THREADS
#define RT_BLOCK_THREADS 64
#endif
// per-wave LDS traversal stack depth: the regular image holds 24 entries
// (6 KB per wave: LDS still fits more waves than the VGPR budget allows),
// the deep image 32; the host picks the image from the built BVH's
// worst-case stack (BVH2: its depth; BVH4: stack4, e.g. 16-17 for the
// reference scenes)
#define RT_STACK_SHALLOW 24
#define RT_STACK_DEEP 32
#ifndef RT_MAX_STACK
#define RT_MAX_STACK RT_STACK_SHALLOW
#endif
// 1: a per-lane BVH4 step writes all three push rows unconditionally (rows at
// or above the new top hold garbage that is never read); the stack then
// carries 3 slack rows past its capacity for the writes of a full stack
#ifndef RT_PUSH_UNCOND
#define RT_PUSH_UNCOND 0
#endif
#define RT_STACK_ROWS (RT_MAX_STACK + (RT_PUSH_UNCOND ? 3 : 0))
#define RT_TILE_LOG 5            // RASTER_TILE_LOGSIZE (VX_config.vh:477-479)
#define RT_TILE_PIXELS 1024
#define RT_RASTER_TILE_LOG 4     // raster workgroup tile: 16x16 pixels, one per thread

#define RT_FLAG_SHADOWS  0x1u
#define RT_FLAG_TIE_HIGH 0x2u    // LEQUAL geometry: equal t -> highest pid
#define RT_FLAG_COMPACT  0x4u    // shard output: compact tile buffer
#define RT_FLAG_PATH     0x8u    // diffuse path trace (pt_kernel.hip)
#define RT_FLAG_FLAT     0x10u   // flat triangle list, no BVH (BASELINE config 2)
#define RT_FLAG_RASTER   0x20u   // draw3d raster pipeline (raster_kernel.hip)
#define RT_FLAG_BVH4     0x40u   // traverse the 4-wide BVH (nodes4) instead of the BVH2
#define RT_FLAG_BVH4H    0x80u   // BVH4 node steps read the binary16 rt_node4h_t form
#define RT_FLAG_COVERAGE 0x100u  // raster mode: covered pixels white, no shading / OM
// primary+shadow frames of image rt_kernel: a wave traces its last geometry chunk's shadow rays in
// place behind the shading's loads (rt_kernel.hip RT_FUSED_CHUNK; app/fused_chunk.h sets it at
// configure, env RT_FUSED_CHUNK=0: off).  Every other image ignores the bit.
#define RT_FLAG_FUSED    0x200u

// a render launch's words (vortex_hip.h vx_hip_set_launch_words, vx_spawn.h
// vx_launch_words; rt_render_start sets them on every frame): w[0..2] the
// frame's light (float bits), w[3] flags -- a moved light reaches the frame
// in its dispatch packet, not through a copy into the argument block
#define RT_LW_LIGHT    0x1u  // w[0..2] is the light (over arg.light)
#define RT_LW_NO_SLIST 0x2u  // the light-space lists are stale: shadow rays walk the BVH
// w[3] bits 8-31: the frame's framebuffer as an arena offset past arg.cbuf_addr, mod 2^32,
// in the allocator's 256-B units (0: cbuf itself) -- two consecutive frames on the driver's
// two launch lanes write apart.  In the launch word: rt_kernel_arg_t stays as it was;
// added at the framebuffer stores (rt_trace.h store_out)
#define RT_LW_CBUF_MASK 0xffffff00u
// w[3] bits 2-7, read by the accumulating path tracer only (pt_kernel.hip PT_ACCUM, image
// pt_accum): bit 2 = the launch treats every accumulation record as zero and does not read
// it, bits 3-7 = the launch's samples per pixel minus one (1..32)
#define RT_LW_ACCUM_RESET   0x4u
#define RT_LW_ACCUM_K_SHIFT 3
#define RT_LW_ACCUM_K_MASK  0xf8u
#define RT_ACCUM_MAX_K      32u
#define RT_ACCUM_MAX_SAMPLES (1u << 24)  // a record's u32 sums of 8-bit samples cannot overflow below it

#define RT_DC_DEPTH   0x1u
#define RT_DC_COLOR   0x2u
#define RT_DC_TEX     0x4u
#define RT_DC_MODULATE 0x8u

#define RT_LEAF_FLAG 0x80000000u
#define RT_EMPTY_REF (-1)

// statistics: user MPM counters, vx_mpm_query(VX_CSR_MPM_BASE + RT_MPM_USER + slot)
#define RT_MPM_USER 3
enum {
  RT_STAT_PRIMARY = 0, RT_STAT_SHADOW, RT_STAT_HITS, RT_STAT_OCCLUDED,
  RT_STAT_NODE_VISITS, RT_STAT_TRI_TESTS, RT_STAT_LAYER_TESTS, RT_STAT_SHADED,
  RT_STAT_TEXEL_BYTES, RT_STAT_BOUNCE, RT_STAT_RECT_TESTS, RT_STAT_EDGE_TESTS, RT_STAT_COUNT = 16
};

// rt_node_t: 4 x float4 =
//   (b0lo.x, b0hi.x, b1lo.x, b1hi.x), (.. y ..), (.. z ..), (c0, c1, 0, 0)
// child ref c: >= 0 internal node index; -1 empty; otherwise a leaf:
//   (c & 0x7fffffff) >> 4 = first triangle, (c & 15) + 1 = triangle count.
typedef struct { float v[16]; } rt_node_t;

// rt_node4_t (BVH4, 128 B): SoA over the 4 children --
//   lo.x[4], hi.x[4], lo.y[4], hi.y[4], lo.z[4], hi.z[4], child[4], pad[4];
// child refs as in rt_node_t (unused slots -1).  Collapsed from the BVH2
// (bvh.cpp): same leaves, same padded boxes, half the levels.
typedef struct { float v[32]; } rt_node4_t;

// rt_node4h_t (BVH4, 64 B): the same node with its 24 box planes as IEEE
// binary16 in rt_node4_t's order (lo.x[4], hi.x[4], lo.y[4], ...), then the
// 4 child refs.  The host rounds every BVH4 box outward to binary16-
// representable values (bvh.cpp RoundBoxes4), so rt_node4_t holds exactly the
// values this form decodes to and both describe one tree.  The kernel reads
// this form (4 loads of 16 B per node step instead of 7); it is uploaded right
// behind the rt_node4_t array (nodes4_addr + 128 * num_nodes4).
typedef struct { uint16_t b[24]; int32_t child[4]; } rt_node4h_t;


// rt_tri_t: (v0.x, v0.y, v0.w, pid), (e1.xyw, 0), (e2.xyw, 0) -- clip (x,y,w)
typedef struct { float v[12]; } rt_tri_t;

// ---- primary visibility (raster-exact primary rays, app/vis.cpp) ----------
// A primary ray through pixel (x, y) hits primitive p exactly where draw3d's
// rasterizer covers (x, y) with p: all three Q15.16 edge values >= 0
// (graphics.cpp:813-825, int32 wrap) inside a 32x32 tile p was binned to
// (gfxutil.cpp:237-271), and the closest hit is the draw3d depth test's
// winner: the smallest 24-bit depth word (graphics.cpp:564-596), ties to the
// first drawn (LESS) or last drawn (LEQUAL) primitive.  Per resolution the
// host computes every primitive's covered-pixel rectangle (exact, integer)
// and a lower bound of its depth word, and the BVH's nodes get the union /
// minimum over their subtrees: primary traversal is a 2D point-in-rect walk
// with depth culling, then the exact fixed-point test at the leaves.
// Pixel rectangles: x0 | x1 << 16 and y0 | y1 << 16, inclusive; an empty
// rectangle is x0 = 0xffff, x1 = 0.
#define RT_VIS_EMPTY_RECT 0x0000ffffu
#define RT_VIS_ZMIN_NONE 0xffffffffu
// rt_vnode_t (64 B), index-aligned with the traversed tree's nodes (BVH4, or
// BVH2 in slots 0-1): per child its covered-pixel rectangle as its corners
// lo = x0 | y0 << 16 and hi = x1 | y1 << 16 (inclusive: a pixel packed as
// x | y << 16 is inside iff two packed 16-bit clamps leave it unchanged),
// depth lower bound and reference (RT_EMPTY_REF when the child covers no
// pixel; its lo = hi = RT_VIS_EMPTY_RECT)
typedef struct {
  uint32_t lo[4], hi[4], zmin[4];
  int32_t child[4];
} rt_vnode_t;
// rt_vtri_t (64 B), index-aligned with the leaf triangle records (tris):
// edges[3][3] Q15.16, covered rectangle, pid, the z attribute (Q7.24
// a0-a2, a1-a2, a2) and the depth lower bound
typedef struct {
  int32_t edges[9];
  uint32_t rx, ry;
  int32_t pid;
  int32_t z[3];
  uint32_t zmin;
} rt_vtri_t;

typedef struct {
  int32_t edges[3][3];     // Q15.16 (graphics.h:61-64)
  int32_t attribs[7][3];   // Q7.24  z,r,g,b,a,u,v x (a0-a2, a1-a2, a2)
  uint32_t dc;             // drawcall index
  uint32_t pad;
} rt_prim_t;

typedef struct {
  uint32_t flags;          // RT_DC_*
  uint32_t tex_logw, tex_logh, tex_format, tex_filter, tex_wrapu, tex_wrapv, tex_stride;
  uint64_t tex_addr;
  uint32_t pad[6];
} rt_dcstate_t;

// Output-merger state of a drawcall for the raster pipeline (raster_kernel):
// DepthTencil / Blender / OutputMerger configuration derived from the
// draw3d DCR writes (draw3d/main.cpp:223-284 -> graphics.cpp:534-620,
// gpu_sw.h:78-98), quirks included.  32 words.
typedef struct {
  uint32_t depth_func, depth_writemask, depth_test_on;
  uint32_t stencil_func, stencil_zpass, stencil_zfail, stencil_fail;
  uint32_t stencil_ref, stencil_mask, stencil_writemask, stencil_on;
  uint32_t blend_mode_rgb, blend_mode_a, blend_src_rgb, blend_src_a, blend_dst_rgb, blend_dst_a;
  uint32_t blend_const, logic_op, blend_on;
  uint32_t cbuf_writemask, color_read, color_write;
  uint32_t prim_offset, prim_count;   // the drawcall's primitives (global pids)
  uint32_t pad[7];
} rt_omstate_t;

// screen bounding box of a primitive in pixels (gfxutil.cpp:168-192, clamped
// to the viewport): x in [lo & 0xffff, lo >> 16), y in [hi & 0xffff, hi >> 16);
// empty (x0 == x1) for degenerate or culled primitives
typedef struct {
  uint32_t x, y;
} rt_bbox_t;

typedef struct {
  uint64_t cbuf_addr, nodes_addr, tris_addr, vlayers_addr, prims_addr, dcs_addr;
  uint64_t ptris_addr;     // rt_tri_t per pid (path trace: bounce-hit barycentrics)
  uint64_t geom_addr;      // rt_tri_t of the geometry prims, ascending pid (flat mode)
  uint32_t width, height, tiles_x, tiles_y;
  uint32_t num_tasks, num_nodes, num_layer_tris, flags;
  uint32_t clear_color, shard_index, shard_count, bounces;
  float sx, sy;            // 2/W, 2/H
  float light[3];
  uint32_t seed;           // path-trace RNG seed
  uint32_t num_geom;       // geometry triangles (flat mode)
  uint32_t num_drawcalls;  // raster mode
  uint32_t raster_tile_log;  // raster mode: tile side 2^log (4: 16x16 px, 1 px/thread; 5: 32x32, 2x2/thread)
  uint32_t num_vnodes;     // rt_vnode_t records (0: no primitive covers a pixel)
  uint64_t zbuf_addr;      // raster mode: depth/stencil buffer, W*H u32
  uint64_t oms_addr;       // raster mode: rt_omstate_t per drawcall
  uint64_t bbox_addr;      // raster mode: rt_bbox_t per pid
  uint64_t nodes4_addr;    // rt_node4_t BVH4 (images built with RT_BVH4)
  uint32_t num_nodes4;
  uint32_t split_tiles;    // the first split_tiles tiles of the work order run 32 pixels per wave
  uint64_t order_addr;     // RT modes: u32 per local tile, the order tiles are worked in
                           // (heaviest first; 0 = identity), see rt_app.cpp TileOrder
  uint64_t vnodes_addr;    // rt_vnode_t per node of the traversed tree (primary visibility)
  uint64_t vtris_addr;     // rt_vtri_t per leaf triangle record (+3 padding records)
  uint64_t vgeom_addr;     // rt_vtri_t per geometry primitive, ascending pid (flat mode)
  uint32_t split_log;      // split tiles run 2^split_log pixels per wave (5: 32, an 8x4 half block)
  uint32_t blist_blocks;   // per-block candidate lists: local 8x8 blocks (local_tiles * 16), 0 = walk the tree
  uint64_t blist_addr;     // rt_bentry_t [entries + 2]: every local block's list, concatenated
  uint64_t bidx_addr;      // uint32[2] per local block lt * 16 + (by & 3) * 4 + (bx & 3): first entry, count
  uint32_t slist_on;       // light-space shadow lists built for `light` (0: shadow rays walk the BVH)
  uint32_t slist_n;        // their cells per cube-face side (RT_SLIST_N unless env RT_SLIST_N)
  uint64_t sidx_addr;      // uint32[2] per light-space cell: first entry, count
  uint64_t slist_addr;     // rt_tri_t per entry (+1 padding record): every cell's triangles, ascending pid
  uint32_t raster_bin_log; // raster mode: binning tile side 2^log (RASTER_TILE_LOGSIZE; draw3d -k)
  uint32_t pathq_lanes;    // pt_queue: paths per wave (64, 32 or 16; 0 = 64)
  uint64_t pathq_addr;     // path tracing in two kernels (pt_primary + pt_queue): uint4 per path
                           // start (task, plane t, hit pid, primary colour), compacted in
                           // RT_PQ_SEGS segments of pathq_seg_cap entries
  uint64_t pathq_ctr_addr; // counters, one 128-B line each (u32 word 32 * i): i < RT_PQ_SEGS
                           // paths queued in segment i; RT_PQ_SEGS + g pt_queue waves done of
                           // group g; 2 * RT_PQ_SEGS groups done (the last zeroes them all)
  uint32_t pathq_seg_cap;  // entries per segment
  uint32_t quad_tiles;     // the first quad_tiles of the split tiles run 16 pixels per wave
                           // (env RT_QUAD_TILES, a task-map probe; 0 by default)
  uint32_t tiles_x_magic;  // min(ceil(2^32 / tiles_x), 2^32 - 1): a tile's row is
                           // mulhi(tile, magic) plus at most one correction (rt_trace.h
                           // tile_row) -- no integer division in the kernels' task map
  uint32_t cdesc_first;    // the first chunk of the whole-block tier (the chunks the table covers)
  uint64_t cdesc_addr;     // rt_cdesc_t per 64-task chunk of the whole-block tier, in work order
                           // (0: no table, the kernels work the task map out themselves)
  // the ordered tail (rt_om_kernel.hip; vx_rt.h RT_SCENE_OM_LAYERS): the drawcalls the RT
  // path cannot trace, folded over the traced head's pixels in submission order
  uint64_t oidx_addr;      // uint32[2] per local 8x8 block (bidx's numbering): first entry, count
  uint64_t olist_addr;     // u32 pid per entry, ascending per block (+ RT_OLIST_PAD padding entries)
  uint64_t ovtris_addr;    // rt_vtri_t per tail primitive: record of pid at pid - otail_base
  uint32_t otail_base;     // the first tail primitive (the tail's pids are consecutive)
  uint32_t otail_count;    // tail primitives (0: no tail)
} rt_kernel_arg_t;
// The accumulating path tracer's argument area, in the argument buffer right behind
// rt_kernel_arg_t (which stays as it is): the accumulation buffer, one 16-B record
// uint32 {sumR, sumG, sumB, n} per framebuffer pixel at the pixel's framebuffer index --
// the per-channel sums of the 8-bit sample values and the number of samples in them
typedef struct {
  uint64_t accum_addr;
  uint64_t pad;
} rt_accum_arg_t;
// The background tier's argument area (rt_kernel.hip RT_BG_TIER), behind the two above, which
// stay where they are: constant from one configure to the next, so the frames in flight may
// read it.  What changes per launch -- the number of geometry-tier workgroups -- is the
// launch's tag.
typedef struct {
  uint32_t bg_first_chunk;  // the first chunk of the work order behind the tiles geometry reaches
                            // (16 * heavy tiles): every chunk from here on has an empty block list
  uint32_t pad;
  uint64_t bglayer_addr;    // rt_bglayer_t per chunk from bg_first_chunk on, in work order (0: no table)
} rt_tier_arg_t;
#define RT_TIER_ARG_OFFSET (sizeof(rt_kernel_arg_t) + sizeof(rt_accum_arg_t))
// The light table of a frame lit by several point lights (rt_kernel.hip RT_LIGHTS, images
// rt_lights / rt_lights_stats; vx_rt.h rt_renderer_set_lights), behind the three above, which
// stay where they are: per light its position and its own light-space shadow lists (slist_on 0:
// that light's shadow rays walk the BVH); every set is built at slist_n cells per face side.
#define RT_MAX_LIGHTS 16u
typedef struct {
  float light[3];
  uint32_t slist_on;
  uint64_t sidx_addr;
  uint64_t slist_addr;
} rt_light_t;
typedef struct {
  uint32_t count, slist_n, pad[2];
  rt_light_t l[RT_MAX_LIGHTS];
} rt_lights_arg_t;
#define RT_LIGHTS_ARG_OFFSET (RT_TIER_ARG_OFFSET + sizeof(rt_tier_arg_t))
// The visibility-record launch's argument area (rt_aov_kernel.hip, image rt_aov; vx_rt.h
// rt_render_aov_start), behind the four above, which stay where they are: the record buffer, one
// 16-B rt_aov_t {pid, depth word | flags, plane t, light mask} per framebuffer pixel at the
// pixel's framebuffer index.  Written when the buffer is allocated, in stream order: the frames
// in flight read the areas in front of it.  The number of lights in use is the launch's tag
// (0 or 1: the argument block's light and lists under the launch words, as a frame; n >= 2: the
// first n entries of the light table).
typedef struct {
  uint64_t aov_addr;
  uint64_t pad;
} rt_aov_arg_t;
#define RT_AOV_ARG_OFFSET (RT_LIGHTS_ARG_OFFSET + sizeof(rt_lights_arg_t))
// rt_aov_t::depth_flags above the 24-bit depth word (vx_rt.h names the same bits)
#define RT_AOV_GEOM       0x01000000u  // a geometry hit
#define RT_AOV_SHADOW_RAY 0x02000000u  // shadow rays start at the pixel
// The pixel of a shadow ray that `occluded` of its k lights (1 <= k <= RT_MAX_LIGHTS) do not
// see: per channel the rounded mean of the k single-light values, c for a light that sees it
// and c >> 1 (shadowed()) for one that does not -- sum = (k - o) * c + o * (c >> 1), mean =
// (2 * sum + k) / (2 * k) in integer division, the accumulation resolve on {sums, k}; the alpha
// byte is c's.  The division is a multiplication by m = ceil(2^20 / d), d = 2k <= 32: with
// e = m * d - 2^20 in [0, d), n * m / 2^20 = n / d + n * e / (d * 2^20), and the second term
// stays below 1 / d -- so the floor is floor(n / d) -- while n * e < 2^20; n = 2 * sum + k <=
// 2 * 16 * 255 + 16 = 8176 and e <= 31 give n * e <= 253 456.  n * m < 2^13 * 2^19 fits 32 bits.
// The kernel and the host (rt_lights_resolve) share this text.
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_lights_mix(uint32_t argb, uint32_t occluded, uint32_t k) {
  const uint32_t d = 2u * k, m = (0x100000u + d - 1u) / d;
  uint32_t out = argb & 0xff000000u;
  for (int s = 0; s <= 16; s += 8) {
    const uint32_t c = (argb >> s) & 0xffu;
    const uint32_t sum = (k - occluded) * c + occluded * (c >> 1);
    out |= (((2u * sum + k) * m) >> 20) << s;
  }
  return out;
}
// Relighting from the visibility records (vx_rt.h rt_relight_capture_start / rt_render_relight_start).
// The capture launch (rt_aov_kernel.hip RT_AOV_BASE, image rt_aov_base) writes rt_aov's records and,
// into the base-colour buffer, the pixel shaded without shadows: one ARGB word per framebuffer
// pixel at the pixel's framebuffer index.  The relight launch (rt_relight_kernel.hip, image
// rt_relight) streams both into the framebuffer in use.  Their argument area, behind the five
// above, which stay where they are: written when the buffers are allocated, in stream order,
// constant until the next configure.
typedef struct {
  uint64_t base_addr;   // the base-colour buffer
  uint32_t npix;        // framebuffer pixels (records, base colours)
  uint32_t cbuf1_off;   // the second framebuffer past arg.cbuf_addr, mod 2^32 (RT_RL_TAG_CBUF1)
} rt_relight_arg_t;
#define RT_RELIGHT_ARG_OFFSET (RT_AOV_ARG_OFFSET + sizeof(rt_aov_arg_t))
// A relight launch's words are its 16 weight bytes (light i: byte i & 3 of word i >> 2); its tag:
#define RT_RL_TAG_N_MASK  0x1fu      // bits 0-4: the lights in use at capture time, 1..RT_MAX_LIGHTS
#define RT_RL_TAG_CBUF1   0x20u      // bit 5: the framebuffer in use is the second one
#define RT_RL_TAG_M_SHIFT 8          // bits 8-30: the divisor's multiplier (rt_relight_div_t::m)
// The relit pixel: light i weighs w_i in 0..255, W = sum w_i >= 1 over the n lights, O = the sum
// over the lights whose mask bit is set.  A pixel with RT_AOV_SHADOW_RAY is, per channel c of the
// base colour, the weighted rounded mean of the single-light values -- (2 * ((W - O) * c + O *
// (c >> 1)) + W) / (2 * W) in integer division -- under the base colour's alpha; any other pixel
// is its base colour.
// The division, exact for every d = 2 * W <= 8160: with L = ceil(log2 d) <= 13 and s = 13 - L,
// d' = d << s lies in (2^12, 2^13] and x' = x << s has floor(x' / d') = floor(x / d).  m =
// ceil(2^34 / d') < 2^22 + 1, e = m * d' - 2^34 in [0, d'): x' * m / 2^34 = x' / d' + x' * e /
// (d' * 2^34), and the second term stays below 1 / d' -- so the floor is floor(x' / d') -- while
// x' * e < 2^34.  x <= 2 * 255 * W + W = 255.5 * d, so x' <= 255.5 * d' < 2^21, and e < 2^13.
// x' * m < 2^44: the product's high word, shifted right by 2.  The kernel and the host
// (rt_relight_resolve) share this text; m depends on W alone and reaches the kernel in its tag.
typedef struct {
  uint32_t s, m;
} rt_relight_div_t;
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_relight_shift(uint32_t W) {  // s of d = 2 * W, 1 <= W <= 4080
  uint32_t L = 1;
  while ((1u << L) < 2u * W) ++L;
  return 13u - L;
}
static inline rt_relight_div_t rt_relight_div(uint32_t W) {  // (the host's: a 64-bit division)
  rt_relight_div_t v;
  v.s = rt_relight_shift(W);
  const uint64_t d = (uint64_t)(2u * W) << v.s;
  v.m = (uint32_t)((((uint64_t)1 << 34) + d - 1u) / d);
  return v;
}
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_relight_mix(uint32_t base, uint32_t O, uint32_t W, uint32_t s, uint32_t m) {
  uint32_t out = base & 0xff000000u;
  for (int sh = 0; sh <= 16; sh += 8) {
    const uint32_t c = (base >> sh) & 0xffu;
    const uint32_t x = 2u * ((W - O) * c + O * (c >> 1)) + W;
    out |= (uint32_t)(((uint64_t)(x << s) * m) >> 34) << sh;
  }
  return out;
}
// O of a record's mask: the weights of the lights in use whose bit is set (bits >= n ignored)
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_relight_occluded(uint32_t mask, const uint32_t w[4], uint32_t n) {
  uint32_t O = 0;
  for (uint32_t i = 0; i < RT_MAX_LIGHTS; ++i)
    O += (i < n && ((mask >> i) & 1u)) ? (w[i >> 2] >> (8u * (i & 3u))) & 0xffu : 0u;
  return O;
}
// Denoising accumulated path frames (vx_rt.h rt_denoise_capture_start / rt_render_denoise_start).
// The capture launch (rt_aov_kernel.hip RT_AOV_BASE=2, image rt_aov_guide) writes one 16-B guide
// record per framebuffer pixel -- {pid, depth word | RT_AOV_GEOM, normal, 0}, the normal's three
// signed bytes packed x | y << 8 | z << 16 -- and the pixel's base colour; the prepare and pass
// launches (rt_denoise_kernel.hip, images rt_denoise_prep / rt_denoise_pass) work on the tap
// records below.  Their argument area, behind the six above, which stay where they are: written
// when the buffers are allocated, in stream order, constant until the next configure.  Every
// buffer holds one entry per framebuffer pixel in framebuffer order (linear W * H only).
typedef struct {
  uint64_t guide_addr;   // 16 B: the guide record (rt_denoise_guide_t)
  uint64_t base_addr;    // 4 B: the base colour (ARGB, the pixel shaded without shadows)
  uint64_t tapg_addr;    // 8 B: what a tap needs of the guide: {pid, or RT_DN_NO_GEOM for a pixel
                         // without RT_AOV_GEOM; depth word | normal x << 24}
  uint64_t irr_addr[2];  // 8 B each, ping-pong: {I_R | I_G << 16, I_B | normal y << 16 | normal z << 24}
                         // of a geometry pixel; {the resolved ARGB pixel, 0} of any other
  uint32_t width, height;
  uint32_t cbuf1_off;    // the second framebuffer past arg.cbuf_addr, mod 2^32 (RT_DN_TAG_CBUF1)
  uint32_t pad;
} rt_denoise_arg_t;
#define RT_DENOISE_ARG_OFFSET (RT_RELIGHT_ARG_OFFSET + sizeof(rt_relight_arg_t))
#define RT_DN_NO_GEOM 0xffffffffu
// A pass launch's words: w[0] = zs (depth shift, 0..23), w[1] = ls (irradiance shift, 0..16);
// its tag:
#define RT_DN_TAG_K_MASK 0x7u   // bits 0-2: the pass k, 1..5 (stride 2^(k-1); input irr[(k-1)&1])
#define RT_DN_TAG_LAST   0x8u   // bit 3: the last pass: remodulate and store to the framebuffer
#define RT_DN_TAG_CBUF1  0x10u  // bit 4: the framebuffer in use is the second one
#define RT_DN_MAX_PASSES 5u
#define RT_DN_MAX_ZS 23u
#define RT_DN_MAX_LS 16u
// The filter's integer pieces (vx_rt.h states the definition; tests/denoise_reference.py restates
// it in numpy from that text).  The kernels and the host share this text.
// an edge stop: E(e) = e >= 9 ? 0 : 256 >> e
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_dn_stop(uint32_t e) { return e >= 9u ? 0u : 256u >> e; }
// byte k of a packed normal, sign-extended
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline int32_t rt_dn_sbyte(uint32_t v, uint32_t k) { return (int32_t)(v << (24u - 8u * k)) >> 24; }
// the normal stop between two packed normals (x | y << 8 | z << 16): c = min(256, |Np . Nq| >> 6),
// wn = (c * c) >> 8, then wn = (wn * wn) >> 8
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_dn_wn(uint32_t np, uint32_t nq) {
  const int32_t d = rt_dn_sbyte(np, 0) * rt_dn_sbyte(nq, 0) + rt_dn_sbyte(np, 1) * rt_dn_sbyte(nq, 1) +
                    rt_dn_sbyte(np, 2) * rt_dn_sbyte(nq, 2);
  uint32_t c = (uint32_t)(d < 0 ? -d : d) >> 6;
  c = c > 256u ? 256u : c;
  const uint32_t w = (c * c) >> 8;
  return (w * w) >> 8;
}
// one channel's irradiance: the mean s / n over the albedo a / 256, I = min(65535, (256 * s +
// d / 2) / d) with d = n * max(a, 1); 256 * s reaches 2^40 (s <= 255 * 2^24), so 64 bits
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_dn_demod(uint32_t s, uint32_t n, uint32_t a) {
  const uint64_t d = (uint64_t)(n ? n : 1u) * (a ? a : 1u);
  const uint64_t q = (256u * (uint64_t)s + d / 2u) / d;
  return q > 65535u ? 65535u : (uint32_t)q;
}
// one channel remodulated: min(255, (I * a + 128) >> 8)
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_dn_remod(uint32_t I, uint32_t a) {
  const uint32_t v = (I * a + 128u) >> 8;
  return v > 255u ? 255u : v;
}
// Ambient occlusion from the visibility records (vx_rt.h rt_renderer_ao_begin / rt_render_ao_start /
// rt_render_ao_resolve_start).  The tracing launch (rt_ao_kernel.hip, image rt_ao) reads the record
// buffer of rt_aov_arg_t and adds, per framebuffer pixel, its occluded samples to one uint32 of the
// count buffer; the resolve launch (rt_ao_resolve_kernel.hip, image rt_ao_resolve) streams the counts
// -- and for RT_AO_MODULATE records and base colours -- into the framebuffer in use.  Their argument
// area, behind the seven above, which stay where they are: written when the buffer is allocated, in
// stream order, constant until the next configure.  Linear W * H framebuffers only.
typedef struct {
  uint64_t ao_addr;     // the count buffer, one uint32 per framebuffer pixel
  uint32_t npix;        // framebuffer pixels
  uint32_t cbuf1_off;   // the second framebuffer past arg.cbuf_addr, mod 2^32 (RT_AO_TAG_CBUF1)
} rt_ao_arg_t;
#define RT_AO_ARG_OFFSET (RT_DENOISE_ARG_OFFSET + sizeof(rt_denoise_arg_t))
// A tracing launch's words: w[0] = the radius (float bits; +inf admitted), w[1] = seed + the sample
// cursor of the launch's first sample (mod 2^32), w[2] = the bits below, w[3] = 0
#define RT_AO_LW_S_MASK 0x3fu      // bits 0-5: the launch's samples per ray pixel minus one (1..64)
#define RT_AO_LW_RESET  0x40u      // bit 6: the launch treats every count as zero and does not read it
#define RT_AO_MAX_S 64u
#define RT_AO_MAX_SAMPLES 65535u   // the sample cursor's cap: 2 * 255 * N + N fits 32 bits with room
// A resolve launch's words are RT_AO_MODULATE's 16 weight bytes (as a relight launch's); its tag:
#define RT_AO_TAG_N_MASK   0x1fu   // bits 0-4: RT_AO_MODULATE under weights: the capture's lights, 1..RT_MAX_LIGHTS
#define RT_AO_TAG_CBUF1    0x20u   // bit 5: the framebuffer in use is the second one
#define RT_AO_TAG_MODULATE 0x40u   // bit 6: RT_AO_MODULATE (else RT_AO_GREY)
#define RT_AO_TAG_WEIGHTS  0x80u   // bit 7: RT_AO_MODULATE relights the base colour under the words' weights
#define RT_AO_TAG_SAMPLES_SHIFT 8  // bits 8-23: N, the samples in the counts, 1..65535
// floor(x / d) for 1 <= d < 2^18 and x <= 256 * d, exact, from rd = 1.0f / (float)d (IEEE binary32, wave-
// uniform in the kernel: d depends on the launch alone).  (float)x is within 2^-24 of x relatively, rd
// within 2^-24 of 1 / d, their product rounds once more: the estimate is within 4 * 2^-24 * 256 = 2^-14
// of x / d, so its floor is floor(x / d) or one to either side, and one multiply-subtract tells which:
// the remainder against 0 and d.  q * d <= 257 * 2^18 fits 32 bits.
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_ao_quot(uint32_t x, uint32_t d, float rd) {
  uint32_t q = (uint32_t)((float)x * rd);
  const int32_t r = (int32_t)(x - q * d);
  q = r < 0 ? q - 1u : q;
  q = r >= (int32_t)d ? q + 1u : q;
  return q;
}
// The ambient term on a pixel (vx_rt.h rt_ao_resolve): per colour channel c of argb, (2 * c * (N - o) +
// N) / (2 * N) in integer division -- c scaled by the unoccluded share, rounded half up -- under argb's
// alpha byte; N = 1..65535 samples, o <= N of them occluded.  rd = 1.0f / (float)(2 * N).
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_ao_mix(uint32_t argb, uint32_t o, uint32_t N, float rd) {
  uint32_t out = argb & 0xff000000u;
  for (int sh = 0; sh <= 16; sh += 8) {
    const uint32_t c = (argb >> sh) & 0xffu;
    out |= rt_ao_quot(2u * c * (N - o) + N, 2u * N, rd) << sh;
  }
  return out;
}
// rt_relight_mix's pixel through rt_ao_quot (d = 2 * W <= 8160, x <= 255.5 * d): the same quotients,
// without the multiplier the relight launch's tag carries (the resolve launch's tag holds N instead)
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_ao_relight_mix(uint32_t base, uint32_t O, uint32_t W, float rd) {
  uint32_t out = base & 0xff000000u;
  for (int sh = 0; sh <= 16; sh += 8) {
    const uint32_t c = (base >> sh) & 0xffu;
    out |= rt_ao_quot(2u * ((W - O) * c + O * (c >> 1)) + W, 2u * W, rd) << sh;
  }
  return out;
}
// Caller-supplied rays against the scene's tree (vx_rt.h rt_query_reserve / rt_query_trace_start /
// rt_query_keys_start).  The tracing launch (rt_query_kernel.hip, image rt_query) reads rt_ray_t records
// (32 B: o[3], tmin, d[3], tmax) and stores one rt_hit_t (8 B: pid, t) per ray; the key launch
// (rt_query_keys_kernel.hip, image rt_query_keys) stores one coherence key per ray.  Their argument area,
// behind the eight above, which stay where they are: written by rt_query_reserve in stream order, constant
// until the next reserve -- a configure does not touch it.
typedef struct {
  uint64_t rays_addr;   // rt_ray_t [capacity]
  uint64_t hits_addr;   // rt_hit_t [capacity]
  uint64_t skip_addr;   // int32 [capacity]: the primitive a ray does not meet (RT_QUERY_SKIP)
  uint64_t perm_addr;   // uint32 [capacity]: slot -> ray index (RT_QUERY_PERM)
  uint64_t keys_addr;   // uint32 [capacity]: the coherence keys
  uint32_t capacity;    // rays reserved
  uint32_t pad;
  float key_lo[3];      // the key grid: the scene box's low corner ...
  float key_inv[3];     // ... and 128 / its extent per axis (0 for a flat axis)
} rt_query_arg_t;
#define RT_QUERY_ARG_OFFSET (RT_AO_ARG_OFFSET + sizeof(rt_ao_arg_t))
// A query launch's words: w[0] = n, the rays of the launch; w[1] = the mode (bits 0-7: RT_QUERY_CLOSEST /
// RT_QUERY_ANY) and the flags (bits 8-15: RT_QUERY_SKIP / RT_QUERY_PERM as vx_rt.h numbers them, shifted);
// w[2] = w[3] = 0 (a frame's light bits: none)
#define RT_QUERY_LW_MODE_MASK 0xffu
#define RT_QUERY_LW_FLAG_SHIFT 8
#define RT_QUERY_MISS_KEY 0xffffffffu
// A malformed ray (vx_rt.h): any of its 8 words NaN, an infinite origin or direction component, or an
// all-zero direction.  w = the record's words: o[3], tmin, d[3], tmax.
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline int rt_query_malformed(const uint32_t w[8]) {
  int bad = 0, zero = 1;
  for (int k = 0; k < 8; ++k) {
    const uint32_t m = w[k] & 0x7fffffffu;
    bad |= m > 0x7f800000u;                            // NaN
    if (k != 3 && k != 7) bad |= m == 0x7f800000u;     // o, d: infinite
    if (k >= 4 && k < 7) zero &= m == 0u;              // d: +-0
  }
  return bad | zero;
}
// The spread of a 7-bit cell index to every third bit (Morton interleave)
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_query_part3(uint32_t c) {
  uint32_t r = 0;
  for (int b = 0; b < 7; ++b) r |= ((c >> b) & 1u) << (3 * b);
  return r;
}
// The coherence key of a ray (vx_rt.h has the definition; every operation binary32, none fused -- each is a
// single rounding, so host and device agree bit for bit)
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_query_key_of(const uint32_t w[8], const float lo[3], const float inv[3]) {
  if (rt_query_malformed(w)) return RT_QUERY_MISS_KEY;
  float o[3], a[3];
  uint32_t key = 0;
  for (int k = 0; k < 3; ++k) {
    const uint32_t ow = w[k], aw = w[4 + k] & 0x7fffffffu;
    __builtin_memcpy(&o[k], &ow, 4);
    __builtin_memcpy(&a[k], &aw, 4);
    key |= (w[4 + k] >> 31) << (31 - k);
    const float g = (o[k] - lo[k]) * inv[k];   // (inf * 0 on a flat axis is NaN: fmaxf returns the 0)
    const uint32_t c = (uint32_t)__builtin_fminf(__builtin_fmaxf(g, 0.0f), 127.0f);
    key |= rt_query_part3(c) << (8 + k);
  }
  const float s = (a[0] + a[1]) + a[2];        // > 0; +inf when it overflows: both cells 0 then
  const uint32_t cx = (uint32_t)__builtin_fminf((a[0] / s) * 16.0f, 15.0f);
  const uint32_t cy = (uint32_t)__builtin_fminf((a[1] / s) * 16.0f, 15.0f);
  return key | (cy << 4) | cx;
}
// Soft shadows from area lights, sampled from the visibility records (vx_rt.h rt_renderer_soft_begin /
// rt_render_soft_start / rt_render_soft_resolve_start).  The tracing launch (rt_soft_kernel.hip, image
// rt_soft) reads the record buffer of rt_aov_arg_t and adds, per light in use and framebuffer pixel, its
// occluded samples to one uint16 of the count planes (plane i at planes_addr + 2 * npix * i); the resolve
// launch (rt_soft_resolve_kernel.hip, image rt_soft_resolve) streams the planes and the relight capture's
// base colours into the framebuffer in use.  Their argument area, behind the nine above, which stay where
// they are: written by rt_renderer_soft_begin in stream order, constant until the session ends.  The
// lights' positions stand beside their radii: a session's lights do not move (a call that changes the
// lights ends it), and one light and several reach a frame by different roads (the launch words, the light
// table) which this launch need not follow.  Linear W * H framebuffers only.
typedef struct {
  uint64_t planes_addr;             // the count planes, uint16 [n][npix]
  uint32_t npix;                    // framebuffer pixels
  uint32_t cbuf1_off;               // the second framebuffer past arg.cbuf_addr, mod 2^32 (RT_SOFT_TAG_CBUF1)
  float radii[RT_MAX_LIGHTS];       // light i's radius, finite and >= 0
  float light[RT_MAX_LIGHTS][3];    // light i's centre
} rt_soft_arg_t;
#define RT_SOFT_ARG_OFFSET (RT_QUERY_ARG_OFFSET + sizeof(rt_query_arg_t))
// A tracing launch's words: w[0] = seed + the sample cursor of the launch's first sample (mod 2^32), w[1] =
// the bits below, w[2] = w[3] = 0 (a frame's flags: none)
#define RT_SOFT_LW_S_MASK  0x3fu      // bits 0-5: the launch's samples per ray pixel and light minus one (1..64)
#define RT_SOFT_LW_RESET   0x40u      // bit 6: the launch treats every count as zero and does not read it
#define RT_SOFT_LW_N_SHIFT 8          // bits 8-12: the lights in use, 1..RT_MAX_LIGHTS
#define RT_SOFT_MAX_S 64u
#define RT_SOFT_MAX_SAMPLES 1024u     // the sample cursor's cap: 511 * N * sum w <= 511 * 1024 * 4080 < 2^32
#define RT_SOFT_VERTEX 64u            // light i's samples are keyed at path vertex RT_SOFT_VERTEX + i
// A resolve launch's words are its 16 weight bytes (as a relight launch's); its tag:
#define RT_SOFT_TAG_N_MASK 0x1fu      // bits 0-4: the session's lights, 1..RT_MAX_LIGHTS
#define RT_SOFT_TAG_CBUF1  0x20u      // bit 5: the framebuffer in use is the second one
#define RT_SOFT_TAG_LIT    0x40u      // bit 6: RT_SOFT_LIT (the capture's base colours), else RT_SOFT_GREY (white)
#define RT_SOFT_TAG_SAMPLES_SHIFT 8   // bits 8-18: N, the samples in the counts, 1..1024
// The soft-shadow pixel (vx_rt.h rt_soft_resolve): D = N * sum w_i, O = sum w_i * o_i (o_i <= N) <= D; per
// colour channel c of base (2 * ((D - O) * c + O * (c >> 1)) + D) / (2 * D) in integer division, the
// relight mean with every light's weight split over its N samples, under base's alpha byte.  The numerator
// is at most 2 * 255 * D + D = 511 * D <= 511 * 1024 * 4080 = 2 134 917 120 < 2^32.  The division is
// rt_ao_quot's, whose argument holds for this divisor too: d = 2 * D < 2^23 is exact in binary32, x <= 255.5
// * d, the estimate (float)x * rd lies within 256 * 3 * 2^-24 < 2^-14 of x / d, and q * d <= 256 * 2^23 =
// 2^31 with a remainder below 2 * d < 2^24 in magnitude.  rd = 1.0f / (float)(2 * D).  O = 0 gives c back: a
// pixel that is not a ray pixel, whose counts are 0, keeps its base colour.  The kernel and the host share
// this text.
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_soft_mix(uint32_t base, uint32_t O, uint32_t D, float rd) {
  uint32_t out = base & 0xff000000u;
  for (int sh = 0; sh <= 16; sh += 8) {
    const uint32_t c = (base >> sh) & 0xffu;
    out |= rt_ao_quot(2u * ((D - O) * c + O * (c >> 1)) + D, 2u * D, rd) << sh;
  }
  return out;
}
// A path-traced frame lit by several point lights (pt_kernel.hip PT_LIGHTS, images pt_lights /
// pt_lights_accum; vx_rt.h rt_renderer_set_path_lights) reads the first count <=
// RT_MAX_PATH_LIGHTS entries of the same table, every one with lists (slist_on 1).  The cap is
// the kernel's LDS: three float accumulators per light and lane, 768 B a light in a one-wave
// workgroup, next to the 6 912 B traversal stack -- 8 lights keep 12 workgroups on a CU.
#define RT_MAX_PATH_LIGHTS 8u
// One channel of such a frame's pixel: the rounded mean (2 * sum + k) / (2 * k) in integer
// division of the k single-light 8-bit values (sum = their sum, 1 <= k <= RT_MAX_PATH_LIGHTS),
// the accumulation resolve on {sum, k}.  As in rt_lights_mix the division is a multiplication
// by m = ceil(2^20 / d), d = 2k <= 16: with e = m * d - 2^20 in [0, d), n * m / 2^20 = n / d +
// n * e / (d * 2^20), whose second term stays below 1 / d -- so the floor is floor(n / d) --
// while n * e < 2^20; n = 2 * sum + k <= 2 * 8 * 255 + 8 = 4088 and e <= 15 give n * e <=
// 61 320.  n * m < 2^12 * 2^19 fits 32 bits.  The kernel and the host (rt_path_lights_resolve)
// share this text.
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t rt_path_lights_mean(uint32_t sum, uint32_t k) {
  const uint32_t d = 2u * k, m = (0x100000u + d - 1u) / d;
  return ((2u * sum + k) * m) >> 20;
}
// padding entries after the last tail list (the first tail pid): the fold
// loads the entry two ahead and the record one ahead of the one it tests
#define RT_OLIST_PAD 2u
// One 64-task chunk of the whole-block tier (an 8x8 pixel block), written by
// the device setup (rt_setup.hip RTS_CDESC) and restated on the host
// (app/setup.cpp ChunkDescs): everything rt_kernel's chunk_map / chunk_pixel
// and the block's list header give, in one 16-B scalar load.  It depends on
// the size, the shard, the work order, the buffer layout and the block
// lists -- not on the light.
typedef struct {
  uint32_t origin;  // the block's first pixel: x | y << 16
  uint32_t out;     // framebuffer word of lane 0 (compact or linear layout resolved)
  uint32_t first;   // the block's candidate list: first entry in blist
  uint32_t count;   // its length (bits 0-15) | the framebuffer words per pixel row << 16
} rt_cdesc_t;
// The background-layer table (rt_kernel.hip RT_BG_LAYERS): one record per chunk at or behind
// rt_tier_arg_t::bg_first_chunk, in work order -- which screen layer covers the chunk's 8x8 block,
// worked out once per configure by the device setup (rt_setup.hip RTS_BGLAYER) with the rule of
// rt_trace.h resolve_layers_n (painter order: the first covering record of vlayers wins;
// rt_layer_covers below) and restated on the host (app/setup.cpp BgLayers).  It depends on the
// scene, the size and the work order, as the chunk table does -- not on the light.
typedef struct {
  uint32_t pid1;  // pid + 1 of the one layer primitive that covers all 64 pixels; RT_BGLAYER_NONE: no layer
                  // covers any of them (the clear colour); 0: mixed, or a pixel outside the image
  uint32_t dc;    // that primitive's drawcall index (0 without one)
} rt_bglayer_t;
#define RT_BGLAYER_NONE 0xffffffffu
// a screen layer's record covers pixel (px, py): inside its rectangle (corners packed lo | hi << 16,
// inclusive) and on the inner side of its three edges (a*x + b*y + c with int32 wrap, >= 0: no top-left
// rule) -- resolve_layers_n's test per lane, the table's builders' per pixel of a block
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline int rt_layer_covers(const int32_t e[9], uint32_t rx, uint32_t ry, uint32_t px, uint32_t py) {
  if (px < (rx & 0xffffu) || px > (rx >> 16) || py < (ry & 0xffffu) || py > (ry >> 16)) return 0;
  for (int k = 0; k < 3; ++k)
    if ((int32_t)((uint32_t)e[3 * k] * px + (uint32_t)e[3 * k + 1] * py + (uint32_t)e[3 * k + 2]) < 0) return 0;
  return 1;
}
// the reciprocal rt_kernel_arg_t::tiles_x_magic holds for `tiles_x` tiles per row
static inline uint32_t rt_tiles_x_magic(uint32_t tiles_x) {
  if (tiles_x <= 1) return 0xffffffffu;
  return (uint32_t)((0x100000000ull + tiles_x - 1) / tiles_x);
}
// the path queue is split into segments (a primary chunk c appends to segment
// c % RT_PQ_SEGS) so its atomics spread over that many counters: one
// device-scope counter for the whole frame serialised ~1 600 atomics
#define RT_PQ_SEGS 64

// ---- light-space shadow lists (shadow rays to the point light) ------------
// A shadow segment P -> L is identified by its direction from the light,
// u = P - L, binned on the 6 faces of a cube around the light: face 2k +
// (u_k < 0) for the dominant axis k (ties to the lower axis), face
// coordinates (u_i, u_j) / |u_k| in [-1, 1] with (i, j) the other two axes in
// order, RT_SLIST_N x RT_SLIST_N cells, cell = (face * N + cy) * N + cx.  A
// cell's list holds every geometry triangle whose projection from the light
// reaches it (clipped to the face frustum widened by RT_SLIST_EPS, polygon
// box and separating-axis test against the cell widened by RT_SLIST_EPS):
// conservative, so any-hit over the list is the brute force's verdict.
// Built on the device (rt_setup.hip SCOUNT .. SSORT); oracle/rt.c sl_build
// restates it.
#define RT_SLIST_N 128              // default cells per face side (the oracle's SL_N); A/B r04g (nearest-first bounded lists): config 3 128 0.01836 / 256 0.0182 / 64 0.02072 ms, config 4 128 0.14286 / 256 0.14324; the lists build 4x fewer cells (set_light 0.137 -> 0.113 ms)
#define RT_SLIST_EPS (1.0f / 512.0f)

// ---- per-8x8-block candidate lists (primary visibility) -------------------
// For every 8x8 pixel block of the shard's tiles (local block lb = local
// tile * 16 + block of the tile), the geometry primitives whose covered-pixel
// rectangle reaches the block, ascending (depth lower bound, geometry index):
// the finer-grained form of draw3d's per-tile primitive lists
// (gfxutil.cpp:237-271).  Each entry carries the union rectangle (corners) of
// itself and the entries after it, so a wave stops scanning once no lane can
// change its winner.  Built on the device (rt_setup.hip, BCOUNT .. BSORT) or by
// the host restatement (rt_app.cpp BuildBlockLists); oracle/rt.c
// vis_build_lists restates them.
typedef struct {
  uint32_t k;              // geometry index (rt_vtri_t vgeom[k])
  uint32_t lo, hi;         // union rectangle of this entry and the rest: corners x | y << 16
  uint32_t zmin;           // this entry's depth lower bound (the smallest of the rest)
} rt_bentry_t;
// padding entries after the last list: block_primary loads the next pair of
// entries with each round's records, so the last round of an odd-length list
// ending at the end of the array reads up to 3 entries past it
#define RT_BLIST_PAD 3u
#define RT_BLIST_PAD_LO 0xffffffffu   // padding entries: a rectangle no pixel is in
#define RT_BLIST_PAD_HI 0xfffefffeu
#define RT_BLIST_MAX_LIST 1024u       // longest list the device sort takes (else: tree walk)
