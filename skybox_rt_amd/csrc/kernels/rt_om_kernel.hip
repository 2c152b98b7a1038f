// rt_om_kernel.hip -- the RT frame of a scene with an ordered tail (vx_rt.h
// RT_SCENE_OM_LAYERS): drawcalls that blend, use the stencil, mask colour
// channels or overlay geometry with depth-off layers cannot be traced, so the
// scene is split where the first of them starts.  The drawcalls before it
// (the traced head) are rendered as rt_kernel renders them -- raster-exact
// primary visibility, screen layers, draw3d shading of the winner and, with
// RT_FLAG_SHADOWS, one shadow ray per geometry hit -- and leave every pixel a
// colour and a depth/stencil word in its lane's registers.  The tail's
// primitives that cover the pixel are then folded over the two words in
// ascending primitive index through the output merger (gfx_device.h
// om_write: depth/stencil test, blending, write masks), the way
// raster_kernel.hip applies every fragment, and the pixel is stored once.
// Without shadow rays the frame is the raster pipeline's frame of the whole
// scene.  Tail fragments cast no shadow rays and occlude none.
//
// One wave per 8x8 block on rt_kernel's task map (chunk_map / chunk_pixel /
// store_out: linear, compact and sharded output alike).  The pixel stays in
// its lane from the head to the store, so the shadow rays are traced in
// place under an `active` mask, not through rt_kernel's LDS compaction
// queue.  The tail comes as per-block lists (rt_common.h oidx / olist, built
// by the host: app/vis.cpp BuildTailLists) in ascending primitive index with
// no depth ordering and no early out -- blending is order dependent.  List
// entries, the primitives' rt_vtri_t / rt_prim_t records and the drawcalls'
// state records are wave-uniform and come in through the scalar cache; the
// next entry's record is loaded with the current entry's test; the two state
// records of a drawcall are reloaded only when the drawcall changes; a
// primitive no lane of the wave is covered by costs its 64-B record and the
// edge functions, nothing else.
//
// Image rt_om (Makefile): the binary16 BVH4 only (RT_ONLY_BVH4H), walked as
// packets whose stack is the lanes of one VGPR, so the image is built with
// the deep stack bound (RT_MAX_STACK 32) at no cost; a tree of another
// layout (the generic deep images' case) is refused by rt_renderer_configure.
#include <hip/hip_runtime.h>

#ifndef RT_BLOCK_THREADS
#define RT_BLOCK_THREADS 64
#endif
#define VX_BLOCK_THREADS RT_BLOCK_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "rt_trace.h"

#if !RT_ONLY_BVH4H
#error "rt_om_kernel.hip walks the binary16 BVH4 only (build with -DRT_ONLY_BVH4H=1)"
#endif

namespace {

using namespace rtk;

// the tail's arrays, read from the argument block where the fold starts
// (rt_trace.h Scene stays as the other images have it)
struct Tail {
  uint32_t oidx, olist, ovtris, base, oms;
};
__device__ __forceinline__ Tail tail_args(const Scene& S) {
  const auto* a = arg_at(S);
  Tail t;
  t.oidx = (uint32_t)a->oidx_addr;
  t.olist = (uint32_t)a->olist_addr;
  t.ovtris = (uint32_t)a->ovtris_addr;
  t.base = a->otail_base;
  t.oms = (uint32_t)a->oms_addr;
  return t;
}

// A drawcall's output-merger state in scalar registers: the first 24 words of
// its rt_omstate_t (everything om_write reads; the primitive range and the
// padding stay out), wave-uniform.  Kept as the six loaded words and named
// field by field where om_write is called, so the record never becomes a
// stack object.
struct OmWords {
  uint4 v[6];
};
__device__ __forceinline__ OmWords load_om(const vx_arena& A, uint32_t off) {
  OmWords o;
  A.sld_u4n<6>(off, o.v);
  return o;
}
static_assert(offsetof(rt_omstate_t, depth_func) == 0 && offsetof(rt_omstate_t, stencil_on) == 40 &&
                  offsetof(rt_omstate_t, blend_on) == 76 && offsetof(rt_omstate_t, color_write) == 88,
              "om_state names rt_omstate_t's words in order");
__device__ __forceinline__ rt_omstate_t om_state(const OmWords& o) {
  rt_omstate_t s = {};
  s.depth_func = o.v[0].x; s.depth_writemask = o.v[0].y; s.depth_test_on = o.v[0].z;
  s.stencil_func = o.v[0].w; s.stencil_zpass = o.v[1].x; s.stencil_zfail = o.v[1].y;
  s.stencil_fail = o.v[1].z; s.stencil_ref = o.v[1].w; s.stencil_mask = o.v[2].x;
  s.stencil_writemask = o.v[2].y; s.stencil_on = o.v[2].z;
  s.blend_mode_rgb = o.v[2].w; s.blend_mode_a = o.v[3].x; s.blend_src_rgb = o.v[3].y;
  s.blend_src_a = o.v[3].z; s.blend_dst_rgb = o.v[3].w; s.blend_dst_a = o.v[4].x;
  s.blend_const = o.v[4].y; s.logic_op = o.v[4].z; s.blend_on = o.v[4].w;
  s.cbuf_writemask = o.v[5].x; s.color_read = o.v[5].y; s.color_write = o.v[5].z;
  return s;
}

__device__ __forceinline__ void kernel_body(const vx_task_t& task, const Scene& S, Counters& cnt) {
  const uint32_t t = task.blockIdx.x;
  // the chunk's task map in scalar registers (every lane runs the same chunk)
  const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane(t) >> 6;
  const ChunkMap cm = chunk_map(S, task_args(S), c);
  uint32_t x, y, out;
  chunk_pixel(S, cm, t & 63u, &x, &y, &out);
  const uint32_t lb = (cm.lt << 4) | cm.blk;
  const bool in = x < S.width && y < S.height;  // edge tiles overhang the image
  cnt.primary += in;
  const bool tie_high = (S.flags & RT_FLAG_TIE_HIGH) != 0;

  // ---- the traced head: rt_kernel's frame, the winner's depth word kept ----
  uint32_t hz;
  const int32_t hit = primary_z(S, lb, x, y, in, tie_high, cnt, &hz);
  cnt.hits += hit >= 0;
  const int32_t spid = resolve_layers(S, x, y, in && hit < 0, hit, cnt);
  uint32_t color = shade_wave(S, spid, x, y, S.clear_color, cnt);
  if (rt_usgpr(S.flags) & RT_FLAG_SHADOWS) {
    Ray r;
    primary_dir(S, x, y, r);
    const float th = hit >= 0 ? plane_t(S, r, hit) : 0.0f;
    const bool shadow = hit >= 0 && secondary_ok(th);
    if (__ballot(shadow) != 0) {
      Ray s;
      shadow_ray(S, r, th, s);
      cnt.shadow += shadow;
      // the light-space lists when built, else the binary16 BVH4 as one packet
      const bool occ = rt_usgpr(S.slist_on) ? occluded_list(S, s, shadow, hit, cnt)
                                            : occluded_packet(walk_scene(S), s, shadow, hit, 1.0f, cnt);
      if (shadow && occ) {
        ++cnt.occluded;
        color = shadowed(color);
      }
    }
  }

  // ---- the ordered tail over (color, ds) ----
  // the raster pipeline's cleared depth/stencil word with the head winner's depth
  uint32_t ds = 0xff000000u | hz;
  const Tail T = tail_args(S);
  const uint2 oc = S.A.sld<uint2>(T.oidx + 8u * lb);  // first entry, count
  if (oc.y != 0) {
    // entry k's record and entry k + 1's pid are in registers when round k
    // starts; the round issues record k + 1 and pid k + 2 before its test
    // (the list carries RT_OLIST_PAD entries of a valid pid past its end)
    uint32_t pid = S.A.sld<uint32_t>(T.olist + 4u * oc.x);
    uint32_t pid_n = S.A.sld<uint32_t>(T.olist + 4u * oc.x + 4u);
    uint4 rec[4];
    S.A.sld_u4n<4>(T.ovtris + 64u * (pid - T.base), rec);
    uint32_t cur_dc = 0xffffffffu;
    OmWords om = {};
    gfx::DcState st = {};
    for (uint32_t k = 0; k < oc.y; ++k) {
      uint4 rec_n[4];
      S.A.sld_u4n<4>(T.ovtris + 64u * (pid_n - T.base), rec_n);
      const uint32_t pid_nn = S.A.sld<uint32_t>(T.olist + 4u * (oc.x + k) + 8u);
      const uint4 A = rec[0], B = rec[1], C = rec[2];
      // coverage: the Q15.16 edge functions inside the primitive's
      // covered-pixel rectangle (draw3d's binning rule, app/vis.cpp)
      const int32_t e0[3] = {(int32_t)A.x, (int32_t)A.y, (int32_t)A.z};
      const int32_t e1[3] = {(int32_t)A.w, (int32_t)B.x, (int32_t)B.y};
      const int32_t e2[3] = {(int32_t)B.z, (int32_t)B.w, (int32_t)C.x};
      const int32_t E0 = gfx::edge_eval(e0, x, y), E1 = gfx::edge_eval(e1, x, y),
                    E2 = gfx::edge_eval(e2, x, y);
      const bool cov = in && rect_in(C.y, x) && rect_in(C.z, y) && E0 >= 0 && E1 >= 0 && E2 >= 0;
      if (__ballot(cov) != 0) {  // wave-uniform
        gfx::Prim p;
        gfx::load_prim<true>(S.A, S.prims + 128u * pid, p);
        const uint32_t d = p.dc();
        if (d != cur_dc) {
          om = load_om(S.A, T.oms + 128u * d);
          st = gfx::load_dcstate<true>(S.A, S.dcs + 64u * d);
          cur_dc = d;
        }
        if (cov) {
          // the fragment's colour and depth word from the edge values, as the
          // raster pipeline shades it (one reciprocal for both)
          uint32_t z;
          const uint32_t fc = gfx::shade_edges(S.A, p, st, E0, E1, E2, &z);
          gfx::om_write(om_state(om), color, ds, fc, z);
        }
      }
      rec[0] = rec_n[0]; rec[1] = rec_n[1]; rec[2] = rec_n[2]; rec[3] = rec_n[3];
      pid = pid_n;
      pid_n = pid_nn;
    }
  }
  if (in) store_out(S, out, color);
}

}  // namespace

VX_MAIN(rt_kernel_arg_t, arg, RT_BLOCK_THREADS) {
  Counters cnt;
  Scene S = load_scene(arg, vx_launch_words);
  const int rc = vx_spawn_tasks(
      S.num_tasks, [&](const vx_task_t& task, const Scene* s) { kernel_body(task, *s, cnt); }, &S);
  // the head's rays, as rt_kernel counts them
  flush_rays(cnt);
  return rc;
}
