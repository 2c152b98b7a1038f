// rt_kernel.hip -- the north-star hot path as a Vortex kernel program for
// gfx950: per-pixel primary rays resolved raster-exactly (trace_primary: the
// wave's 8x8 block scans its candidate list, or walks the tree as a packet;
// the draw3d fixed-point coverage + 24-bit depth test decide), screen layers,
// draw3d-exact shading of the winner, and an any-hit Möller–Trumbore shadow
// ray per geometry hit, with the shadow rays compacted into full waves
// (ballot + mbcnt into an LDS queue).  A full queue of shadow rays is traced
// per lane over each ray's light-space cell list (occluded_list) when the
// lists are built -- the default -- or as one packet walking the binary16
// BVH4 (occluded_packet).  Image rt_bvh (RT_BVH_WALK) keeps only the BVH
// walks: the packet walk of the tree for primary visibility and the shadow
// packet (BASELINE config 3's "full BVH traversal").
//
// Launched by libvortex-hip.so (vx_start) as its entry (VX_ENTRY); the body
// reads its rt_kernel_arg_t from the STARTUP_ARG DCRs and calls
// vx_spawn_tasks_ex() with one task per pixel (64 consecutive tasks = one
// wave = an 8x8 pixel block, 16 waves = one 32x32 raster tile, the
// reference's tile unit).  The node-visit / triangle-test counts of the
// RT_INSTRUMENT image are exactly the traversal work the oracle (oracle/rt.c)
// restates, the basis of the algorithmic byte count of SURVEY.md 8(d).
//
// Scene reads are buffer loads through one arena descriptor (vx_arena):
// 32-bit offsets, no FLAT loads.  Numerics are bit-identical to the oracle:
// every fused multiply-add is an explicit fmaf, everything else is compiled
// with -ffp-contract=off, divisions are IEEE.
//
// Images (Makefile): rt_kernel (binary16 BVH4 only), rt_bvh (the same
// without the list code paths), rt_kernel_deep (every
// BVH layout: per-lane walks with a 32-entry LDS stack for the layouts the
// packet walk does not read), rt_lights (RT_LIGHTS: rt_kernel lit by the
// lights of a table, every queued shadow ray against each of them in one
// drain), pt_primary (RT_PATHQ).  BASELINE config 2, the flat geometry list
// with no BVH, is a kernel of its own: rt_flat_kernel.hip.
#include <hip/hip_runtime.h>

#ifndef RT_BLOCK_THREADS
#define RT_BLOCK_THREADS 64
#endif
#define VX_BLOCK_THREADS RT_BLOCK_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "rt_trace.h"

// 1 (rt_lights, rt_lights_stats): a frame lit by the lights of the table behind the argument
// block (rt_common.h rt_lights_arg_t), every queued shadow ray tested against each of them in
// one drain (shadow_drain)
#ifndef RT_LIGHTS
#define RT_LIGHTS 0
#endif
#ifndef RT_PATHQ
#define RT_PATHQ 0  // 1: image pt_primary, the path tracer's first kernel (rt_trace.h pathq_append)
#endif
// 1 (rt_kernel, rt_kernel_stats): a launch with a tag deals its workgroups in a geometry and a
// background tier (bg_tier below)
#ifndef RT_BG_TIER
#define RT_BG_TIER 0
#endif
// 1 (RT_KERNEL_DEFS): a background-tier wave of rt_kernel takes its chunk's layer and drawcall
// from the setup's table (rt_common.h rt_bglayer_t) instead of resolving the layers per lane
// (RT_BG_TABLE).  The instrumented image keeps the layer loop -- its layer_tests count the
// records a wave fetched -- and so do the several-lights images, which are not judged on
// overlapped background chunks and stay byte for byte what they were.
#ifndef RT_BG_LAYERS
#define RT_BG_LAYERS 0
#endif
#if RT_BG_LAYERS && !RT_BG_TIER
#error "RT_BG_LAYERS is for the background tier"
#endif
#if RT_BG_LAYERS && !defined(RT_INSTRUMENT) && !RT_LIGHTS
#define RT_BG_TABLE 1
#else
#define RT_BG_TABLE 0
#endif
// 1 (RT_KERNEL_IMG_DEFS: rt_kernel and its A/B variants; the stamp image): under RT_FLAG_FUSED a wave
// traces its last chunk's shadow rays in place, around its shading's loads (fused_planes / fused_header / fused_verdict below)
#ifndef RT_FUSED_CHUNK
#define RT_FUSED_CHUNK 0
#endif
#if RT_FUSED_CHUNK && (RT_LIGHTS || RT_PATHQ || RT_BVH_WALK || !RT_ONLY_BVH4H)
#error "RT_FUSED_CHUNK is for the one-light primary+shadow list image on the binary16 BVH4"
#endif
#if RT_LIGHTS && (RT_PATHQ || RT_BVH_WALK || !RT_ONLY_BVH4H)
#error "RT_LIGHTS is for the primary+shadow list image on the binary16 BVH4"
#endif
#if RT_BG_TIER && (RT_PATHQ || RT_BVH_WALK || !RT_CHUNK_DESC)
#error "RT_BG_TIER is for the primary+shadow list image with the chunk descriptor table"
#endif

namespace {

using namespace rtk;

constexpr int kWaves = RT_BLOCK_THREADS / 64;

// Wave-private LDS: the compaction queue of deferred shadow rays, and the
// per-lane walks' stack[depth][lane] (deep images: layouts other than the
// binary16 BVH4 walk per lane)
#define RT_QUEUE 128
// (queued shadow rays walking the BVH per lane instead of as one packet:
// BVH-walk frame 0.0411 vs 0.0333 ms, r05n -- 102 VGPRs, 4 waves per SIMD)
#define RT_LANE_STACK (!RT_ONLY_BVH4H)
struct WaveLds {
#if RT_LANE_STACK
  int32_t stack[RT_STACK_ROWS][64];
#define RT_WSTACK(w, lane) (&(w).stack[0][(lane)])
#else
#define RT_WSTACK(w, lane) ((int32_t*)nullptr)
#endif
  uint32_t q_out[RT_QUEUE];  // framebuffer word (chunk_pixel)
  uint32_t q_xy[RT_QUEUE];   // pixel x | y << 16
  float q_t[RT_QUEUE];
  int32_t q_pid[RT_QUEUE];
  uint32_t q_color[RT_QUEUE];
  uint32_t q_count;
};

#if RT_FUSED_CHUNK
// vx_spawn_chunks_ex (vx_spawn.h) over the chunks [0, c1), handing kernel_func each chunk's place
// in the wave's deal: the wave takes every nw-th chunk, so chunk c is its last when c + nw >= c1.
// From the loop's own registers: nothing is read and nothing more is held across the chunks.
struct ChunkPlace {
  bool last;
};
template <typename F, typename E, typename Arg>
__device__ __forceinline__ int spawn_chunks_placed(uint32_t num_tasks, uint32_t c1, uint32_t w, uint32_t nw,
                                                   F kernel_func, E epilogue, Arg* arg) {
  __vx_declare_tasks(num_tasks);
  const uint32_t nchunks = (num_tasks + VX_CHUNK - 1) / VX_CHUNK;
  if (c1 > nchunks) c1 = nchunks;
  uint32_t ran = 0;
  vx_task_t task;
  task.threadIdx.x = task.threadIdx.y = task.threadIdx.z = 0;
  task.blockIdx.y = task.blockIdx.z = 0;
  // (the wave's index as a scalar: the chunk loop is a scalar loop and a chunk's place a scalar
  // compare, no lane mask kept across the body)
  for (uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane(w); c < c1; c += nw) {
    const uint32_t t = c * VX_CHUNK + (threadIdx.x & 63u);
    if (t < num_tasks) {
      task.task_id = t;
      task.blockIdx.x = t;
      ChunkPlace cp;
      cp.last = c + nw >= c1;
      kernel_func(task, cp, arg);
      ++ran;
    }
    // (behind the wave's last chunk the final drain below is this one and more: the same rounds)
    if (c + nw < c1) epilogue(false, arg);
  }
  epilogue(true, arg);
  vx_mpm_add(VX_MPM_TASKS, ran);
  return 0;
}

// A wave's last chunk with the light-space lists on: from block_primary's
// winners on, the colour (layers, primitive record, drawcall record, texels) and the shadow
// verdict (plane record, cell header, list records) do not depend on each other, and the chunk's
// rays go nowhere but through this wave -- so kernel_body traces them in place, per lane, their
// loads issued around the shading's instead of after a trip through the LDS queue:
//   fused_planes  the winners' plane records, issued before the layer loop;
//   fused_header  behind the layers: th, the shadow ray and its cell from the Ray and x, y the wave
//                 holds, and the cell header (off, n: one 8-byte load) issued ahead of shade_wave's
//                 records and taps.  Vector loads return in order: the wait for the taps covers it;
//   fused_verdict behind the shade: the scan as occluded_list runs it (slist_scan) and the pixel's
//                 one store.
// The layers and the shade are kernel_body's own, one copy for both ways through a chunk (a second
// copy of them for this path: 32 SGPR spills against the parent's 26).  Across the shade a lane
// keeps its segment and the header, eight VGPRs.  Pixels and the ray counters are those of
// kernel_body + shadow_drain.
struct FusedRay {
  float o[3], d[3];  // the shadow segment (shadow_ray)
  uint2 hd;          // its cell's off, n; n = 0: no ray, or an empty cell -- nothing to scan
};
struct PlaneRec {
  float4 a, b, c;
};
__device__ __forceinline__ PlaneRec fused_planes(const Scene& S, int32_t hit) {
  PlaneRec P;
  P.a = P.b = P.c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (hit >= 0) {
    const uint32_t o = S.ptris + 48u * (uint32_t)hit;
    P.a = S.A.ld_f4(o);
    P.b = S.A.ld_f4(o + 16);
    P.c = S.A.ld_f4(o + 32);
  }
  return P;
}
__device__ __forceinline__ FusedRay fused_header(const Scene& S, uint32_t x, uint32_t y, int32_t hit,
                                                 const PlaneRec& P, Counters& cnt) {
  FusedRay f;
  Ray r, s;
  primary_dir(S, x, y, r);
  const float th = hit >= 0 ? plane_t(r, P.a, P.b, P.c) : 0.0f;
  const bool shadow = hit >= 0 && secondary_ok(th);
  shadow_ray(S, r, th, s);
  f.hd = make_uint2(0u, 0u);
  if (shadow) f.hd = S.A.ld_u2(S.sidx + 8u * slist_cell(s, S.slist_n));
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    f.o[k] = s.o[k];
    f.d[k] = s.d[k];
  }
  cnt.shadow += shadow;
  return f;
}
__device__ __forceinline__ void fused_verdict(const Scene& S, uint32_t x, uint32_t y, uint32_t out, bool in,
                                              int32_t hit, FusedRay f, uint32_t color, Counters& cnt) {
  if (f.hd.y != 0u) {
    Ray s;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      s.o[k] = f.o[k];
      s.d[k] = f.d[k];
    }
    if (slist_scan(S, s, hit, cnt, S.slist, f.hd.x, f.hd.y)) {
      ++cnt.occluded;
      color = shadowed(color);
    }
  }
  if (in) store_out(S, out, color);
}
#endif

#if RT_FUSED_CHUNK
// (cp: the chunk's place in the wave's deal)
#define RT_BODY_DEAL , const ChunkPlace &cp
// (a wave-uniform word of the body tested where it stands, rt_usgpr: hoisted out of the chunk loop and
// kept as lane masks, these tests were SGPR spills the image with the fused path has no room for;
// the other images keep their code)
#define RT_BODY_U(v) rt_usgpr(v)
#else
#define RT_BODY_DEAL
#define RT_BODY_U(v) (v)
#endif
__device__ __forceinline__ void kernel_body(const vx_task_t& task, const Scene& S, WaveLds& w,
                                            Counters& cnt RT_BODY_DEAL) {
  const uint32_t t = task.blockIdx.x;
  // the chunk's task map in scalar registers (every lane runs the same chunk)
  const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane(t) >> 6;
  uint32_t x, y, out;
#if RT_CHUNK_DESC && !RT_BVH_WALK
  // a chunk of the whole-block tier with the setup's descriptor table: the
  // block's origin, lane 0's framebuffer word and the list header in one
  // scalar load; other tiers, or no table: chunk_map and the bidx load
  uint2 oc = make_uint2(0u, 0u);
  if (RT_BODY_U(S.cdesc) != 0 && c >= S.cdesc_first) {
    const uint4 d = S.A.sld_u4(S.cdesc + 16u * (c - S.cdesc_first));
    uint32_t ln = t & 63u;
    asm volatile("" : "+v"(ln));  // worked out here: hoisted out of the chunk loop its parts spill
    x = (d.x & 0xffffu) + (ln & 7u);
    y = (d.x >> 16) + (ln >> 3);
    out = d.y + (ln >> 3) * (d.w >> 16) + (ln & 7u);
    oc = make_uint2(d.z, d.w & 0xffffu);
  } else {
    const ChunkMap cm = chunk_map(S, task_args(S), c);
    uint32_t cx, cy, co;
    chunk_pixel(S, cm, t & 63u, &cx, &cy, &co);
    x = cx;
    y = cy;
    out = co;
    if (RT_BODY_U(S.blist_blocks)) oc = block_header(S, (cm.lt << 4) | cm.blk);
  }
#else
  const ChunkMap cm = chunk_map(S, task_args(S), c);
  chunk_pixel(S, cm, t & 63u, &x, &y, &out);
  const uint32_t lb = (cm.lt << 4) | cm.blk;
#endif
  const bool in = x < S.width && y < S.height;  // edge tiles overhang the image
  cnt.primary += in;
  const bool tie_high = (RT_BODY_U(S.flags) & RT_FLAG_TIE_HIGH) != 0;
#ifdef RT_STAMPS
  if (lane_id() == 0) __vx_mpm_lds[3] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
  // primary visibility: the raster's winner at this pixel
#if RT_CHUNK_DESC && !RT_BVH_WALK
  int32_t hit;
  if (RT_BODY_U(S.blist_blocks)) {
    hit = block_primary(S, oc, x, y, in, tie_high, cnt);
  } else {  // no lists: the packet walk of the tree (trace_primary)
    const int32_t h = trace_primary_packet(walk_scene(S), x, y, in, tie_high, cnt);
    hit = in ? h : -1;
  }
#else
  const int32_t hit = trace_primary(S, lb, x, y, in, tie_high, cnt);
#endif
#ifdef RT_STAMPS
  if (lane_id() == 0) __vx_mpm_lds[14] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
  cnt.hits += hit >= 0;
#if RT_FUSED_CHUNK
  // wave-uniform: the frame's flag and shadows, lists that hold for this frame's light (load_scene
  // clears slist_on under RT_LW_NO_SLIST), the wave's last chunk; an earlier chunk's rays, still
  // queued, are drained behind it as ever
  const bool fused = (rt_usgpr(S.flags) & (RT_FLAG_FUSED | RT_FLAG_SHADOWS)) == (RT_FLAG_FUSED | RT_FLAG_SHADOWS) &&
                     rt_usgpr(S.slist_on) && cp.last;
  PlaneRec P;
  if (fused) P = fused_planes(S, hit);
#endif
  const int32_t spid = resolve_layers(S, x, y, in && hit < 0, hit, cnt);
#ifdef RT_STAMPS
  if (lane_id() == 0) __vx_mpm_lds[4] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
#if RT_FUSED_CHUNK
  FusedRay fr;
  if (fused) fr = fused_header(S, x, y, hit, P, cnt);
#endif
  uint32_t color = shade_wave(S, spid, x, y, S.clear_color, cnt);
#ifdef RT_STAMPS
  if (lane_id() == 0) __vx_mpm_lds[11] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
#if RT_FUSED_CHUNK
  if (fused) {
    fused_verdict(S, x, y, out, in, hit, fr, color, cnt);
#ifdef RT_STAMPS
    if (lane_id() == 0) __vx_mpm_lds[5] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
    return;
  }
#endif
  Ray r;
  primary_dir(S, x, y, r);
  const float th = hit >= 0 ? plane_t(S, r, hit) : 0.0f;
#if RT_PATHQ
  // path tracing, first kernel: a path starts at the winner's plane; its
  // pixel is written by pt_queue when the path ends
  const bool path = hit >= 0 && secondary_ok(th);
  pathq_append(S, path, t, th, hit, color);
  if (in && !path) store_out(S, out, color);
  (void)w;
  return;
#endif
  const bool shadow = hit >= 0 && secondary_ok(th) && (rt_usgpr(S.flags) & RT_FLAG_SHADOWS) != 0;
  // wave64 compaction: lanes with a pending shadow ray append it to the
  // wave's LDS queue at ballot/mbcnt-assigned slots
  const uint64_t m = __ballot(shadow);
  if (m) {
    const uint32_t base = w.q_count;
    if (shadow) {
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi(
          (uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      const uint32_t slot = base + rank;
      w.q_out[slot] = out;
      w.q_xy[slot] = x | (y << 16);
      w.q_t[slot] = th;
      w.q_pid[slot] = hit;
      w.q_color[slot] = color;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane_id() == 0) w.q_count = base + (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
  }
  if (in && !shadow) store_out(S, out, color);
#ifdef RT_STAMPS
  if (lane_id() == 0) __vx_mpm_lds[5] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
}

// Called by all 64 lanes after every chunk: trace full waves of 64 shadow
// rays while the queue holds >= 64 (or whatever is left at the end).
__device__ __forceinline__ void shadow_drain(bool final, const Scene& S, WaveLds& w,
                                             Counters& cnt) {
#ifdef RT_STAMPS
  if (final && lane_id() == 0) __vx_mpm_lds[15] = (uint32_t)__builtin_amdgcn_s_memrealtime();
  if (final && lane_id() == 0) __vx_mpm_lds[8] = w.q_count;  // the final drain's shadow rays
  if (!final && w.q_count >= 64 && lane_id() == 0)
    __vx_mpm_lds[6] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
  if (!(rt_usgpr(S.flags) & RT_FLAG_SHADOWS)) return;
  const uint32_t lane = lane_id();
  uint32_t n = w.q_count;
  const bool tie_high = (S.flags & RT_FLAG_TIE_HIGH) != 0;
  while (n >= 64 || (final && n > 0)) {
    const uint32_t take = n < 64 ? n : 64;
    const uint32_t base = n - take;
    const bool active = lane < take;
    const uint32_t slot = base + lane;  // < RT_QUEUE for every lane
    const uint32_t xy = w.q_xy[slot];
#if RT_LIGHTS
    // the packet against every light of the table in turn (a wave-uniform loop: the table is
    // read through the scalar cache); a lane some light does not see stays in the packet for
    // the lights after it, so each light's packet holds the rays of that light's own frame.
    // o = the lights that do not see the lane's ray: its pixel is the rounded mean of the
    // single-light frames' values (rt_common.h rt_lights_mix), stored once
    Ray p;
    primary_dir(S, xy & 0xffffu, xy >> 16, p);
    const float th = w.q_t[slot];
    const int32_t pid = w.q_pid[slot];
    const auto* LA = lights_args(S);
    const uint32_t nl = LA->count, sn = LA->slist_n;
    uint32_t o = 0;
    for (uint32_t i = 0; i < nl; ++i) {
      const float L[3] = {LA->l[i].light[0], LA->l[i].light[1], LA->l[i].light[2]};
      Ray s;
      shadow_ray(S, p, th, s, L);
      cnt.shadow += active;
      const bool occ = LA->l[i].slist_on ? occluded_list(S, s, active, pid, cnt, (uint32_t)LA->l[i].sidx_addr,
                                                         (uint32_t)LA->l[i].slist_addr, sn)
                                         : occluded_packet(walk_scene(S), s, active, pid, 1.0f, cnt);
      o += occ ? 1u : 0u;
    }
    cnt.occluded += o;
    if (active) store_out(S, w.q_out[slot], rt_lights_mix(w.q_color[slot], o, nl));
    (void)tie_high;
#else
    Ray p, s;
    primary_dir(S, xy & 0xffffu, xy >> 16, p);
    shadow_ray(S, p, w.q_t[slot], s);
    cnt.shadow += active;
    uint32_t color = w.q_color[slot];
    float ts;
    // the light-space lists when built (occluded_list), else the BVH: the
    // binary16 BVH4 as one packet, other layouts per lane (deep images)
    const bool occ = !RT_BVH_WALK && rt_usgpr(S.slist_on) ? occluded_list(S, s, active, w.q_pid[slot], cnt)
                     : (RT_ONLY_BVH4H || (S.flags & RT_FLAG_BVH4H))
                         ? occluded_packet(walk_scene(S), s, active, w.q_pid[slot], 1.0f, cnt)
                         : active && trace<true>(walk_scene(S), s, 0.0f, 1.0f, w.q_pid[slot], tie_high, &ts,
                                                 RT_WSTACK(w, lane), cnt) >= 0;
    if (occ) {
      ++cnt.occluded;
      color = shadowed(color);
    }
    if (active) store_out(S, w.q_out[slot], color);
#endif
    n = base;
  }
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) w.q_count = n;
  __builtin_amdgcn_wave_barrier();
}

#if RT_BG_TIER
// The background tier.  A tiered launch (launch tag Tg
// != 0: the host's choice, runtime/bg_tier.h) deals its chunks in two ranges
// of the work order: workgroups [0, Tg) take the chunks of the tiles geometry
// reaches, [0, bg_first_chunk), through kernel_body as ever; the workgroups
// behind them take the chunks from bg_first_chunk on, whose block lists are
// all empty (the work order is heaviest tile first and bg_first_chunk = 16 *
// the tiles of weight > 0; a block with a list entry lies in a tile of weight
// > 0).  For such a chunk kernel_body finds no winner in any lane and queues
// no shadow ray: what it leaves is the layers, the shade and the store, which
// is all bg_tier runs -- the same functions on the same arguments, so pixels
// and counters are those of kernel_body.  A code path of its own from the
// wave's first instruction on: the geometry path's scene load, chunk loop and
// queue never see it.
//
// The scene fields resolve_layers / shade_wave / store_out read, and the
// chunk table; everything else stays 0 and is dead.
__device__ __forceinline__ Scene load_scene_bg(const rt_kernel_arg_t* ga, const vx_launch_words_t& lw) {
  const auto* a = arg_entry(ga);
  Scene s;
  s.argp = (uint64_t)a;
  s.A = vx_arena::get();
  s.nodes = s.nodes4 = s.tris = s.ptris = s.geom = s.order = 0;
  s.vnodes = s.vtris = s.vgeom = s.num_vnodes = 0;
  s.num_nodes = s.num_nodes4 = s.num_geom = s.flags = 0;
  s.shard_index = s.shard_count = s.tiles_x = s.bounces = s.seed = s.split_tiles = s.split_log = 0;
  s.tiles_x_magic = 0;
  s.sx = s.sy = s.light[0] = s.light[1] = s.light[2] = 0.0f;
  s.blist = s.bidx = s.blist_blocks = 0;
  s.sidx = s.slist = s.slist_on = s.slist_n = 0;
  s.vlayers = (uint32_t)a->vlayers_addr;
  s.num_layer = a->num_layer_tris;
  s.prims = (uint32_t)a->prims_addr;
  s.dcs = (uint32_t)a->dcs_addr;
  s.cbuf = (uint32_t)a->cbuf_addr;
  s.width = a->width;
  s.height = a->height;
  s.clear_color = a->clear_color;
  s.num_tasks = a->num_tasks;
  s.cdesc = (uint32_t)a->cdesc_addr;
  s.cdesc_first = a->cdesc_first;
  s.lw3 = lw.w[3];
  return s;
}

__device__ __forceinline__ arg_ptr<rt_tier_arg_t> tier_arg(const rt_kernel_arg_t* ga) {
  return arg_entry<rt_tier_arg_t>(ga, RT_TIER_ARG_OFFSET);
}
__device__ __forceinline__ uint32_t bg_first_chunk(const rt_kernel_arg_t* ga) { return tier_arg(ga)->bg_first_chunk; }

// A background-tier wave: wave (blockIdx.x - tg) * kWaves + its index in the
// workgroup of the (gridDim.x - tg) * kWaves that share the chunks
// [bg_first_chunk, chunks).  No LDS, no queue, no drain.
__device__ __forceinline__ void bg_tier(const rt_kernel_arg_t* arg, uint32_t tg, const vx_launch_words_t& lw) {
  const Scene S = load_scene_bg(arg, lw);
  Counters cnt;
  const uint32_t nchunks = (S.num_tasks + VX_CHUNK - 1) / VX_CHUNK;
  const uint32_t nw = (gridDim.x - tg) * kWaves;  // (blockIdx.x >= tg: at least kWaves)
  uint32_t ran = 0;
  // (the wave's index as a scalar: the chunk loop is a scalar loop, no exec mask kept across it)
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t c0 = bg_first_chunk(arg);
#if RT_BG_TABLE
  const uint32_t bgl = (uint32_t)tier_arg(arg)->bglayer_addr;  // 0: no table (env RT_BG_LAYERS=0)
#endif
  for (uint32_t c = c0 + (blockIdx.x - tg) * kWaves + wv; c < nchunks; c += nw) {
    const uint32_t ln = threadIdx.x & 63u;
    if (c * VX_CHUNK + ln < S.num_tasks) {
      const uint4 d = S.A.sld_u4(S.cdesc + 16u * (c - S.cdesc_first));
#if RT_BG_TABLE
      // the chunk's layer from the table, its load in flight with the descriptor's (both addresses
      // follow from c): a block under one layer primitive -- all 64 pixels inside the image --
      // skips the layer loop and hands shade_wave that pid in every lane and its drawcall, so the
      // primitive's and the drawcall's records load together; a block under no layer shades
      // nothing and stores the clear colour; entry 0 (mixed, or over the image's edge) runs the
      // layer loop.  (A shade site of its own here, without shade_wave's ballots: 69 SGPR spills
      // against 26, and the frame rendered alone 3 % slower -- DESIGN.md 4.1 r18.)
      uint2 e = make_uint2(0u, 0u);
      if (bgl != 0) e = S.A.sld<uint2>(bgl + 8u * (c - c0));
#endif
      const uint32_t x = (d.x & 0xffffu) + (ln & 7u);
      const uint32_t y = (d.x >> 16) + (ln >> 3);
      const uint32_t out = d.y + (ln >> 3) * (d.w >> 16) + (ln & 7u);
      const bool in = x < S.width && y < S.height;
      cnt.primary += in;
#if RT_BG_TABLE
      int32_t spid = (int32_t)e.x - 1;  // (RT_BGLAYER_NONE: -2, nothing to shade)
      uint32_t kdc = e.y;
      if (e.x == 0) {
        spid = resolve_layers(S, x, y, in, -1, cnt);
        kdc = RT_NO_DC;
      }
      const uint32_t color = shade_wave(S, spid, x, y, S.clear_color, cnt, kdc);
#else
      const int32_t spid = resolve_layers(S, x, y, in, -1, cnt);
      const uint32_t color = shade_wave(S, spid, x, y, S.clear_color, cnt);
#endif
      if (in) store_out(S, out, color);
      ++ran;
    }
  }
  vx_mpm_add(VX_MPM_TASKS, ran);
  flush(RT_STAT_PRIMARY, cnt.primary);
#ifdef RT_INSTRUMENT
  flush(RT_STAT_LAYER_TESTS, cnt.layer_tests);
  flush(RT_STAT_SHADED, cnt.shaded);
  flush(RT_STAT_TEXEL_BYTES, cnt.texel_bytes);
#endif
}
#endif

}  // namespace

// primary + shadow images: registers for 7 waves per SIMD (<= 72 VGPRs: 67,
// 22 SGPR spills) -- A/B on the light-space-list image (r03g, same frames):
// 5 (71 VGPRs, 6-7 resident) 0.02574 ms, 7 0.02470, 8 (64 VGPRs, 39 SGPR
// spills) 0.02532: the frame is latency-bound with the chip full of waves
// (DESIGN 4.1), so more resident waves win until the spills cost more.
// (r02: capping occupancy lower with LDS padding cost +27 / +80 %.)  The
// deep images (every layout, 32-entry stack) keep the compiler's choice.
// The BVH-walk image (rt_bvh: packet walks, no lists) is better at 5
// (A/B r04f: 5 0.03644 ms, 6 0.03676, 7 0.03768, 8 0.03752).
#if !defined(RT_WAVES_PER_EU) && RT_ONLY_BVH4H
#if RT_BVH_WALK
#define RT_WAVES_PER_EU 5
#else
#define RT_WAVES_PER_EU 7
#endif
#endif
#ifdef RT_WAVES_PER_EU
VX_MAIN_OCC(rt_kernel_arg_t, arg, RT_BLOCK_THREADS, RT_WAVES_PER_EU) {
#else
VX_MAIN(rt_kernel_arg_t, arg, RT_BLOCK_THREADS) {
#endif
#if RT_BG_TIER
  // a tiered launch (tag = its geometry-tier workgroups): the workgroups behind them run the
  // background tier and nothing of what follows
  if (vx_launch_tag != 0 && blockIdx.x >= vx_launch_tag) {
    bg_tier(arg, vx_launch_tag, vx_launch_words);
    return 0;
  }
#endif
  __shared__ WaveLds s_wave[kWaves];
  WaveLds& w = s_wave[threadIdx.x >> 6];
#ifdef RT_STAMPS
  const uint64_t t_stamp0 = __builtin_amdgcn_s_memrealtime();
#endif
  Counters cnt;
  Scene S = load_scene(arg, vx_launch_words);
#ifdef RT_STAMPS
  if (threadIdx.x == 0) __vx_mpm_lds[10] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
  if ((threadIdx.x & 63u) == 0) w.q_count = 0;
  __builtin_amdgcn_wave_barrier();
#if RT_BG_TIER
  // the geometry tier of a tiered launch: its tag's workgroups share the chunks below
  // bg_first_chunk; tag 0: the grid's waves share every chunk, vx_spawn_tasks_ex's deal
  const uint32_t tier_wgs = vx_launch_tag != 0 ? vx_launch_tag : gridDim.x;
  const uint32_t tier_end = vx_launch_tag != 0 ? bg_first_chunk(arg) : 0xffffffffu;
#endif
#if RT_FUSED_CHUNK
  // the same deals, each chunk with its place in the wave's
#if RT_BG_TIER
  const uint32_t deal_w = blockIdx.x * kWaves + (threadIdx.x >> 6), deal_nw = tier_wgs * kWaves, deal_end = tier_end;
#else
  const uint32_t deal_w = __vx_logical_block() * kWaves + (threadIdx.x >> 6), deal_nw = gridDim.x * kWaves,
                 deal_end = 0xffffffffu;
#endif
  const int rc = spawn_chunks_placed(
      S.num_tasks, deal_end, deal_w, deal_nw,
      [&](const vx_task_t& task, const ChunkPlace& cp, const Scene* s) { kernel_body(task, *s, w, cnt, cp); },
      [&](bool final, const Scene* s) { shadow_drain(final, *s, w, cnt); }, &S);
#elif RT_BG_TIER
  const int rc = vx_spawn_chunks_ex(
      S.num_tasks, 0u, tier_end, blockIdx.x * kWaves + (threadIdx.x >> 6), tier_wgs * kWaves,
      [&](const vx_task_t& task, const Scene* s) { kernel_body(task, *s, w, cnt); },
      [&](bool final, const Scene* s) { shadow_drain(final, *s, w, cnt); }, &S);
#else
  const int rc = vx_spawn_tasks_ex(
      S.num_tasks,
      [&](const vx_task_t& task, const Scene* s) { kernel_body(task, *s, w, cnt); },
      [&](bool final, const Scene* s) { shadow_drain(final, *s, w, cnt); }, &S);
#endif
#ifdef RT_STAMPS  // diagnostic image: per-wave phase timestamps
  if (threadIdx.x == 0) {
    // 12: start, 13: end, 14: primary traced, 15: shadow drain begins
    // (low 32 bits of s_memrealtime, 100 MHz)
    __vx_mpm_lds[12] = (uint32_t)t_stamp0;
    __vx_mpm_lds[13] = (uint32_t)__builtin_amdgcn_s_memrealtime();
  }
#endif
#ifndef RT_STAMPS  // the stamp image keeps slots 3-9 for phase stamps / iteration counts
  flush_rays(cnt);
#endif
#ifdef RT_INSTRUMENT
  flush(RT_STAT_NODE_VISITS, cnt.visits);
  flush(RT_STAT_TRI_TESTS, cnt.tests);
  flush(RT_STAT_LAYER_TESTS, cnt.layer_tests);
  flush(RT_STAT_SHADED, cnt.shaded);
  flush(RT_STAT_TEXEL_BYTES, cnt.texel_bytes);
#endif
  return rc;
}

