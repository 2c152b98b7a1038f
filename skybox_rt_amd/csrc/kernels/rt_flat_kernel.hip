// rt_flat_kernel.hip -- BASELINE config 2 as a Vortex kernel program for
// gfx950: the primary+shadow frame over the flat geometry list, no BVH (images
// rt_flat / rt_flat_stats, and the flatstamp diagnostic pair).  Per pixel what
// rt_kernel.hip resolves -- raster-exact primary visibility (the draw3d
// fixed-point coverage + 24-bit depth test), screen layers, draw3d-exact
// shading of the winner and an any-hit Möller–Trumbore shadow ray per geometry
// hit -- with every ray's primitive list split across the waves of a 512-thread
// workgroup (flat_chunk) instead of a walk per wave; rt_trace.h holds the
// pieces shared with the other RT kernel programs.  Launched like rt_kernel.hip
// (VX_ENTRY, rt_kernel_arg_t), with the same numerics rules.
#include <hip/hip_runtime.h>

#ifndef RT_BLOCK_THREADS
#define RT_BLOCK_THREADS 64
#endif
#define VX_BLOCK_THREADS RT_BLOCK_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "rt_trace.h"

namespace {

using namespace rtk;

constexpr int kWaves = RT_BLOCK_THREADS / 64;

// Config 2 reads the geometry list straight from L2: the block test reads
// 64 rectangle words per instruction with vector loads, so a workgroup
// starts on its chunk at once (r05j, 256^2, median ms: the rectangle words
// staged in LDS 0.0101, unstaged 0.0096, unstaged with 512-thread workgroups
// at 8 waves per SIMD 0.0090; r02: whole 64-B records in LDS 0.0479).  The
// shadow rays read the MT records (rt_tri_t) of S.geom.
//
// Every ray's primitive list is split across the workgroup's waves: a
// workgroup step takes one 64-task chunk (vx_spawn_chunks_block),
// wave w tests the list entries w, w + kWaves, ... for the chunk's 64
// pixels (flat_chunk), the per-wave winners meet in LDS (vis_better is a
// strict order on (depth word, pid), so the reduction order is immaterial)
// and wave 0 shades and stores; shadow rays split the list in ranges, the
// first occluder in list order found by a min over the waves' first hits
// (which is also brute_trace's test count).
// Without shadow rays waves 1.. leave the chunk once their winners are in
// LDS and wave 0 shades and stores with no second barrier -- the winners
// double-buffered by chunk parity, so a wave's next chunk never overwrites
// words wave 0 is still reducing (it must pass the next chunk's barrier,
// which wave 0 reaches only after its reduction)
struct FlatLds {
  uint32_t z[2][kWaves][64];
  int32_t pid[2][kWaves][64];
  uint32_t first[kWaves][64];
};

// a record's rectangle word with its rectangle as packed corners (lo = x0 |
// y0 << 16, hi = x1 | y1 << 16 in .y / .z; an empty rectangle becomes
// lo = 0xffffffff, hi = 0xfffefffe, which no pixel matches), so a wave's
// rectangle test is two packed 16-bit clamps and one compare (rect2_in)
__device__ __forceinline__ uint4 rect_corners(uint4 c) {
  const uint32_t rx = c.y, ry = c.z;
  const bool empty = (rx & 0xffffu) > (rx >> 16) || (ry & 0xffffu) > (ry >> 16);
  c.y = empty ? 0xffffffffu : (rx & 0xffffu) | (ry << 16);
  c.z = empty ? 0xfffefffeu : (rx >> 16) | (ry & 0xffff0000u);
  return c;
}
__device__ __forceinline__ void flat_chunk(const vx_task_t& task, bool valid, const Scene& S,
                                           FlatLds& L, uint32_t& par, Counters& cnt) {
  const uint32_t w = threadIdx.x >> 6, lane = lane_id();
  const uint32_t pb = par;  // this chunk's winner buffer
  par ^= 1u;
  const uint32_t t = task.blockIdx.x;
  uint32_t x = 0, y = 0, out = 0;
  if (valid) {
    // the chunk's task map in scalar registers (block-uniform chunk)
    const ChunkMap cm = chunk_map(S, task_args(S), (uint32_t)__builtin_amdgcn_readfirstlane(t) >> 6);
    chunk_pixel(S, cm, t & 63u, &x, &y, &out);
  }
  const bool in = valid && x < S.width && y < S.height;
  const uint32_t px = in ? x : 0xffffffffu;  // outside every pixel rectangle
  const uint32_t pp = in ? x | (y << 16) : 0xffffffffu;  // packed pixel (rect_corners)
  const bool tie_high = (S.flags & RT_FLAG_TIE_HIGH) != 0;
  const uint32_t n = S.num_geom, per = (n + kWaves - 1) / kWaves;
  const uint32_t k0 = w * per < n ? w * per : n, k1 = k0 + per < n ? k0 + per : n;
  uint32_t bz = VX_OM_DEPTH_MASK;
  int32_t bp = -1;
  // Two levels: the wave's lanes take 64 of its entries at once and test
  // each one's rectangle against the chunk's 8x8 block (packed corners:
  // lo <= block hi and hi >= block lo, halfwise); then, for the entries that
  // reach the block only, the per-pixel rectangle test and, where a lane
  // lies in it, the edges and depth -- the records two at a time (one
  // 64-B scalar load each, the second in flight while the first is tested).
  // The same entries get the same tests as a one-level scan of every entry
  // per pixel (the block test only skips entries no pixel of the block lies
  // in): identical winners and counts, with 1/64 of the rectangle-test
  // instructions (r04).  Wave w takes entries w, w + kWaves, ...: a region's
  // triangles, often consecutive in the list, spread over the waves.
  {
    const uint32_t bx = (uint32_t)__builtin_amdgcn_readfirstlane(x) & ~7u;  // lane 0: the block's corner
    const uint32_t by = (uint32_t)__builtin_amdgcn_readfirstlane(y) & ~7u;
    const uint32_t blo = bx | (by << 16), bhi = (bx + 7u) | ((by + 7u) << 16);
    const uint32_t mine = w < n ? (n - w + kWaves - 1) / kWaves : 0u;  // this wave's entries
    for (uint32_t i = 0; i < mine; i += 64u) {
      const uint32_t il = i + lane;
      bool ov = false;
      if (il < mine) {
        const uint32_t kl = il * kWaves + w;
        const uint4 C = rect_corners(S.A.ld_u4(S.vgeom + 64u * kl + 32u));
        // max(lo, block hi) == block hi and min(hi, block lo) == block lo
        ov = rect2_clamp(C.y, 0xffffffffu, bhi) == bhi && rect2_clamp(0u, C.z, blo) == blo;
      }
      uint64_t m = __ballot(ov);
#ifdef RT_INSTRUMENT
      cnt.rect_tests += lane == 0 ? (mine - i < 64u ? mine - i : 64u) : 0u;
#endif
      while (m != 0) {
        const uint32_t j0 = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        const bool two = m != 0;
        const uint32_t j1 = two ? (uint32_t)__builtin_ctzll(m) : j0;
        if (two) m &= m - 1;
        const uint32_t ka = (i + j0) * kWaves + w, kb = (i + j1) * kWaves + w;
        uint4 ra[4], rb[4];
        S.A.sld_u4n<4>(S.vgeom + 64u * ka, ra);
        S.A.sld_u4n<4>(S.vgeom + 64u * kb, rb);
        const uint4 Ca = rect_corners(ra[2]), Cb = rect_corners(rb[2]);
        const bool ina = rect2_in(Ca.y, Ca.z, pp);
        if (__ballot(ina) != 0) {  // wave-uniform
#ifdef RT_INSTRUMENT
          cnt.edge_tests += lane == 0 ? 1u : 0u;
#endif
          vis_test_in(ra[0], ra[1], ra[2], ra[3], ina, px, y, tie_high, bz, bp);
        }
        const bool inb = two && rect2_in(Cb.y, Cb.z, pp);
        if (__ballot(inb) != 0) {
#ifdef RT_INSTRUMENT
          cnt.edge_tests += lane == 0 ? 1u : 0u;
#endif
          vis_test_in(rb[0], rb[1], rb[2], rb[3], inb, px, y, tie_high, bz, bp);
        }
      }
    }
#ifdef RT_INSTRUMENT
    cnt.tests += in ? mine : 0u;  // the whole list per ray, summed over the waves
#endif
  }
#ifdef RT_STAMPS  // 3: wave 0's list scan done, 4: the slowest wave's (after the barrier)
  if (threadIdx.x == 0) __vx_mpm_lds[3] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
  L.z[pb][w][lane] = bz;
  L.pid[pb][w][lane] = bp;
  __syncthreads();
#ifdef RT_STAMPS
  if (threadIdx.x == 0) __vx_mpm_lds[4] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
  const bool early = (S.flags & RT_FLAG_SHADOWS) == 0;  // block-uniform
  if (early && w != 0) return;
  int32_t hit = -1;
  uint32_t hz = VX_OM_DEPTH_MASK;
  for (uint32_t i = 0; i < kWaves; ++i) {
    const int32_t p = L.pid[pb][i][lane];
    if (p >= 0 && vis_better(L.z[pb][i][lane], p, hz, hit, tie_high)) {
      hz = L.z[pb][i][lane];
      hit = p;
    }
  }
  uint32_t color = 0;
  if (w == 0) {
    cnt.primary += in;
    cnt.hits += hit >= 0;
    const int32_t spid = resolve_layers(S, x, y, in && hit < 0, hit, cnt);
    color = shade_wave(S, spid, x, y, S.clear_color, cnt);
#ifdef RT_STAMPS  // 5: shaded (wave 0)
    asm volatile("" : : "v"(color));  // the colour is complete before the stamp
    if (threadIdx.x == 0) __vx_mpm_lds[5] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
  }
  if (early) {  // wave 0 only: no shadow rays, no second barrier
    if (in) store_out(S, out, color);
    return;
  }
  Ray r;
  primary_dir(S, x, y, r);
  const float th = hit >= 0 ? plane_t(S, r, hit) : 0.0f;
  const bool shadow = in && hit >= 0 && secondary_ok(th) && (S.flags & RT_FLAG_SHADOWS) != 0;
  if (__ballot(shadow)) {  // block-uniform: every wave holds the same 64 rays
    Ray sr;
    shadow_ray(S, r, th, sr);
    float ts;
    uint32_t first = 0xffffffffu;
    if (shadow) trace_flat_range<true>(S, sr, k0, k1, 0.0f, 1.0f, hit, tie_high, &ts, &first);
    L.first[w][lane] = first;
  }
  __syncthreads();
  if (w == 0) {
    if (shadow) {
      uint32_t first = 0xffffffffu;
      for (uint32_t i = 0; i < kWaves; ++i) first = L.first[i][lane] < first ? L.first[i][lane] : first;
      cnt.shadow += 1;
#ifdef RT_INSTRUMENT
      cnt.tests += first != 0xffffffffu ? first + 1 : n;  // brute_trace stops at the first occluder
#endif
      if (first != 0xffffffffu) {
        ++cnt.occluded;
        color = shadowed(color);
      }
    }
    if (in) store_out(S, out, color);
  }
}

}  // namespace

// config 2: 4 workgroups per CU (1 024: one per 256^2 chunk) -- A/B r04i:
// 0.01084 ms vs 0.01108 at 16/CU; registers for 8 waves per SIMD, so all
// 1 024 workgroups of 512 threads are resident at once (r05j)
__device__ __attribute__((used)) uint32_t __vx_grid_per_cu = 4;
#ifndef RT_WAVES_PER_EU  // (an A/B passing the macro keeps its value)
#define RT_WAVES_PER_EU 8
#endif
VX_MAIN_OCC(rt_kernel_arg_t, arg, RT_BLOCK_THREADS, RT_WAVES_PER_EU) {
#ifdef RT_STAMPS
  const uint64_t t_stamp0 = __builtin_amdgcn_s_memrealtime();
#endif
  Counters cnt;
  Scene S = load_scene(arg, vx_launch_words);
#ifdef RT_STAMPS
  if (threadIdx.x == 0) __vx_mpm_lds[10] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
  // the workgroup's waves start their first chunk together
  __syncthreads();
#ifdef RT_STAMPS  // 11: past the start barrier
  if (threadIdx.x == 0) __vx_mpm_lds[11] = (uint32_t)__builtin_amdgcn_s_memrealtime();
#endif
  __shared__ FlatLds s_flat;
  uint32_t par = 0;
  const int rc = vx_spawn_chunks_block(
      S.num_tasks,
      [&](const vx_task_t& task, bool valid, const Scene* s) { flat_chunk(task, valid, *s, s_flat, par, cnt); },
      &S);
#ifdef RT_STAMPS  // diagnostic image: per-workgroup phase timestamps (scripts/flat_timeline.py)
  if (threadIdx.x == 0) {
    // 12: start, 13: end (low 32 bits of s_memrealtime, 100 MHz)
    __vx_mpm_lds[12] = (uint32_t)t_stamp0;
    __vx_mpm_lds[13] = (uint32_t)__builtin_amdgcn_s_memrealtime();
  }
#endif
#ifndef RT_STAMPS  // the stamp image keeps slots 3-9 for phase stamps
  flush_rays(cnt);
#endif
#ifdef RT_INSTRUMENT
  flush(RT_STAT_NODE_VISITS, cnt.visits);
  flush(RT_STAT_TRI_TESTS, cnt.tests);
  flush(RT_STAT_LAYER_TESTS, cnt.layer_tests);
  flush(RT_STAT_SHADED, cnt.shaded);
  flush(RT_STAT_TEXEL_BYTES, cnt.texel_bytes);
  flush(RT_STAT_RECT_TESTS, cnt.rect_tests);
  flush(RT_STAT_EDGE_TESTS, cnt.edge_tests);
#endif
  return rc;
}
