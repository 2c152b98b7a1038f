// rt_aov_kernel.hip -- the per-pixel visibility records of a primary+shadow
// frame (vx_rt.h rt_render_aov_start, rt_aov_t): what rt_kernel resolves per
// pixel and drops at its store -- the shaded primitive, the winner's 24-bit
// depth word, the plane t its secondary rays start at, and per light whether
// the light sees the point -- written as one 16-byte record per framebuffer
// pixel, at the pixel's framebuffer index, into a buffer of the launch's own.
// No shading: no shade_wave, no texel reads, no shading-record traffic.
//
// One wave per 8x8 block on rt_kernel's task map (chunk_map / chunk_pixel:
// linear, compact and sharded output alike).  The pixel stays in its lane from
// the primary test to the store, so the shadow rays are traced in place under
// the lane mask (rt_om_kernel.hip's pattern), not through rt_kernel's LDS
// compaction queue: a wave-uniform loop over the lights in use, each light's
// ray on that light's own light-space lists (occluded_list) or, where a light
// has none, as one packet walking the binary16 BVH4 (occluded_packet).  The
// verdicts are the frames': both tests answer "any occluder on the segment".
//
// The lights in use: the launch's tag n.  n < 2: the argument block's light
// and lists under the launch words, exactly as a frame reads them (load_scene:
// RT_LW_LIGHT, RT_LW_NO_SLIST).  n >= 2: the first n entries of the light
// table behind the argument block (rt_common.h rt_lights_arg_t), read through
// the scalar cache.  The record buffer's address stands behind the table
// (rt_aov_arg_t).
//
// Image rt_aov (Makefile): the binary16 BVH4 only (RT_ONLY_BVH4H).
//
// Image rt_aov_base (RT_AOV_BASE=1; vx_rt.h rt_relight_capture_start): the same
// launch, the same records, and the pixel shaded without shadows -- shade_wave
// as rt_kernel calls it, the colour a frame of this configuration without
// RT_RENDER_SHADOWS stores -- written at the pixel's framebuffer index into the
// base-colour buffer (rt_common.h rt_relight_arg_t), for rt_relight_kernel.hip.
//
// Image rt_aov_guide (RT_AOV_BASE=2; vx_rt.h rt_denoise_capture_start): the
// denoiser's capture, launched under a path configuration's arguments -- the
// task map is the one pt_kernel deals its waves by (chunk_map / chunk_pixel:
// 32-pixel waves of split tiles leave their upper lanes off the image), and
// primary visibility, layers and shade_wave are what pt_kernel runs before it
// starts a path.  Per pixel the guide record {pid, depth word | RT_AOV_GEOM,
// geometric normal, 0} (rt_common.h rt_denoise_arg_t) in place of the
// visibility record, and the base colour; no shadow ray is traced.  A third
// build and not a launch of rt_aov_base: that image would trace one shadow ray
// per pixel for a mask nobody reads, and the normal would need a pass of its
// own over pid and the triangle records -- here the lane has the pid in hand.
#include <hip/hip_runtime.h>

#ifndef RT_BLOCK_THREADS
#define RT_BLOCK_THREADS 64
#endif
#ifndef RT_AOV_BASE
#define RT_AOV_BASE 0
#endif
#define VX_BLOCK_THREADS RT_BLOCK_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "rt_trace.h"

#if !RT_ONLY_BVH4H
#error "rt_aov_kernel.hip walks the binary16 BVH4 only (build with -DRT_ONLY_BVH4H=1)"
#endif

namespace {

using namespace rtk;

#if RT_AOV_BASE != 2
// the record buffer as an arena offset (rt_app checks it lies below 4 GiB)
__device__ __forceinline__ uint32_t aov_base(const Scene& S) {
  return (uint32_t)arg_at<rt_aov_arg_t>(S, RT_AOV_ARG_OFFSET)->aov_addr;
}
#endif

#if RT_AOV_BASE == 2
// the guide records and the base colours of the denoiser's capture, the same way
__device__ __forceinline__ uint32_t guide_records(const Scene& S) {
  return (uint32_t)arg_at<rt_denoise_arg_t>(S, RT_DENOISE_ARG_OFFSET)->guide_addr;
}
__device__ __forceinline__ uint32_t base_colours(const Scene& S) {
  return (uint32_t)arg_at<rt_denoise_arg_t>(S, RT_DENOISE_ARG_OFFSET)->base_addr;
}
// The guide normal of triangle `pid` (rt_tri_t by pid in ptris), three signed bytes packed
// x | y << 8 | z << 16: rt_path.h tri_normal's first three statements -- cross3, len =
// sqrtf(dot3(n, n)), n / len, no facing flip -- then rintf(n_i * 127); 0 when len is 0 or
// not finite.
__device__ __forceinline__ uint32_t guide_normal(const Scene& S, int32_t pid) {
  const uint32_t o = S.ptris + 48u * (uint32_t)pid;
  const float4 b = S.A.ld_f4(o + 16), c = S.A.ld_f4(o + 32);
  const float e1[3] = {b.x, b.y, b.z}, e2[3] = {c.x, c.y, c.z};
  float n[3];
  cross3(n, e1, e2);
  const float len = sqrtf(dot3(n, n));
  if (!(len > 0.0f && len < INFINITY)) return 0u;
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) v |= ((uint32_t)(int32_t)rintf((n[k] / len) * 127.0f) & 0xffu) << (8 * k);
  return v;
}
#elif RT_AOV_BASE
// the base-colour buffer, the same way
__device__ __forceinline__ uint32_t base_colours(const Scene& S) {
  return (uint32_t)arg_at<rt_relight_arg_t>(S, RT_RELIGHT_ARG_OFFSET)->base_addr;
}
#endif

#if RT_AOV_BASE != 2
// one light's verdict for the wave's shadow rays: true where the light does not see the lane's point
__device__ __forceinline__ bool light_occluded(const Scene& S, const Ray& p, float th, const float L[3],
                                               bool shadow, int32_t hit, uint32_t slist_on, uint32_t sidx,
                                               uint32_t slist, uint32_t slist_n, Counters& cnt) {
  Ray s;
  shadow_ray(S, p, th, s, L);
  cnt.shadow += shadow;
  const bool occ = rt_usgpr(slist_on) ? occluded_list(S, s, shadow, hit, cnt, sidx, slist, slist_n)
                                      : occluded_packet(walk_scene(S), s, shadow, hit, 1.0f, cnt);
  return shadow && occ;
}
#endif

__device__ __forceinline__ void kernel_body(const vx_task_t& task, const Scene& S, uint32_t nl, uint32_t aov,
                                            uint32_t base, Counters& cnt) {
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

  // primary visibility, the winner's depth word kept
  uint32_t hz;
  const int32_t hit = primary_z(S, lb, x, y, in, tie_high, cnt, &hz);
  cnt.hits += hit >= 0;
  const int32_t spid = resolve_layers(S, x, y, in && hit < 0, hit, cnt);
#if RT_AOV_BASE
  // the unshadowed pixel (lanes outside the image have spid < 0 and no store)
  const uint32_t color = shade_wave(S, spid, x, y, S.clear_color, cnt);
  if (in) S.A.st_u32(base + 4u * out, color);
#endif
#if RT_AOV_BASE == 2
  // the guide record: a geometry pixel's normal is its winner's (lanes without one read nothing)
  (void)nl;
  const uint32_t gn = hit >= 0 ? guide_normal(S, hit) : 0u;
  if (in) S.A.st_u4(aov + 16u * out, make_uint4((uint32_t)spid, hz | (hit >= 0 ? RT_AOV_GEOM : 0u), gn, 0u));
  return;
#else

  float th = 0.0f;
  uint32_t df = hz | (hit >= 0 ? RT_AOV_GEOM : 0u), mask = 0;
  if (__ballot(hit >= 0) != 0) {
    Ray r;
    primary_dir(S, x, y, r);
    th = hit >= 0 ? plane_t(S, r, hit) : 0.0f;
    const bool shadow = hit >= 0 && secondary_ok(th) && (rt_usgpr(S.flags) & RT_FLAG_SHADOWS) != 0;
    if (__ballot(shadow) != 0) {
      df |= shadow ? RT_AOV_SHADOW_RAY : 0u;
      if (nl < 2) {
        // (the scene's own light through the same call as a light of the table: written with the plain
        // shadow_ray / occluded_list overloads the branch compiles to other code)
        const float L[3] = {S.light[0], S.light[1], S.light[2]};
        mask = light_occluded(S, r, th, L, shadow, hit, S.slist_on, S.sidx, S.slist, S.slist_n, cnt) ? 1u : 0u;
      } else {
        // (a lane some light does not see stays in the packet for the lights after it)
        const auto* LA = lights_args(S);
        const uint32_t sn = LA->slist_n;
        for (uint32_t i = 0; i < nl; ++i) {
          const float L[3] = {LA->l[i].light[0], LA->l[i].light[1], LA->l[i].light[2]};
          const bool occ = light_occluded(S, r, th, L, shadow, hit, LA->l[i].slist_on, (uint32_t)LA->l[i].sidx_addr,
                                          (uint32_t)LA->l[i].slist_addr, sn, cnt);
          mask |= occ ? 1u << i : 0u;
        }
      }
      cnt.occluded += (uint32_t)__popc(mask);
    }
  }
  if (in) S.A.st_u4(aov + 16u * out, make_uint4((uint32_t)spid, df, __float_as_uint(th), mask));
#endif
}

}  // namespace

VX_MAIN(rt_kernel_arg_t, arg, RT_BLOCK_THREADS) {
  Counters cnt;
  Scene S = load_scene(arg, vx_launch_words);
  // (the tag is a kernel argument: the light count and the buffer stay in scalar registers)
  const uint32_t nl = vx_launch_tag < RT_MAX_LIGHTS ? vx_launch_tag : RT_MAX_LIGHTS;
#if RT_AOV_BASE == 2
  const uint32_t aov = guide_records(S);
#else
  const uint32_t aov = aov_base(S);
#endif
#if RT_AOV_BASE
  const uint32_t base = base_colours(S);
#else
  const uint32_t base = 0;
#endif
  const int rc = vx_spawn_tasks(
      S.num_tasks, [&](const vx_task_t& task, const Scene* s) { kernel_body(task, *s, nl, aov, base, cnt); }, &S);
  // a frame's primary rays and hits; the shadow rays of every light, the masks' set bits
  flush_rays(cnt);
  return rc;
}
