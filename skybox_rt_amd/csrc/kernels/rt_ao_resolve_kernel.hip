// rt_ao_resolve_kernel.hip -- the ambient term resolved into the framebuffer in
// use (vx_rt.h rt_render_ao_resolve_start): per framebuffer pixel the count of
// occluded samples (rt_common.h rt_ao_arg_t, written by rt_ao_kernel.hip) over
// the launch's N samples scales a colour (rt_ao_mix) -- white for RT_AO_GREY,
// the relit pixel for RT_AO_MODULATE: the relight capture's base colour under
// the per-light weights of the launch words (rt_relight_kernel.hip's pixel), or
// the base colour itself without weights.  No scene, no tree, no texel, no LDS:
// a streaming pass in rt_relight_kernel.hip's access shape -- 8 B a pixel for
// grey (4 B count in, 4 B out), 28 B for modulate (16 B record, 4 B colour and
// 4 B count in, 4 B out).
//
// A wave takes RT_AR_PIXELS = 4 runs of 64 consecutive pixels, lane l pixel
// 64 j + l of run j: every count, colour and store access is 256 B contiguous
// per wave, every record load 1 KiB; all loads of a lane are issued before the
// first use.  Grid as rt_relight_kernel.hip's.
//
// Wave-uniform inputs: the tag carries N, the mode, which framebuffer is in use
// and the light count (rt_common.h RT_AO_TAG_*); the words are the weights.  The
// two divisions, by 2 N and by 2 W, are exact from one binary32 reciprocal each
// (rt_common.h rt_ao_quot).
#include <hip/hip_runtime.h>

#define RT_AR_THREADS 256
#define RT_AR_PIXELS 4
#define VX_BLOCK_THREADS RT_AR_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "vx_spawn.h"
#include "rt_common.h"

// workgroups per CU (hip_driver.cpp reads it): 2048 on the chip, the streaming kernels' cap
__device__ __attribute__((used)) uint32_t __vx_grid_per_cu = 8;

namespace {

__device__ __forceinline__ uint32_t sgpr(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }

}  // namespace

VX_MAIN(rt_kernel_arg_t, arg, RT_AR_THREADS) {
  const vx_arena A = vx_arena::get();
  // the argument areas through the scalar cache (constant during the launch)
  const uint64_t ap = ((uint64_t)sgpr((uint32_t)((uint64_t)arg >> 32)) << 32) | sgpr((uint32_t)(uint64_t)arg);
  const auto* ka = (const __attribute__((address_space(4))) rt_kernel_arg_t*)ap;
  const auto* va = (const __attribute__((address_space(4))) rt_aov_arg_t*)(ap + RT_AOV_ARG_OFFSET);
  const auto* ra = (const __attribute__((address_space(4))) rt_relight_arg_t*)(ap + RT_RELIGHT_ARG_OFFSET);
  const auto* aa = (const __attribute__((address_space(4))) rt_ao_arg_t*)(ap + RT_AO_ARG_OFFSET);
  const uint32_t tag = sgpr(vx_launch_tag);
  const uint32_t N = (tag >> RT_AO_TAG_SAMPLES_SHIFT) & 0xffffu, n = tag & RT_AO_TAG_N_MASK;
  const bool modulate = (tag & RT_AO_TAG_MODULATE) != 0, weighted = (tag & RT_AO_TAG_WEIGHTS) != 0;
  const uint32_t ao = (uint32_t)aa->ao_addr, npix = aa->npix;
  const uint32_t fb = (uint32_t)ka->cbuf_addr + ((tag & RT_AO_TAG_CBUF1) ? aa->cbuf1_off : 0u);
  // (read by a modulate launch only: the relight capture wrote the areas)
  const uint32_t rec = modulate ? (uint32_t)va->aov_addr : 0u, base = modulate ? (uint32_t)ra->base_addr : 0u;
  const uint32_t w[4] = {sgpr(vx_launch_words.w[0]), sgpr(vx_launch_words.w[1]), sgpr(vx_launch_words.w[2]),
                         sgpr(vx_launch_words.w[3])};
  uint32_t W = 0;
  for (uint32_t i = 0; i < n; ++i) W += (w[i >> 2] >> (8u * (i & 3u))) & 0xffu;
  W = W ? W : 1u;
  const float rdN = 1.0f / (float)(2u * (N ? N : 1u)), rdW = 1.0f / (float)(2u * W);
  const uint32_t live = n >= RT_MAX_LIGHTS ? 0xffffu : (1u << n) - 1u;  // the lights in use

  __vx_declare_tasks(npix);
  const uint32_t span = 64u * RT_AR_PIXELS;  // pixels a wave takes per step
  const uint32_t nwaves = gridDim.x * (RT_AR_THREADS / 64u);
  const uint32_t wave = blockIdx.x * (RT_AR_THREADS / 64u) + (threadIdx.x >> 6);
  for (uint32_t p0 = sgpr(wave * span); p0 < npix; p0 += nwaves * span) {
    const uint32_t p = p0 + (threadIdx.x & 63u);
    uint32_t o[RT_AR_PIXELS], c[RT_AR_PIXELS];
    uint4 r[RT_AR_PIXELS];
    // (past the end: offsets the loads may form, results unused, no store)
#pragma unroll
    for (int j = 0; j < RT_AR_PIXELS; ++j) {
      const uint32_t q = p + 64u * j < npix ? p + 64u * j : npix - 1u;
      o[j] = A.ld_u32(ao + 4u * q);
      c[j] = 0xffffffffu;
      r[j] = make_uint4(0u, 0u, 0u, 0u);
      if (modulate) {
        c[j] = A.ld_u32(base + 4u * q);
        if (weighted) r[j] = A.ld_u4(rec + 16u * q);
      }
    }
#pragma unroll
    for (int j = 0; j < RT_AR_PIXELS; ++j) {
      uint32_t col = c[j];
      const uint32_t mask = (r[j].y & RT_AOV_SHADOW_RAY) ? r[j].w & live : 0u;
      if (__ballot(mask != 0) != 0) col = rt_ao_relight_mix(col, rt_relight_occluded(mask, w, n), W, rdW);
      // (a wave of pixels without an occluded sample stores its colours: rt_ao_mix(c, 0, N) = c)
      if (__ballot(o[j] != 0) != 0) {
        // (a count past N cannot be: clamped, so the subtraction stays in range whatever the buffer holds)
        const uint32_t oc = o[j] < N ? o[j] : N;
        if (modulate) {
          col = rt_ao_mix(col, oc, N, rdN);
        } else {  // white: one quotient serves the three channels
          const uint32_t g = rt_ao_quot(2u * 255u * (N - oc) + N, 2u * N, rdN);
          col = 0xff000000u | (g << 16) | (g << 8) | g;
        }
      }
      if (p + 64u * j < npix) A.st_u32(fb + 4u * (p + 64u * j), col);
    }
  }
  return 0;
}
