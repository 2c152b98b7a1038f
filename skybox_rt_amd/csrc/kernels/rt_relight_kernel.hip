// rt_relight_kernel.hip -- a frame relit from its visibility records (vx_rt.h
// rt_render_relight_start): per framebuffer pixel the record's depth_flags and
// light_mask (rt_aov_t, written by the capture launch, rt_aov_kernel.hip
// RT_AOV_BASE) and the pixel's base colour -- shaded without shadows by the
// same launch -- give the pixel under per-light weights (rt_common.h
// rt_relight_mix), stored to the framebuffer in use.  No scene, no tree, no
// texel, no LDS: a streaming pass over 24 B a pixel (16 B record and 4 B colour
// in, 4 B out).
//
// Access shape.  The record is loaded whole, one 16-B load per pixel: the two
// words the pixel needs sit at bytes 4 and 12 of it, so two dword loads would
// touch the same 128-B lines with twice the instructions and a quarter of the
// width; the memory system moves whole lines either way, and 24 B a pixel is
// what the launch is charged with.  A wave takes RT_RL_PIXELS = 4 runs of 64
// consecutive pixels, lane l pixel 64 j + l of run j: every record load is
// 1 KiB contiguous per wave, every colour load and store 256 B contiguous
// (a lane's four pixels 64 apart: a 16-B colour access per lane would need the
// records transposed through LDS).  All eight loads of a lane (80 B) are
// issued before the first use.  Grid: 256-thread workgroups, 8 per CU, the
// module's grid of 2048 on 256 CUs -- a workgroup steps over 1024 pixels, so
// 1024^2 is one step for 1024 workgroups and 4 waves of 5 KiB in flight on
// every SIMD, past what covers the memory latency at full bandwidth; larger
// frames stride.
//
// Wave-uniform inputs: the 16 weight bytes are the four launch words; the
// launch tag carries the light count, which framebuffer is in use and the
// divisor's multiplier (rt_common.h RT_RL_TAG_*); the buffers and the pixel
// count sit in the argument areas (rt_aov_arg_t, rt_relight_arg_t).
#include <hip/hip_runtime.h>

#define RT_RL_THREADS 256
#define RT_RL_PIXELS 4
#define VX_BLOCK_THREADS RT_RL_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "vx_spawn.h"
#include "rt_common.h"

// workgroups per CU (hip_driver.cpp reads it): 2048 on the chip, the streaming kernels' cap
__device__ __attribute__((used)) uint32_t __vx_grid_per_cu = 8;

namespace {

__device__ __forceinline__ uint32_t sgpr(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }

}  // namespace

VX_MAIN(rt_kernel_arg_t, arg, RT_RL_THREADS) {
  const vx_arena A = vx_arena::get();
  // the argument areas through the scalar cache (constant during the launch)
  const uint64_t ap = ((uint64_t)sgpr((uint32_t)((uint64_t)arg >> 32)) << 32) | sgpr((uint32_t)(uint64_t)arg);
  const auto* ka = (const __attribute__((address_space(4))) rt_kernel_arg_t*)ap;
  const auto* aa = (const __attribute__((address_space(4))) rt_aov_arg_t*)(ap + RT_AOV_ARG_OFFSET);
  const auto* ra = (const __attribute__((address_space(4))) rt_relight_arg_t*)(ap + RT_RELIGHT_ARG_OFFSET);
  const uint32_t tag = sgpr(vx_launch_tag);
  const uint32_t n = tag & RT_RL_TAG_N_MASK, m = (tag >> RT_RL_TAG_M_SHIFT) & 0x7fffffu;
  const uint32_t rec = (uint32_t)aa->aov_addr, base = (uint32_t)ra->base_addr, npix = ra->npix;
  const uint32_t fb = (uint32_t)ka->cbuf_addr + ((tag & RT_RL_TAG_CBUF1) ? ra->cbuf1_off : 0u);
  const uint32_t w[4] = {sgpr(vx_launch_words.w[0]), sgpr(vx_launch_words.w[1]), sgpr(vx_launch_words.w[2]),
                         sgpr(vx_launch_words.w[3])};
  uint32_t W = 0;
  for (uint32_t i = 0; i < n; ++i) W += (w[i >> 2] >> (8u * (i & 3u))) & 0xffu;
  const uint32_t s = rt_relight_shift(W ? W : 1u);
  const uint32_t live = n >= RT_MAX_LIGHTS ? 0xffffu : (1u << n) - 1u;  // the lights in use

  __vx_declare_tasks(npix);
  const uint32_t span = 64u * RT_RL_PIXELS;  // pixels a wave takes per step
  const uint32_t nwaves = gridDim.x * (RT_RL_THREADS / 64u);
  const uint32_t wave = blockIdx.x * (RT_RL_THREADS / 64u) + (threadIdx.x >> 6);
  for (uint32_t p0 = sgpr(wave * span); p0 < npix; p0 += nwaves * span) {
    const uint32_t p = p0 + (threadIdx.x & 63u);
    uint4 r[RT_RL_PIXELS];
    uint32_t c[RT_RL_PIXELS];
    // (past the end: offsets the loads may form, results unused, no store)
#pragma unroll
    for (int j = 0; j < RT_RL_PIXELS; ++j) {
      const uint32_t q = p + 64u * j < npix ? p + 64u * j : npix - 1u;
      r[j] = A.ld_u4(rec + 16u * q);
      c[j] = A.ld_u32(base + 4u * q);
    }
#pragma unroll
    for (int j = 0; j < RT_RL_PIXELS; ++j) {
      const uint32_t mask = (r[j].y & RT_AOV_SHADOW_RAY) ? r[j].w & live : 0u;
      uint32_t out = c[j];
      if (__ballot(mask != 0) != 0) {  // (a wave of pixels every light sees stores its base colours)
        const uint32_t O = rt_relight_occluded(mask, w, n);
        out = rt_relight_mix(c[j], O, W, s, m);
      }
      if (p + 64u * j < npix) A.st_u32(fb + 4u * (p + 64u * j), out);
    }
  }
  return 0;
}
