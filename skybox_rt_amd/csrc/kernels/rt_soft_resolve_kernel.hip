// rt_soft_resolve_kernel.hip -- the soft-shadow term resolved into the
// framebuffer in use (vx_rt.h rt_render_soft_resolve_start): per framebuffer
// pixel the n lights' counts of occluded samples (rt_common.h rt_soft_arg_t,
// written by rt_soft_kernel.hip) over the launch's N samples, under the launch
// words' per-light weights, darken a colour (rt_soft_mix) -- the relight
// capture's base colour for RT_SOFT_LIT, white for RT_SOFT_GREY.  No scene, no
// tree, no texel, no LDS: a streaming pass in rt_relight_kernel.hip's access
// shape -- 2 n + 8 B a pixel for lit (n count halves and 4 B colour in, 4 B
// out), 2 n + 4 B for grey.  The record is not read: a pixel that is not a ray
// pixel has counts 0 (the tracing launch stores them), and rt_soft_mix with O =
// 0 is the base colour.
//
// A wave takes RT_SR_PIXELS = 4 runs of 64 consecutive pixels, lane l pixel
// 64 j + l of run j: every colour and store access is 256 B contiguous per
// wave, every count access 128 B per plane.  Grid as rt_relight_kernel.hip's.
//
// Wave-uniform inputs: the tag carries N, the mode, which framebuffer is in use
// and the light count (rt_common.h RT_SOFT_TAG_*); the words are the weights.
// The division by 2 D is exact from one binary32 reciprocal (rt_common.h
// rt_ao_quot, rt_soft_mix).
#include <hip/hip_runtime.h>

#define RT_SR_THREADS 256
#define RT_SR_PIXELS 4
#define VX_BLOCK_THREADS RT_SR_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "vx_spawn.h"
#include "rt_common.h"

// workgroups per CU (hip_driver.cpp reads it): 2048 on the chip, the streaming kernels' cap
__device__ __attribute__((used)) uint32_t __vx_grid_per_cu = 8;

namespace {

__device__ __forceinline__ uint32_t sgpr(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }

}  // namespace

VX_MAIN(rt_kernel_arg_t, arg, RT_SR_THREADS) {
  const vx_arena A = vx_arena::get();
  // the argument areas through the scalar cache (constant during the launch)
  const uint64_t ap = ((uint64_t)sgpr((uint32_t)((uint64_t)arg >> 32)) << 32) | sgpr((uint32_t)(uint64_t)arg);
  const auto* ka = (const __attribute__((address_space(4))) rt_kernel_arg_t*)ap;
  const auto* ra = (const __attribute__((address_space(4))) rt_relight_arg_t*)(ap + RT_RELIGHT_ARG_OFFSET);
  const auto* sa = (const __attribute__((address_space(4))) rt_soft_arg_t*)(ap + RT_SOFT_ARG_OFFSET);
  const uint32_t tag = sgpr(vx_launch_tag);
  const uint32_t N = (tag >> RT_SOFT_TAG_SAMPLES_SHIFT) & 0x7ffu;
  const uint32_t n = (tag & RT_SOFT_TAG_N_MASK) < RT_MAX_LIGHTS ? tag & RT_SOFT_TAG_N_MASK : RT_MAX_LIGHTS;
  const bool lit = (tag & RT_SOFT_TAG_LIT) != 0;
  const uint32_t planes = (uint32_t)sa->planes_addr, npix = sa->npix;
  const uint32_t fb = (uint32_t)ka->cbuf_addr + ((tag & RT_SOFT_TAG_CBUF1) ? sa->cbuf1_off : 0u);
  // (read by a lit launch only: the relight capture wrote the area)
  const uint32_t base = lit ? (uint32_t)ra->base_addr : 0u;
  const uint32_t w[4] = {sgpr(vx_launch_words.w[0]), sgpr(vx_launch_words.w[1]), sgpr(vx_launch_words.w[2]),
                         sgpr(vx_launch_words.w[3])};
  uint32_t W = 0;
  for (uint32_t i = 0; i < n; ++i) W += (w[i >> 2] >> (8u * (i & 3u))) & 0xffu;
  const uint32_t D = (N ? N : 1u) * (W ? W : 1u);
  const float rd = 1.0f / (float)(2u * D);

  if (npix == 0) return 0;  // (no pixel: nothing to clamp an index to)
  __vx_declare_tasks(npix);
  const uint32_t span = 64u * RT_SR_PIXELS;  // pixels a wave takes per step
  const uint32_t nwaves = gridDim.x * (RT_SR_THREADS / 64u);
  const uint32_t wave = blockIdx.x * (RT_SR_THREADS / 64u) + (threadIdx.x >> 6);
  for (uint32_t p0 = sgpr(wave * span); p0 < npix; p0 += nwaves * span) {
    const uint32_t p = p0 + (threadIdx.x & 63u);
    uint32_t q[RT_SR_PIXELS], c[RT_SR_PIXELS], O[RT_SR_PIXELS];
    // (past the end: offsets the loads may form, results unused, no store)
#pragma unroll
    for (int j = 0; j < RT_SR_PIXELS; ++j) {
      q[j] = p + 64u * j < npix ? p + 64u * j : npix - 1u;
      c[j] = lit ? A.ld_u32(base + 4u * q[j]) : 0xffffffffu;
      O[j] = 0u;
    }
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t wi = (w[i >> 2] >> (8u * (i & 3u))) & 0xffu;
      uint32_t o[RT_SR_PIXELS];
#pragma unroll
      for (int j = 0; j < RT_SR_PIXELS; ++j) o[j] = A.ld_u16(planes + 2u * (i * npix + q[j]));
      // (a count past N cannot be: clamped, so O <= D whatever the planes hold)
#pragma unroll
      for (int j = 0; j < RT_SR_PIXELS; ++j) O[j] += wi * (o[j] < N ? o[j] : N);
    }
#pragma unroll
    for (int j = 0; j < RT_SR_PIXELS; ++j) {
      uint32_t col = c[j];
      // (a wave of pixels without an occluded sample stores its colours: rt_soft_mix(c, 0, D) = c)
      if (__ballot(O[j] != 0) != 0) col = rt_soft_mix(col, O[j], D, rd);
      if (p + 64u * j < npix) A.st_u32(fb + 4u * (p + 64u * j), col);
    }
  }
  return 0;
}
