// rt_soft_kernel.hip -- soft shadows from area lights, sampled from a frame's
// visibility records (vx_rt.h rt_render_soft_start): per ray pixel of the
// records the last record launch wrote (rt_aov_t: RT_AOV_GEOM and a plane t that
// is finite and > 0) and per light in use, S any-hit segments from the frame's
// shadow origin -- P = d * (t * (1 - 2^-12)) -- to a point of the light's sphere:
// its centre plus its radius times bounce_dir about the unit vector from the
// centre to P, under pt_key(seed + c, p, RT_SOFT_VERTEX + i) for sample cursor c
// and light i -- a cosine-weighted point of the hemisphere that faces P, uniform
// over the disc P sees.  A sample is occluded iff some geometry triangle other
// than the pixel's own meets the segment (tmax = 1).  The number of occluded
// samples is added to one uint16 per light and framebuffer pixel (rt_common.h
// rt_soft_arg_t: a plane per light).  A tracing launch that shades nothing,
// reads no texel, writes neither the framebuffer nor the visibility records and
// needs no global atomic: the workgroup of an 8x8 block owns the block's 64 x n
// counts.
//
// rt_ao_kernel.hip's structure: one workgroup of RT_SOFT_WAVES waves per 8x8
// block of the linear framebuffer, lane l of every wave the pixel (l & 7, l >>
// 3) of the block.  The lane loads its pixel's 16-B record; a block without a
// ray pixel stores its zeros when the launch resets (RT_SOFT_LW_RESET) and
// leaves before it touches the scene.  Otherwise the ray pixels write their
// origin, primitive and pixel index to LDS at their rank among the block's ray
// pixels (wave 0's lanes; every wave has read the same records), and the
// block's live x n x S (pixel, light, sample) triples are dealt to the lanes in
// rounds of 64, round i to wave i mod RT_SOFT_WAVES -- pixel-major (pixel,
// light, sample: neighbouring lanes share an origin) or with
// -DRT_SOFT_LIGHT_MAJOR=1 light-major (light, pixel, sample: neighbouring lanes
// share a target).  A lane normalises, samples and traces one triple per round.
//
// The launch's table: a launch adds at most 64 to a (pixel, light) count, so
// four lights' counts of a pixel pack into one LDS word -- a verdict adds 1 <<
// 8 * (i & 3) to word [i >> 2][rank], 1 KiB at 16 lights beside the column
// stack's 6.75 KiB a wave.  At the end the pixel's lane of wave 0 stores, per
// light, its byte or the old count plus it: 2 B a lane, 128 B a wave and plane.
//
// The lights (centre, radius) come from the launch's own argument area to an
// LDS table once per workgroup: a triple's light differs from lane to lane.
//
// The walk: the per-lane any-hit walk on the LDS column stack (trace<true>), or
// with -DRT_SOFT_PACKET=1 the wave's packet walk (occluded_packet) -- the A/B of
// DESIGN.md 2.6.  Either answers "any occluder on the segment", so the counts
// are the same.
//
// The launch words: w[0] seed + cursor of the launch's first sample (mod 2^32),
// w[1] RT_SOFT_LW_*: the samples, the reset bit and the lights in use; w[2] 0;
// w[3] 0 (a frame's flags: none).
#include <hip/hip_runtime.h>

#ifndef RT_SOFT_WAVES
#define RT_SOFT_WAVES 1
#endif
#define RT_BLOCK_THREADS (64 * RT_SOFT_WAVES)
#ifndef RT_SOFT_PACKET
#define RT_SOFT_PACKET 0
#endif
#ifndef RT_SOFT_LIGHT_MAJOR
#define RT_SOFT_LIGHT_MAJOR 0
#endif
#define VX_BLOCK_THREADS RT_BLOCK_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "rt_trace.h"
#include "rt_path.h"  // pt_key, bounce_dir

#if !RT_ONLY_BVH4H
#error "rt_soft_kernel.hip walks the binary16 BVH4 only (build with -DRT_ONLY_BVH4H=1)"
#endif
#if RT_SOFT_WAVES < 1 || RT_SOFT_WAVES > 4
#error "rt_soft_kernel.hip: RT_SOFT_WAVES is 1..4"
#endif

// workgroups per CU (hip_driver.cpp reads it): rt_ao_kernel.hip's 128 waves -- the per-lane images run its
// walk on its stack; the packet images, without a stack in LDS, are not held below that by LDS either
__device__ __attribute__((used)) uint32_t __vx_grid_per_cu = 128 / RT_SOFT_WAVES;

namespace {

using namespace rtk;

struct SoftLds {
#if !RT_SOFT_PACKET
  int32_t stack[RT_SOFT_WAVES][RT_STACK_ROWS][64];  // the per-lane walk's column stacks
#endif
  float v[3][64];                        // a ray pixel's origin P at its rank
  int32_t pid[64];                       // its primitive
  uint32_t pix[64];                      // its framebuffer index
  uint32_t occ[RT_MAX_LIGHTS / 4][64];   // its occluded samples of this launch, four lights a word
  float lt[4][RT_MAX_LIGHTS];            // light i: radius, centre
};

__device__ __forceinline__ void kernel_body(const vx_task_t& task, const Scene& S, SoftLds& L, uint32_t rec_buf,
                                            uint32_t planes, uint32_t npix, uint32_t nbx, uint32_t seed0, uint32_t ns,
                                            uint32_t nl, bool reset, Counters& cnt) {
  const uint32_t ln = task.blockIdx.x & 63u, wv = threadIdx.x >> 6;
  const bool own = RT_SOFT_WAVES == 1 || wv == 0;  // the wave that writes the tables and stores the counts
  // the block in scalar registers (every lane runs the same block)
  const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane(task.blockIdx.x) >> 6;
  const uint32_t by = b / nbx, bx = b - by * nbx;
  const uint32_t x = 8u * bx + (ln & 7u), y = 8u * by + (ln >> 3);
  const bool in = x < S.width && y < S.height;  // edge blocks overhang the image
  const uint32_t p = y * S.width + x;
  uint4 rec = make_uint4(0u, 0u, 0u, 0u);
  if (in) rec = S.A.ld_u4(rec_buf + 16u * p);
  const float th = __uint_as_float(rec.z);
  const bool ray = in && (rec.y & RT_AOV_GEOM) != 0 && secondary_ok(th);
  const uint64_t m = __ballot(ray);
  if (m == 0) {
    // (every wave of the workgroup read the same records, so m is the same in all of them: they all
    // leave here, ahead of the barriers below, or none does)
    if (reset && in && own)
      for (uint32_t i = 0; i < nl; ++i) S.A.st_u16(planes + 2u * (i * npix + p), 0u);
    return;
  }
  const uint32_t live = (uint32_t)__popcll(m);
  const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (own) {
#pragma unroll
    for (uint32_t g = 0; g < RT_MAX_LIGHTS / 4; ++g) L.occ[g][ln] = 0u;
  }
  if (ray && own) {
    // the frame's shadow origin (rt_trace.h shadow_ray)
    Ray r;
    primary_dir(S, x, y, r);
    const float tt = th * 0.999755859375f;
#pragma unroll
    for (int k = 0; k < 3; ++k) L.v[k][rank] = r.d[k] * tt;
    L.pid[rank] = (int32_t)rec.x;
    L.pix[rank] = p;
  }
  __syncthreads();  // (the tables are written)
  const uint32_t total = live * nl * ns;
  for (uint32_t q0 = 64u * (uint32_t)__builtin_amdgcn_readfirstlane(wv); q0 < total; q0 += 64u * RT_SOFT_WAVES) {
    const uint32_t q = q0 + ln;
    const bool in_q = q < total;
    const uint32_t qq = in_q ? q : 0u;
    // the triple: pixel rank k, light i, sample j
#if RT_SOFT_LIGHT_MAJOR
    const uint32_t i = qq / (live * ns), rem = qq - i * (live * ns), k = rem / ns, j = rem - k * ns;
#else
    const uint32_t k = qq / (nl * ns), rem = qq - k * (nl * ns), i = rem / ns, j = rem - i * ns;
#endif
    Ray a;
    float c[3], mv[3], u[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      a.o[d] = L.v[d][k];
      c[d] = L.lt[1 + d][i];
      mv[d] = a.o[d] - c[d];
    }
    const float rad = L.lt[0][i];
    const float len = sqrtf(dot3(mv, mv));
    // (a pixel at the light's centre, or out of binary32's range of it: no direction, no segment)
    const bool act = in_q && len > 0.0f && len < INFINITY;
    const float dl = act ? len : 1.0f;
#pragma unroll
    for (int d = 0; d < 3; ++d) mv[d] = mv[d] / dl;
    const int32_t pid = L.pid[k];
    bounce_dir(mv, pt_key(seed0 + j, L.pix[k], RT_SOFT_VERTEX + i), u);
#pragma unroll
    for (int d = 0; d < 3; ++d) a.d[d] = fmaf(rad, u[d], c[d]) - a.o[d];
    ray_setup(a);
    cnt.shadow += act;
#if RT_SOFT_PACKET
    const bool occ = occluded_packet(S, a, act, pid, 1.0f, cnt);
#else
    float ts;
    const bool occ = act && trace<true>(S, a, 0.0f, 1.0f, pid, false, &ts, &L.stack[wv][0][ln], cnt) >= 0;
#endif
    cnt.occluded += occ;
    if (occ) atomicAdd(&L.occ[i >> 2][k], 1u << (8u * (i & 3u)));
  }
  __syncthreads();  // (the verdicts are counted)
  if (in && own) {
    // four lights a step: one table word, the four old counts in flight together
    for (uint32_t g = 0; 4u * g < nl; ++g) {
      const uint32_t word = ray ? L.occ[g][rank] : 0u;
      uint32_t old[4] = {0u, 0u, 0u, 0u};
      if (!reset) {
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e)
          if (4u * g + e < nl) old[e] = S.A.ld_u16(planes + 2u * ((4u * g + e) * npix + p));
      }
#pragma unroll
      for (uint32_t e = 0; e < 4; ++e)
        if (4u * g + e < nl) S.A.st_u16(planes + 2u * ((4u * g + e) * npix + p), old[e] + ((word >> (8u * e)) & 0xffu));
    }
  }
  __syncthreads();  // (read before the workgroup's next block zeroes the table)
}

}  // namespace

VX_MAIN(rt_kernel_arg_t, arg, RT_BLOCK_THREADS) {
  __shared__ SoftLds s_soft;
  Counters cnt;
  Scene S = load_scene(arg, vx_launch_words);
  const uint32_t rec_buf = (uint32_t)arg_at<rt_aov_arg_t>(S, RT_AOV_ARG_OFFSET)->aov_addr;
  const auto sa = arg_at<rt_soft_arg_t>(S, RT_SOFT_ARG_OFFSET);
  const uint32_t planes = (uint32_t)sa->planes_addr, npix = sa->npix;
  const uint32_t seed0 = vx_launch_words.w[0], w1 = vx_launch_words.w[1];
  const uint32_t ns = min((w1 & RT_SOFT_LW_S_MASK) + 1u, RT_SOFT_MAX_S);
  const uint32_t nl = min(max((w1 >> RT_SOFT_LW_N_SHIFT) & 0x1fu, 1u), RT_MAX_LIGHTS);
  const bool reset = (w1 & RT_SOFT_LW_RESET) != 0;
  // the lights, once per workgroup (a lane's own index: vector loads of the argument area)
  if (threadIdx.x < RT_MAX_LIGHTS) {
    const rt_soft_arg_t* g = (const rt_soft_arg_t*)(S.argp + RT_SOFT_ARG_OFFSET);
    const uint32_t i = threadIdx.x;
    s_soft.lt[0][i] = g->radii[i];
#pragma unroll
    for (int d = 0; d < 3; ++d) s_soft.lt[1 + d][i] = g->light[i][d];
  }
  __syncthreads();
  const uint32_t nbx = (S.width + 7u) >> 3, nby = (S.height + 7u) >> 3;
  // (every wave of the workgroup sees the block's 64 tasks; the task count is a multiple of 64)
  const int rc = vx_spawn_chunks_block(
      nbx * nby * 64u,
      [&](const vx_task_t& task, bool, const Scene* s) {
        kernel_body(task, *s, s_soft, rec_buf, planes, npix, nbx, seed0, ns, nl, reset, cnt);
      },
      &S);
  // the rays traced and the sum of their verdicts, the only two
  flush(RT_STAT_SHADOW, cnt.shadow);
  flush(RT_STAT_OCCLUDED, cnt.occluded);
  return rc;
}
