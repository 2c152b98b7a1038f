// rt_ao_kernel.hip -- ambient occlusion from a frame's visibility records
// (vx_rt.h rt_render_ao_start): per ray pixel of the records the last record
// launch wrote (rt_aov_t: RT_AOV_GEOM and a plane t that is finite and > 0), S
// any-hit rays from the path tracer's first vertex -- P = d * (t * (1 - 2^-12)),
// the geometric normal facing the eye, bounce_dir under pt_key(seed + c, p, 0)
// for sample cursor c -- each occluded iff some geometry triangle other than
// the pixel's own lies within `radius` along it.  The number of occluded
// samples is added to one uint32 per framebuffer pixel (rt_common.h
// rt_ao_arg_t).  A tracing launch that shades nothing, reads no texel, writes
// neither the framebuffer nor the visibility records and needs no global
// atomic: the workgroup of an 8x8 block owns the block's 64 counts.
//
// One workgroup of RT_AO_WAVES waves per 8x8 block of the linear framebuffer,
// lane l of every wave the pixel (l & 7, l >> 3) of the block (RT_AO_WAVES 1:
// one wave per block; more: the block's rounds dealt over the waves, which
// share the block's LDS tables -- a block's rays are a serial chain of rounds
// otherwise, and at 1024^2 tekkaman only an eighth of the blocks hold a ray
// pixel, too few one-wave chains to fill the chip).  The lane loads its pixel's
// 16-B record; a block without a ray pixel stores its zeros when the launch
// resets (RT_AO_LW_RESET) and leaves before it touches the scene.  Otherwise the
// ray pixels write their first vertex (P, n, pid, pixel index) to LDS at their
// rank among the block's ray pixels (wave 0's lanes; every wave has read the
// same records), and the block's live x S (pixel, sample) pairs are dealt to the
// lanes in rounds of 64, pixel-major -- neighbouring lanes share an origin, and
// a block with three ray pixels still traces on full waves -- round i to wave
// i mod RT_AO_WAVES.  A lane traces one ray per round and adds its verdict to
// its pixel's slot of a 64-entry LDS table; at the end the pixel's lane of wave
// 0 stores the slot, or the old count plus it.
//
// The walk: the per-lane any-hit walk on the LDS column stack (trace<true>), or
// with -DRT_AO_PACKET=1 the wave's packet walk (occluded_packet) -- the A/B of
// DESIGN.md 2.6.  Either answers "any occluder within radius", so the counts
// are the same.
//
// The launch words: w[0] the radius (float bits, +inf admitted), w[1] seed +
// cursor of the launch's first sample (mod 2^32), w[2] RT_AO_LW_*: the samples
// and the reset bit; w[3] 0 (a frame's flags: none).
#include <hip/hip_runtime.h>

#ifndef RT_AO_WAVES
#define RT_AO_WAVES 1
#endif
#define RT_BLOCK_THREADS (64 * RT_AO_WAVES)
#ifndef RT_AO_PACKET
#define RT_AO_PACKET 0
#endif
#define VX_BLOCK_THREADS RT_BLOCK_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "rt_trace.h"
#include "rt_path.h"  // pt_key, bounce_dir, tri_normal

#if !RT_ONLY_BVH4H
#error "rt_ao_kernel.hip walks the binary16 BVH4 only (build with -DRT_ONLY_BVH4H=1)"
#endif
#if RT_AO_WAVES < 1 || RT_AO_WAVES > 4
#error "rt_ao_kernel.hip: RT_AO_WAVES is 1..4"
#endif

// workgroups per CU (hip_driver.cpp reads it): the path tracer's 128 waves, whose waves run the
// same per-lane walk on the same stack
__device__ __attribute__((used)) uint32_t __vx_grid_per_cu = 128 / RT_AO_WAVES;

namespace {

using namespace rtk;

struct AoLds {
#if !RT_AO_PACKET
  int32_t stack[RT_AO_WAVES][RT_STACK_ROWS][64];  // the per-lane walk's column stacks
#endif
  float v[6][64];     // a ray pixel's first vertex at its rank: P, n
  int32_t pid[64];    // its primitive
  uint32_t pix[64];   // its framebuffer index
  uint32_t occ[64];   // its occluded samples of this launch
};

__device__ __forceinline__ void kernel_body(const vx_task_t& task, const Scene& S, AoLds& L, uint32_t rec_buf,
                                            uint32_t ao_buf, uint32_t nbx, float radius, uint32_t seed0, uint32_t ns,
                                            bool reset, Counters& cnt) {
  const uint32_t ln = task.blockIdx.x & 63u, wv = threadIdx.x >> 6;
  const bool own = RT_AO_WAVES == 1 || wv == 0;  // the wave that writes the tables and stores the counts
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
    if (reset && in && own) S.A.st_u32(ao_buf + 4u * p, 0u);
    return;
  }
  const uint32_t live = (uint32_t)__popcll(m);
  const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  uint32_t old = 0;
  if (!reset && in && own) old = S.A.ld_u32(ao_buf + 4u * p);
  if (own) L.occ[ln] = 0u;
  if (ray && own) {
    // the path tracer's first vertex (pt_kernel.hip path_step, v = 0)
    Ray r;
    primary_dir(S, x, y, r);
    const uint32_t o = S.ptris + 48u * rec.x;
    const float4 t1 = S.A.ld_f4(o + 16), t2 = S.A.ld_f4(o + 32);
    const float e1[3] = {t1.x, t1.y, t1.z}, e2[3] = {t2.x, t2.y, t2.z};
    float n[3];
    tri_normal(e1, e2, r.d, n);
    const float tt = th * 0.999755859375f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      L.v[k][rank] = r.d[k] * tt;
      L.v[3 + k][rank] = n[k];
    }
    L.pid[rank] = (int32_t)rec.x;
    L.pix[rank] = p;
  }
  __syncthreads();  // (the tables are written)
  const uint32_t total = live * ns;
  for (uint32_t q0 = 64u * (uint32_t)__builtin_amdgcn_readfirstlane(wv); q0 < total; q0 += 64u * RT_AO_WAVES) {
    const uint32_t q = q0 + ln;
    const bool act = q < total;
    const uint32_t k = act ? q / ns : 0u, j = q - k * ns;  // pixel-major
    Ray a;
    float n[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      a.o[i] = L.v[i][k];
      n[i] = L.v[3 + i][k];
    }
    const int32_t pid = L.pid[k];
    bounce_dir(n, pt_key(seed0 + j, L.pix[k], 0u), a.d);
    ray_setup(a);
    cnt.shadow += act;
#if RT_AO_PACKET
    const bool occ = occluded_packet(S, a, act, pid, radius, cnt);
#else
    float ts;
    const bool occ = act && trace<true>(S, a, 0.0f, radius, pid, false, &ts, &L.stack[wv][0][ln], cnt) >= 0;
#endif
    cnt.occluded += occ;
    if (occ) atomicAdd(&L.occ[k], 1u);
  }
  __syncthreads();  // (the verdicts are counted)
  if (in && own) S.A.st_u32(ao_buf + 4u * p, old + (ray ? L.occ[rank] : 0u));
  __syncthreads();  // (read before the workgroup's next block zeroes the table)
}

}  // namespace

VX_MAIN(rt_kernel_arg_t, arg, RT_BLOCK_THREADS) {
  __shared__ AoLds s_ao;
  Counters cnt;
  Scene S = load_scene(arg, vx_launch_words);
  const uint32_t rec_buf = (uint32_t)arg_at<rt_aov_arg_t>(S, RT_AOV_ARG_OFFSET)->aov_addr;
  const uint32_t ao_buf = (uint32_t)arg_at<rt_ao_arg_t>(S, RT_AO_ARG_OFFSET)->ao_addr;
  const float radius = __uint_as_float(vx_launch_words.w[0]);
  const uint32_t seed0 = vx_launch_words.w[1], w2 = vx_launch_words.w[2];
  const uint32_t ns = min((w2 & RT_AO_LW_S_MASK) + 1u, RT_AO_MAX_S);
  const bool reset = (w2 & RT_AO_LW_RESET) != 0;
  const uint32_t nbx = (S.width + 7u) >> 3, nby = (S.height + 7u) >> 3;
  // (every wave of the workgroup sees the block's 64 tasks; the task count is a multiple of 64)
  const int rc = vx_spawn_chunks_block(
      nbx * nby * 64u,
      [&](const vx_task_t& task, bool, const Scene* s) {
        kernel_body(task, *s, s_ao, rec_buf, ao_buf, nbx, radius, seed0, ns, reset, cnt);
      },
      &S);
  // the rays traced and the sum of their verdicts, the only two
  flush(RT_STAT_SHADOW, cnt.shadow);
  flush(RT_STAT_OCCLUDED, cnt.occluded);
  return rc;
}
