// rt_query_kernel.hip -- caller-supplied rays against the scene's tree (vx_rt.h
// rt_query_trace_start): per ray of the query buffers (rt_common.h
// rt_query_arg_t) one closest-hit or any-hit walk of the binary16 BVH4 and one
// rt_hit_t {pid, t} stored at the ray's own index; a miss is {-1, 0.0f}.  A
// tracing launch that shades nothing, reads no texel, writes neither a
// framebuffer nor a record buffer and counts nothing.
//
// A wave takes 64 consecutive ray slots per task (vx_spawn_tasks: task q is lane
// q & 63 of chunk q >> 6), workgroups of RT_QUERY_WAVES waves, each wave with
// its own LDS column stack; the waves of a workgroup share nothing and meet at
// no barrier.  Lane l of task i handles slot q = 64 i + l; its ray index is
// perm[q] under RT_QUERY_PERM, else q.  Lanes with q >= n run nothing: they load
// and store nothing.  A permutation entry >= n -- not a permutation of [0, n) --
// is dropped the same way, so no index leaves the first n records.  The ray
// arrives as two 16-B loads (o, tmin | d, tmax), the skip word is loaded only
// under RT_QUERY_SKIP, and one predicate (rt_query_malformed) keeps a malformed
// ray from the walk: it stores the miss.  The mode is wave-uniform, from the
// launch words: trace<false> or trace<true> of rt_trace.h as they are, with
// tie_high = false.  One 8-B store per lane.
//
// The launch words: w[0] = n; w[1] = mode | flags << 8 (rt_common.h
// RT_QUERY_LW_*); w[2] = w[3] = 0.
#include <hip/hip_runtime.h>

#ifndef RT_QUERY_WAVES
#define RT_QUERY_WAVES 1
#endif
#define RT_BLOCK_THREADS (64 * RT_QUERY_WAVES)
#define VX_BLOCK_THREADS RT_BLOCK_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "rt_trace.h"

#if !RT_ONLY_BVH4H
#error "rt_query_kernel.hip walks the binary16 BVH4 only (build with -DRT_ONLY_BVH4H=1)"
#endif
#if RT_QUERY_WAVES < 1 || RT_QUERY_WAVES > 4
#error "rt_query_kernel.hip: RT_QUERY_WAVES is 1..4"
#endif

// workgroups per CU (hip_driver.cpp reads it): 128 waves, as rt_ao's, whose waves run the same
// per-lane walk -- the blocks waiting for a slot are the load balancer
__device__ __attribute__((used)) uint32_t __vx_grid_per_cu = 128 / RT_QUERY_WAVES;

namespace {

using namespace rtk;

struct QueryBufs {
  uint32_t rays, hits, skip, perm, n;
  bool any, use_skip, use_perm;
};

__device__ __forceinline__ void query_body(uint32_t q, const Scene& S, const QueryBufs& B, int32_t* stack,
                                           Counters& cnt) {
  uint32_t i = q;
  if (B.use_perm) {
    i = S.A.ld_u32(B.perm + 4u * q);
    if (i >= B.n) return;
  }
  const uint4 a = S.A.ld_u4(B.rays + 32u * i), b = S.A.ld_u4(B.rays + 32u * i + 16u);
  int32_t skip = -1;
  if (B.use_skip) skip = (int32_t)S.A.ld_u32(B.skip + 4u * i);
  const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  int32_t pid = -1;
  float t = 0.0f;
  if (!rt_query_malformed(w) && S.num_geom != 0u) {
    Ray r;
    r.o[0] = __uint_as_float(a.x);
    r.o[1] = __uint_as_float(a.y);
    r.o[2] = __uint_as_float(a.z);
    r.d[0] = __uint_as_float(b.x);
    r.d[1] = __uint_as_float(b.y);
    r.d[2] = __uint_as_float(b.z);
    ray_setup(r);
    const float tmin = __uint_as_float(a.w), tmax = __uint_as_float(b.w);
    if (B.any)
      pid = trace<true>(S, r, tmin, tmax, skip, false, &t, stack, cnt);
    else
      pid = trace<false>(S, r, tmin, tmax, skip, false, &t, stack, cnt);
  }
  S.A.st_u2(B.hits + 8u * i, make_uint2((uint32_t)pid, pid >= 0 ? __float_as_uint(t) : 0u));
}

}  // namespace

VX_MAIN(rt_kernel_arg_t, arg, RT_BLOCK_THREADS) {
  __shared__ int32_t s_stack[RT_QUERY_WAVES][RT_STACK_ROWS][64];  // the per-lane walk's column stacks
  Counters cnt;
  Scene S = load_scene(arg, vx_launch_words);
  const auto* qa = arg_at<rt_query_arg_t>(S, RT_QUERY_ARG_OFFSET);
  QueryBufs B;
  B.rays = (uint32_t)qa->rays_addr;
  B.hits = (uint32_t)qa->hits_addr;
  B.skip = (uint32_t)qa->skip_addr;
  B.perm = (uint32_t)qa->perm_addr;
  const uint32_t cap = qa->capacity;
  const uint32_t w0 = (uint32_t)__builtin_amdgcn_readfirstlane(vx_launch_words.w[0]);
  const uint32_t w1 = (uint32_t)__builtin_amdgcn_readfirstlane(vx_launch_words.w[1]);
  B.n = w0 < cap ? w0 : cap;  // (the host checked it: no index leaves the buffers whatever the words hold)
  B.any = (w1 & RT_QUERY_LW_MODE_MASK) == 1u;
  B.use_skip = ((w1 >> RT_QUERY_LW_FLAG_SHIFT) & 1u) != 0u;
  B.use_perm = ((w1 >> RT_QUERY_LW_FLAG_SHIFT) & 2u) != 0u;
  int32_t* stack = &s_stack[threadIdx.x >> 6][0][threadIdx.x & 63u];
  return vx_spawn_tasks(
      B.n, [&](const vx_task_t& task, const Scene* s) { query_body(task.task_id, *s, B, stack, cnt); }, &S);
}
