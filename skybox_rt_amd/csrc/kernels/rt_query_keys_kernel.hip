// rt_query_keys_kernel.hip -- the coherence keys of caller-supplied rays (vx_rt.h
// rt_query_keys_start): per ray of the query buffers (rt_common.h rt_query_arg_t)
// one uint32 -- the direction's sign bits over the Morton code of the origin's
// cell in the scene box over the direction's cell (rt_common.h rt_query_key_of,
// the function the host's rt_query_key calls) -- so that rays sorted by key
// share an octant, start close together and point the same way.  Malformed rays
// get 0xFFFFFFFF and sort to the end.  No scene, no tree, no LDS: a streaming
// pass of 32 B in and 4 B out per ray, lane l of a task ray 64 i + l (two 16-B
// loads, one 4-B store: 256 B contiguous per wave).  Sorting is the caller's.
//
// The launch words: w[0] = n; the rest 0.  The grid's box (low corner and 128 /
// extent per axis) is in the argument area, written by rt_query_reserve.
#include <hip/hip_runtime.h>

#define RT_QK_THREADS 256
#define VX_BLOCK_THREADS RT_QK_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "vx_spawn.h"
#include "rt_common.h"

// workgroups per CU (hip_driver.cpp reads it): 2048 on the chip, the streaming kernels' cap
__device__ __attribute__((used)) uint32_t __vx_grid_per_cu = 8;

namespace {

__device__ __forceinline__ uint32_t sgpr(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }

}  // namespace

VX_MAIN(rt_kernel_arg_t, arg, RT_QK_THREADS) {
  const vx_arena A = vx_arena::get();
  // the argument area through the scalar cache (constant during the launch)
  const uint64_t ap = ((uint64_t)sgpr((uint32_t)((uint64_t)arg >> 32)) << 32) | sgpr((uint32_t)(uint64_t)arg);
  const auto* qa = (const __attribute__((address_space(4))) rt_query_arg_t*)(ap + RT_QUERY_ARG_OFFSET);
  const uint32_t rays = (uint32_t)qa->rays_addr, keys = (uint32_t)qa->keys_addr, cap = qa->capacity;
  const float lo[3] = {qa->key_lo[0], qa->key_lo[1], qa->key_lo[2]};
  const float inv[3] = {qa->key_inv[0], qa->key_inv[1], qa->key_inv[2]};
  const uint32_t w0 = sgpr(vx_launch_words.w[0]);
  uint32_t n = w0 < cap ? w0 : cap;  // (the host checked it: no index leaves the buffers)
  return vx_spawn_tasks(
      n,
      [&](const vx_task_t& task, rt_kernel_arg_t*) {
        const uint32_t i = task.task_id;
        const uint4 a = A.ld_u4(rays + 32u * i), b = A.ld_u4(rays + 32u * i + 16u);
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        A.st_u32(keys + 4u * i, rt_query_key_of(w, lo, inv));
      },
      arg);
}
