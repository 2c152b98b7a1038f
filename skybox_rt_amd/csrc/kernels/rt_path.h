// rt_path.h -- the path tracer's sampling routines, one form each, shared by
// pt_kernel.hip (every path vertex) and rt_kat.hip (known-answer tables,
// tests/test_gpu_ray_kat.py): the PCG hash stream, the bounce key, the
// hash -> [-1, 1) map, the cosine-weighted bounce direction (disk rejection
// sampling, PT_TRIES attempts, then the pole) and the geometric normal.
// Numerics as rt_trace.h: explicit fmaf, IEEE division and square root,
// restated op for op by the oracle (oracle/rt.c pcg_hash .. pt_normal).
#pragma once

#include "rt_trace.h"

#define PT_TRIES 8u      // disk rejection-sampling attempts (ORC_PT_TRIES)

namespace {

using namespace rtk;

__device__ __forceinline__ uint32_t pcg_hash(uint32_t v) {
  const uint32_t state = v * 747796405u + 2891336453u;
  const uint32_t word = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
  return (word >> 22u) ^ word;
}
__device__ __forceinline__ uint32_t pt_key(uint32_t seed, uint32_t px, uint32_t v) {
  return pcg_hash(px ^ pcg_hash(seed ^ (0x9E3779B9u * (v + 1u))));
}
__device__ __forceinline__ float pt_u11(uint32_t h) {
  return (float)(h >> 8) * 0x1p-23f - 1.0f;
}

// cosine-weighted direction about unit normal n (oracle pt_bounce_dir)
__device__ __forceinline__ void bounce_dir(const float n[3], uint32_t key, float dir[3]) {
  float x = 0.0f, y = 0.0f;
  for (uint32_t i = 0; i < PT_TRIES; ++i) {
    const float a = pt_u11(pcg_hash(key + 2u * i)), b = pt_u11(pcg_hash(key + 2u * i + 1u));
    if (fmaf(a, a, b * b) < 1.0f) { x = a; y = b; break; }
  }
  const float z = sqrtf(1.0f - fmaf(x, x, y * y));
  const float sgn = n[2] >= 0.0f ? 1.0f : -1.0f;
  const float a = -1.0f / (sgn + n[2]);
  const float b = (n[0] * n[1]) * a;
  const float t1[3] = {fmaf(sgn * (n[0] * n[0]), a, 1.0f), sgn * b, -(sgn * n[0])};
  const float t2[3] = {b, fmaf(n[1] * n[1], a, sgn), -n[1]};
#pragma unroll
  for (int k = 0; k < 3; ++k) dir[k] = fmaf(x, t1[k], fmaf(y, t2[k], z * n[k]));
}

// unit geometric normal facing against din (oracle pt_normal)
__device__ __forceinline__ void tri_normal(const float e1[3], const float e2[3], const float din[3],
                                           float n[3]) {
  cross3(n, e1, e2);
  const float len = sqrtf(dot3(n, n));
  n[0] = n[0] / len; n[1] = n[1] / len; n[2] = n[2] / len;
  if (dot3(n, din) > 0.0f) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
}

}  // namespace
