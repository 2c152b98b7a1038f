// rt_kat.hip -- the ray routines of rt_trace.h and rt_path.h (the functions
// every ray of rt_kernel / pt_kernel / rt_om / rt_aov calls, never a copy)
// over tables of records, for known-answer tests against the exact model
// (tests/ray_reference.py, tests/test_gpu_ray_kat.py).  Thread per record, one
// wave per workgroup; a mode word selects the table:
//   MT    mt_hit and mt_hit_bf of one ray and one triangle
//   SLAB  slab and slab_nf of one ray (after ray_setup) and one box, the
//         planes once as fp32 and once as the binary16 values a rt_node4h_t
//         holds (converted by the cast node4_step<., true> applies)
//   WALK  every BVH walk over a scene the argument block describes (node and
//         triangle arrays uploaded by the test): trace closest and any,
//         occluded_packet, trace_coop, and trace_flat_range over the whole
//         list -- the device's own brute force -- one ray per lane, each lane
//         with its own limits, skip pid, tie rule and activity bit
//   PT    pcg_hash, pt_key, pt_u11, bounce_dir, tri_normal
// A slot of the output a record does not produce (an inactive lane, a walk
// form the tree's layout has no code for) keeps what the test filled it with.
#include <hip/hip_runtime.h>

#define VX_BLOCK_THREADS 64  // vx_spawn.h: the workgroup size as a constant
#include "rt_trace.h"
#include "rt_path.h"

#define KAT_MT 0u
#define KAT_SLAB 1u
#define KAT_WALK 2u
#define KAT_PT 3u

#define KAT_MT_REC 16u     // o[3] d[3] v0[3] e1[3] e2[3] tmin
#define KAT_MT_OUT 4u      // mt_hit verdict, t | mt_hit_bf verdict, t (t: 0 on a miss)
#define KAT_SLAB_REC 20u   // o[3] d[3] planes[6] tmin tmax half[3] (lo | hi << 16 per axis) pad[3]
#define KAT_SLAB_OUT 8u    // per plane set: slab | slab_nf << 1, slab tnear, slab_nf tnear, tfar
#define KAT_WALK_REC 12u   // o[3] d[3] tmin tmax skip flags (1 tie_high, 2 active) pad[2]
#define KAT_WALK_OUT 12u   // see walk_body
#define KAT_PT_REC 20u     // v seed px vertex h key n[3] e1[3] e2[3] din[3] pad[2]
#define KAT_PT_OUT 12u     // pcg_hash pt_key pt_u11 dir[3] normal[3] pad[3]

typedef struct {
  uint32_t mode, count;
  uint64_t rec_addr;    // uint32 [count * <mode>_REC]
  uint64_t out_addr;    // uint32 [count * <mode>_OUT]
  // WALK: the scene (every address below 4 GiB)
  uint64_t nodes_addr;  // rt_node_t [num_nodes]
  uint64_t nodes4_addr; // rt_node4_t [num_nodes4], then rt_node4h_t [num_nodes4]
  uint64_t tris_addr;   // rt_tri_t [leaf order] + 3 padding records
  uint64_t geom_addr;   // rt_tri_t [num_geom], ascending pid
  uint32_t num_nodes, num_nodes4, num_geom, flags;  // flags: RT_FLAG_BVH4 / RT_FLAG_BVH4H
} rt_kat_arg_t;

namespace {

using namespace rtk;

__device__ __forceinline__ float f32(uint32_t u) { return __uint_as_float(u); }
__device__ __forceinline__ uint32_t u32(float f) { return __float_as_uint(f); }

__device__ __forceinline__ void mt_body(uint32_t i, const rt_kat_arg_t* a) {
  const uint32_t* q = vx_ptr<uint32_t>(a->rec_addr) + KAT_MT_REC * i;
  Ray r;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.o[k] = f32(q[k]);
    r.d[k] = f32(q[3 + k]);
    r.inv[k] = r.oi[k] = 0.0f;
  }
  const float4 v0 = make_float4(f32(q[6]), f32(q[7]), f32(q[8]), 0.0f);
  const float4 e1 = make_float4(f32(q[9]), f32(q[10]), f32(q[11]), 0.0f);
  const float4 e2 = make_float4(f32(q[12]), f32(q[13]), f32(q[14]), 0.0f);
  const float tmin = f32(q[15]);
  uint32_t* out = vx_ptr<uint32_t>(a->out_addr) + KAT_MT_OUT * i;
  float t = 0.0f, tb = 0.0f;
  const bool h = mt_hit(r, v0, e1, e2, tmin, &t);
  const bool hb = mt_hit_bf(r, v0, e1, e2, tmin, &tb);
  out[0] = h ? 1u : 0u;
  out[1] = h ? u32(t) : 0u;
  out[2] = hb ? 1u : 0u;
  out[3] = hb ? u32(tb) : 0u;
}

__device__ __forceinline__ void slab_body(uint32_t i, const rt_kat_arg_t* a) {
  const uint32_t* q = vx_ptr<uint32_t>(a->rec_addr) + KAT_SLAB_REC * i;
  Ray r;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.o[k] = f32(q[k]);
    r.d[k] = f32(q[3 + k]);
  }
  ray_setup(r);
  const float tmin = f32(q[12]), tmax = f32(q[13]);
  uint32_t* out = vx_ptr<uint32_t>(a->out_addr) + KAT_SLAB_OUT * i;
#pragma unroll
  for (int set = 0; set < 2; ++set) {
    float p[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (set == 0) {
        p[2 * k] = f32(q[6 + 2 * k]);
        p[2 * k + 1] = f32(q[7 + 2 * k]);
      } else {  // node4_step<., true>'s conversion of a record's halves
        const uint32_t u = q[14 + k];
        p[2 * k] = (float)__builtin_bit_cast(_Float16, (uint16_t)(u & 0xffffu));
        p[2 * k + 1] = (float)__builtin_bit_cast(_Float16, (uint16_t)(u >> 16));
      }
    }
    float tn = 0.0f, tn2 = 0.0f, tf = 0.0f;
    const bool h = slab(p[0], p[1], p[2], p[3], p[4], p[5], r, tmin, tmax, &tn);
    const bool h2 = slab_nf(p[0], p[1], p[2], p[3], p[4], p[5], r, tmin, tmax, &tn2, &tf);
    out[4 * set] = (h ? 1u : 0u) | (h2 ? 2u : 0u);
    out[4 * set + 1] = u32(tn);
    out[4 * set + 2] = u32(tn2);
    out[4 * set + 3] = u32(tf);
  }
}

__device__ __forceinline__ void pt_body(uint32_t i, const rt_kat_arg_t* a) {
  const uint32_t* q = vx_ptr<uint32_t>(a->rec_addr) + KAT_PT_REC * i;
  uint32_t* out = vx_ptr<uint32_t>(a->out_addr) + KAT_PT_OUT * i;
  out[0] = pcg_hash(q[0]);
  out[1] = pt_key(q[1], q[2], q[3]);
  out[2] = u32(pt_u11(q[4]));
  const float n[3] = {f32(q[6]), f32(q[7]), f32(q[8])};
  float dir[3];
  bounce_dir(n, q[5], dir);
  const float e1[3] = {f32(q[9]), f32(q[10]), f32(q[11])}, e2[3] = {f32(q[12]), f32(q[13]), f32(q[14])};
  const float din[3] = {f32(q[15]), f32(q[16]), f32(q[17])};
  float nn[3];
  tri_normal(e1, e2, din, nn);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    out[3 + k] = u32(dir[k]);
    out[6 + k] = u32(nn[k]);
  }
}

// the Scene fields the walks read, from the argument block (wave-uniform
// values: the walks form scalar addresses from them); everything else 0
__device__ __forceinline__ Scene kat_scene(const rt_kat_arg_t* a) {
  auto uni = [](uint64_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v); };
  Scene s;
  s.A = vx_arena::get();
  s.nodes = uni(a->nodes_addr);
  s.nodes4 = uni(a->nodes4_addr);
  s.tris = uni(a->tris_addr);
  s.geom = uni(a->geom_addr);
  s.num_nodes = uni(a->num_nodes);
  s.num_nodes4 = uni(a->num_nodes4);
  s.num_geom = uni(a->num_geom);
  s.flags = uni(a->flags);
  s.prims = s.dcs = s.cbuf = s.ptris = s.order = 0;
  s.vnodes = s.vtris = s.vlayers = s.vgeom = s.num_vnodes = 0;
  s.num_layer = s.width = s.height = s.shard_index = s.shard_count = s.tiles_x = 0;
  s.clear_color = s.bounces = s.seed = s.split_tiles = s.split_log = s.tiles_x_magic = s.num_tasks = 0;
  s.sx = s.sy = s.light[0] = s.light[1] = s.light[2] = 0.0f;
  s.argp = 0;
  s.blist = s.bidx = s.blist_blocks = s.sidx = s.slist = s.slist_on = s.slist_n = 0;
  s.cdesc = s.cdesc_first = s.lw3 = 0;
  return s;
}

// One ray per lane.  Output words of a lane (active lanes only):
//   0, 1   trace<false> over the tree's layout: pid, t (0 on a miss)
//   2      trace<true>: occluded
//   3      occluded_packet (binary16 BVH4 only): occluded, from 0 below tmax
//   4, 5   trace_coop (binary16 BVH4 only): pid, t, from 0 below +inf
//   6, 7   trace_flat_range<false> over [0, num_geom): pid, t
//   8      trace_flat_range<true>: occluded
//   9, 10  trace_flat_range<false> from 0 below +inf: pid, t (trace_coop's limits)
//   11     trace_flat_range<true> from 0 below tmax (occluded_packet's limits)
// All 64 lanes of the wave are here (the launch's count is a multiple of 64):
// occluded_packet is called by every lane with its activity bit, as the frame
// kernels call it; trace_coop runs by lane pairs 2p, 2p + 1 holding one ray,
// as the path tracer calls it -- first the lower lane's ray, then the upper
// lane's, the pair tracing a ray when its owner is active and the owner
// storing the result, so a pair with one idle lane still walks with both.
__device__ __forceinline__ void walk_body(uint32_t i, const rt_kat_arg_t* a, int32_t* stack) {
  const uint32_t* q = vx_ptr<uint32_t>(a->rec_addr) + KAT_WALK_REC * i;
  uint32_t* out = vx_ptr<uint32_t>(a->out_addr) + KAT_WALK_OUT * i;
  const Scene S = kat_scene(a);
  Counters cnt;
  Ray r;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    r.o[k] = f32(q[k]);
    r.d[k] = f32(q[3 + k]);
  }
  ray_setup(r);
  const float tmin = f32(q[6]), tmax = f32(q[7]);
  const int32_t skip = (int32_t)q[8];
  const bool tie_high = (q[9] & 1u) != 0u, act = (q[9] & 2u) != 0u;
  const uint32_t n = S.num_geom;
  if (act) {
    float t = 0.0f;
    uint32_t first;
    int32_t p = trace<false>(S, r, tmin, tmax, skip, tie_high, &t, stack, cnt);
    out[0] = (uint32_t)p;
    out[1] = p >= 0 ? u32(t) : 0u;
    out[2] = trace<true>(S, r, tmin, tmax, skip, tie_high, &t, stack, cnt) >= 0 ? 1u : 0u;
    p = trace_flat_range<false>(S, r, 0u, n, tmin, tmax, skip, tie_high, &t, &first);
    out[6] = (uint32_t)p;
    out[7] = p >= 0 ? u32(t) : 0u;
    out[8] = trace_flat_range<true>(S, r, 0u, n, tmin, tmax, skip, tie_high, &t, &first) >= 0 ? 1u : 0u;
    p = trace_flat_range<false>(S, r, 0u, n, 0.0f, INFINITY, skip, tie_high, &t, &first);
    out[9] = (uint32_t)p;
    out[10] = p >= 0 ? u32(t) : 0u;
    out[11] = trace_flat_range<true>(S, r, 0u, n, 0.0f, tmax, skip, tie_high, &t, &first) >= 0 ? 1u : 0u;
  }
  if ((S.flags & RT_FLAG_BVH4H) == 0u) return;  // wave-uniform
  const bool occ = occluded_packet(S, r, act, skip, tmax, cnt);
  if (act) out[3] = occ ? 1u : 0u;
  const int ln = (int)lane_id();
  const bool hi = (ln & 1) != 0;
  int32_t* pstack = hi ? stack - 1 : stack;  // the pair's stack: lane 2p's column
  for (int pass = 0; pass < 2; ++pass) {
    const int src = (ln & ~1) | pass;  // the pair's lane whose ray this pass traces
    Ray c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c.o[k] = __shfl(r.o[k], src);
      c.d[k] = __shfl(r.d[k], src);
    }
    ray_setup(c);
    const int32_t cskip = __shfl(skip, src);
    const bool ctie = __shfl((int)tie_high, src) != 0, cact = __shfl((int)act, src) != 0;
    if (cact) {
      float t = 0.0f;
      const int32_t p = trace_coop(S, c, cskip, ctie, &t, pstack, hi, cnt);
      if (ln == src) {
        out[4] = (uint32_t)p;
        out[5] = p >= 0 ? u32(t) : 0u;
      }
    }
  }
}

}  // namespace

VX_MAIN(rt_kat_arg_t, arg, 64) {
  __shared__ int32_t s_stack[RT_STACK_ROWS][64];
  int32_t* stack = &s_stack[0][lane_id()];
  const uint32_t mode = arg->mode;
  // (a walk table runs whole waves: its record count is a multiple of 64)
  if (mode > KAT_PT || (mode == KAT_WALK && (arg->count & 63u) != 0u)) return -1;
  return vx_spawn_tasks(
      arg->count,
      [&](const vx_task_t& t, rt_kat_arg_t* a) {
        if (mode == KAT_MT) mt_body(t.task_id, a);
        else if (mode == KAT_SLAB) slab_body(t.task_id, a);
        else if (mode == KAT_WALK) walk_body(t.task_id, a, stack);
        else pt_body(t.task_id, a);
      },
      arg);
}
