// rt_btrim_kernel.hip -- the block lists trimmed to their winners, once per configure
// (setup_common.h rt_btrim_arg_t).  A block's candidate list holds every
// geometry primitive whose covered rectangle reaches the block; which of them win a pixel depends
// on the scene, the size and the shard -- configure's inputs -- and not on the light, so the
// frames' scans need not read the others again every frame.
//
// One wave per local 8x8 block, on rt_kernel's whole-block task map (chunk_map / chunk_pixel /
// block_header under an argument block without work order or split tiles: chunk c is block c).
// The wave runs block_primary itself, with the scene's tie rule, so the coverage and depth rule
// stands once; then, entry by entry, it ballots "this lane's pixel is in the image and its winner
// is the entry's primitive" and one lane writes the kept entries to the front of the list's slots
// in btrim and the header (bidx's offset, the kept count) to btidx.  The other lanes copy the
// list's remaining slots from blist.  A pixel's winner is the best covering entry under
// vis_better, a total order; it is kept, so the best of the kept entries is the same primitive.
#include <hip/hip_runtime.h>

#ifndef RT_BLOCK_THREADS
#define RT_BLOCK_THREADS 64
#endif
#define VX_BLOCK_THREADS RT_BLOCK_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "rt_trace.h"
#include "setup_common.h"

namespace {

using namespace rtk;

struct Trim {
  uint32_t btrim, btidx, stat, entries;  // arena offsets (the host keeps them below 4 GiB)
};

__device__ __forceinline__ void kernel_body(const vx_task_t& task, const Scene& S, const Trim& T, Counters& cnt) {
  const uint32_t t = task.blockIdx.x;
  const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane(t) >> 6;
  const ChunkMap cm = chunk_map(S, task_args(S), c);
  uint32_t x, y, out;
  chunk_pixel(S, cm, t & 63u, &x, &y, &out);
  const uint32_t lb = (cm.lt << 4) | cm.blk;
  if (lb >= rt_usgpr(S.blist_blocks)) return;
  const bool in = x < S.width && y < S.height;  // edge tiles overhang the image
  const bool tie_high = (S.flags & RT_FLAG_TIE_HIGH) != 0;
  const uint2 oc = block_header(S, lb);
  const int32_t hit = block_primary(S, oc, x, y, in, tie_high, cnt);
  const uint32_t l = lane_id();
  uint32_t kept = 0;  // wave-uniform
  for (uint32_t k = 0; k < oc.y; ++k) {
    const uint4 e = S.A.sld_u4(S.blist + 16u * (oc.x + k));
    const int32_t pid = (int32_t)S.A.sld<uint32_t>(S.vgeom + 64u * e.x + 44u);  // rt_vtri_t::pid
    if (__ballot(in && hit == pid) == 0) continue;
    if (l == 0) S.A.st_u4(T.btrim + 16u * (oc.x + kept), e);
    ++kept;
  }
  // the slots behind the kept entries: the list's own entries, as a scan may load them ahead
  for (uint32_t k = kept + l; k < oc.y; k += 64u)
    S.A.st_u4(T.btrim + 16u * (oc.x + k), S.A.ld_u4(S.blist + 16u * (oc.x + k)));
  if (l == 0) {
    S.A.st_u32(T.btidx + 8u * lb, oc.x);
    S.A.st_u32(T.btidx + 8u * lb + 4u, kept);
    if (kept) {
      atomicAdd(vx_ptr<uint32_t>(T.stat), kept);
      atomicAdd(vx_ptr<uint32_t>(T.stat + 4u), 1u);
    }
  }
  // the padding entries behind the last list (block 0's wave)
  if (lb == 0 && l < RT_BLIST_PAD)
    S.A.st_u4(T.btrim + 16u * (T.entries + l), make_uint4(0u, RT_BLIST_PAD_LO, RT_BLIST_PAD_HI, RT_VIS_ZMIN_NONE));
}

}  // namespace

VX_MAIN(rt_kernel_arg_t, arg, RT_BLOCK_THREADS) {
  Counters cnt;
  Scene S = load_scene(arg, vx_launch_words);
  const auto* ta = arg_at<rt_btrim_arg_t>(S, RT_BTRIM_ARG_OFFSET);
  const Trim T{(uint32_t)ta->btrim_addr, (uint32_t)ta->btidx_addr, (uint32_t)ta->stat_addr, ta->entries};
  return vx_spawn_tasks(
      S.num_tasks, [&](const vx_task_t& task, const Scene* s) { kernel_body(task, *s, T, cnt); }, &S);
}
