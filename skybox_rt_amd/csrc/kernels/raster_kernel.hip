// raster_kernel.hip -- the reference's draw3d hot path itself on gfx950
// (the full raster-parity pipeline): per drawcall,
// tile binning, homogeneous fixed-point edge functions, the draw3d shader
// (fixed-point interpolation, R5G6B5/... bilinear sampler) and the output
// merger (depth/stencil test, blending, write masks), pixel-exact with the
// reference's golden images through the oracle (oracle/raster.c).
//
// MI355X mapping: one 256-thread workgroup per raster tile -- 16x16 pixels,
// one per thread (RT_RASTER_TILE_LOG, default), or the reference's 32x32
// (RASTER_TILE_LOGSIZE = 5) with each thread owning a 2x2 quad (the
// reference's stamp, graphics.cpp:840, kernel.cpp:73-79).  Results do not
// depend on the tile size (per-pixel semantics; the oracle's tile-size
// invariance test); 16x16 gives 4x the workgroups and a 4x shorter
// per-thread pixel loop at 1024^2, where the 32x32 form ran one round of
// 1024 workgroups bound by its heaviest tile.  A pixel's
// colour and depth/stencil words stay in the owning thread's registers for
// the whole frame -- initialised to draw3d's clear values, written once -- so the order-dependent OM
// semantics of the reference (per-tile ascending primitive order,
// gpu_sw.h:38-61; drawcalls in order, draw3d/main.cpp:179) hold trivially.
// Binning (gfxutil.cpp:237-271) happens in the workgroup: each chunk of 256
// primitives is bbox-tested against the tile in parallel and compacted in
// order (ballot + mbcnt + a 4-wave prefix in LDS) into the tile's list; the
// listed primitives' records are staged in LDS during binning and read back
// as broadcasts.  One launch renders every drawcall of the frame.
#include <hip/hip_runtime.h>

#include "gfx_device.h"
#include "rt_common.h"
#include "vx_spawn.h"

#define RS_BLOCK 256

namespace {

constexpr int kWaves = RS_BLOCK / 64;

__device__ __forceinline__ uint32_t lane_id() {
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

struct RsLds {
  uint32_t list[RS_BLOCK];   // the tile's primitives (global pids) of one chunk, in order
  uint2 bb[RS_BLOCK];        // their screen boxes (per-pixel bin test, bins finer than the tile)
  uint32_t wave_n[kWaves];
  uint4 rec[RS_BLOCK][8];    // their rt_prim_t records (128 B each), staged during binning, same order
};

struct Frame {
  vx_arena A;
  uint32_t prims, dcs, oms, bbox, cbuf, zbuf;
  uint32_t width, height, tiles_x, num_dc, clear_color, clear_depth, tile_log;
  uint32_t bin_log;          // binning tile side 2^bin_log (RASTER_TILE_LOGSIZE, draw3d -k)
  bool coverage;             // the raster app: covered pixels white (raster/kernel.cpp:35-45)
};

// the reference bins a primitive to the tiles its screen box [x0, x1) x
// [y0, y1) reaches (gfxutil.cpp:237-250); does it reach the region [lo, hi)?
__device__ __forceinline__ bool bins_to(uint2 bb, uint32_t x_lo, uint32_t x_hi, uint32_t y_lo,
                                        uint32_t y_hi) {
  const uint32_t bx0 = bb.x & 0xffffu, bx1 = bb.x >> 16, by0 = bb.y & 0xffffu, by1 = bb.y >> 16;
  return bx0 < bx1 && bx0 < x_hi && bx1 > x_lo && by0 < y_hi && by1 > y_lo;
}

// thread -> its pixel group: g x g pixels at (gx, gy), g = tile side / 16
__device__ __forceinline__ void thread_pixels(const Frame& F, uint32_t tile, uint32_t t,
                                              uint32_t* gx, uint32_t* gy, uint32_t* g) {
  const uint32_t gs = 1u << (F.tile_log - 4);
  *g = gs;
  *gx = ((tile % F.tiles_x) << F.tile_log) + gs * (t & 15u);
  *gy = ((tile / F.tiles_x) << F.tile_log) + gs * (t >> 4);
}

__device__ __forceinline__ rt_omstate_t load_om(const vx_arena& A, uint32_t off) {
  rt_omstate_t s;
  uint32_t* w = reinterpret_cast<uint32_t*>(&s);
#pragma unroll
  for (int i = 0; i < 8; ++i) {  // all 32 words (128 B)
    const uint4 v = A.sld_u4(off + 16 * i);
    w[4 * i + 0] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
  }
  return s;
}

// the frame's drawcalls over one tile; col/ds = this thread's quad
__device__ __forceinline__ void render_tile(const Frame& F, uint32_t tile, RsLds& L, uint32_t col[4],
                                            uint32_t ds[4], uint32_t& frags) {
  const uint32_t x0 = (tile % F.tiles_x) << F.tile_log, y0 = (tile / F.tiles_x) << F.tile_log;
  // the bins this workgroup tile lies in: the enclosing bin when bins are at
  // least as large as the tile, else the tile itself (then every pixel also
  // tests its own bin below)
  const bool fine_bins = F.bin_log < F.tile_log;
  const uint32_t bmask = fine_bins ? ((1u << F.tile_log) - 1u) : ((1u << F.bin_log) - 1u);
  const uint32_t bx_lo = x0 & ~bmask, bx_hi = bx_lo + bmask + 1u;
  const uint32_t by_lo = y0 & ~bmask, by_hi = by_lo + bmask + 1u;
  const uint32_t pmask = (1u << F.bin_log) - 1u;
  uint32_t qx, qy, gs;
  thread_pixels(F, tile, threadIdx.x, &qx, &qy, &gs);
  const uint32_t npx = gs * gs;
  const uint32_t w = threadIdx.x >> 6;
  for (uint32_t d = 0; d < F.num_dc; ++d) {
    const rt_omstate_t om = load_om(F.A, F.oms + 128u * d);
    const gfx::DcState st = gfx::load_dcstate<true>(F.A, F.dcs + 64u * d);
    for (uint32_t base = 0; base < om.prim_count; base += RS_BLOCK) {
      // bin: which primitives of this chunk touch the tile (bbox, pixels)
      const uint32_t i = base + threadIdx.x;
      bool ov = false;
      uint32_t g = 0;
      uint2 bb = make_uint2(0u, 0u);
      if (i < om.prim_count) {
        g = om.prim_offset + i;
        bb = make_uint2(F.A.ld_u32(F.bbox + 8u * g), F.A.ld_u32(F.bbox + 8u * g + 4));
        // binned at the reference's granularity whatever this workgroup's
        // tile size: fixed-point coverage can reach a few pixels past the
        // float bbox, and the reference covers those pixels iff they lie in
        // a tile the primitive was binned to
        ov = bins_to(bb, bx_lo, bx_hi, by_lo, by_hi);
      }
      const uint64_t m = __ballot(ov);
      if (lane_id() == 0) L.wave_n[w] = (uint32_t)__popcll(m);
      __syncthreads();
      uint32_t pre = 0, n = 0;
#pragma unroll
      for (int k = 0; k < kWaves; ++k) {
        const uint32_t c = L.wave_n[k];
        pre += (uint32_t)k < w ? c : 0u;
        n += c;
      }
      if (ov) {
        const uint32_t r = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        L.list[pre + r] = g;
        L.bb[pre + r] = bb;
#pragma unroll
        for (int k = 0; k < 8; ++k) L.rec[pre + r][k] = F.A.ld_u4(F.prims + 128u * g + 16u * k);
      }
      __syncthreads();
      // rasterize the listed primitives in order
      for (uint32_t k = 0; k < n; ++k) {
        gfx::Prim p;
#pragma unroll
        for (int i = 0; i < 8; ++i) {  // broadcast LDS reads
          const uint4 v = L.rec[k][i];
          p.w[4 * i + 0] = (int32_t)v.x; p.w[4 * i + 1] = (int32_t)v.y;
          p.w[4 * i + 2] = (int32_t)v.z; p.w[4 * i + 3] = (int32_t)v.w;
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          if (j >= npx) break;
          const uint32_t x = qx + (j & 1u), y = qy + (j >> 1);
          int32_t e[3];
          // inclusive coverage, no top-left rule, viewport scissor
          // (graphics.cpp:813-825; the edge KAT image tests gfx::covers)
          bool in = gfx::covers(p.edge(0), x, y, e) && x < F.width && y < F.height;
          const int32_t e0 = e[0], e1 = e[1], e2 = e[2];
          if (fine_bins)  // the pixel's own bin must be one the primitive was binned to
            in = in && bins_to(L.bb[k], x & ~pmask, (x & ~pmask) + pmask + 1u, y & ~pmask,
                               (y & ~pmask) + pmask + 1u);
          if (in) {
            if (F.coverage) {
              col[j] = 0xffffffffu;
            } else {
              uint32_t z;
              const uint32_t c = gfx::shade_edges(F.A, p, st, e0, e1, e2, &z);
              gfx::om_write(om, col[j], ds[j], c, z);
            }
            ++frags;
          }
        }
      }
      __syncthreads();  // the list is rebuilt for the next chunk
    }
  }
}

__device__ __forceinline__ void flush(int slot, uint32_t v) { vx_mpm_add(RT_MPM_USER + slot, v); }

}  // namespace

VX_MAIN(rt_kernel_arg_t, arg, RS_BLOCK) {
  __shared__ RsLds s_rs;
  Frame F;
  F.A = vx_arena::get();
  F.prims = (uint32_t)arg->prims_addr;
  F.dcs = (uint32_t)arg->dcs_addr;
  F.oms = (uint32_t)arg->oms_addr;
  F.bbox = (uint32_t)arg->bbox_addr;
  F.cbuf = (uint32_t)arg->cbuf_addr;
  F.zbuf = (uint32_t)arg->zbuf_addr;
  F.width = arg->width;
  F.height = arg->height;
  F.tiles_x = arg->tiles_x;
  F.num_dc = arg->num_drawcalls;
  F.clear_color = arg->clear_color;
  F.clear_depth = 0xffffffffu;
  F.tile_log = arg->raster_tile_log;
  F.bin_log = arg->raster_bin_log;
  F.coverage = (arg->flags & RT_FLAG_COVERAGE) != 0;
  uint32_t frags = 0, pixels = 0;
  uint32_t col[4], ds[4], qx = 0, qy = 0, npx = 1;
  // task = one thread's pixel group; a workgroup step = one tile
  const int rc = vx_spawn_tasks_block(
      arg->num_tasks,
      [&](const vx_task_t& task, bool valid, const Frame* f) {
        uint32_t gs;
        thread_pixels(*f, task.blockIdx.x / RS_BLOCK, task.blockIdx.x % RS_BLOCK, &qx, &qy, &gs);
        npx = gs * gs;
        // the frame starts from draw3d's clears (main.cpp:478-490: colour
        // 0xff000000, depth/stencil 0xffffffff), fused here: no read-back
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
          const uint32_t px = qx + (j & 1u), py = qy + (j >> 1);
          col[j] = f->clear_color;
          ds[j] = f->clear_depth;
          pixels += j < npx && valid && px < f->width && py < f->height;
        }
      },
      [&](uint32_t step, const Frame* f) {
        render_tile(*f, step, s_rs, col, ds, frags);
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {  // ... and written once
          const uint32_t px = qx + (j & 1u), py = qy + (j >> 1);
          if (j < npx && px < f->width && py < f->height) {
            const uint32_t o = 4u * (py * f->width + px);
            f->A.st_u32(f->cbuf + o, col[j]);
            f->A.st_u32(f->zbuf + o, ds[j]);
          }
        }
      },
      &F);
  flush(RT_STAT_PRIMARY, pixels);
  flush(RT_STAT_SHADED, frags);
  return rc;
}
