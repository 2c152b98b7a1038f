// rt_denoise_kernel.hip -- the edge-avoiding a-trous filter over the accumulation records of a
// path frame (vx_rt.h rt_render_denoise_start states the definition; rt_common.h rt_dn_* are its
// integer pieces, shared with the host).  One source, two images:
//
// rt_denoise_prep (DN_PASS=0): a streaming pass, one pixel per lane, in rt_relight_kernel.hip's
// shape -- per framebuffer pixel the accumulation record (16 B), the guide record (16 B) and the
// base colour (4 B) in, two 8-B tap records out.  A geometry pixel's mean radiance is demodulated
// by its base colour into three 16-bit irradiances; any other pixel is resolved here
// (rt_accum_resolve) and carried through the passes as its finished ARGB word, so no pass reads a
// 16-B record again.
//
// What a tap reads.  A tap needs 129 bits of its pixel: three u16 irradiances, the pid, the 24-bit
// depth word, three normal bytes and the geometry flag.  The flag is folded into the pid (a pixel
// without geometry stores RT_DN_NO_GEOM there: a geometry winner's pid is never -1), which leaves
// 128 bits, split by what changes: {pid, z | Nx << 24} is written once by the prepare pass,
// {I_R | I_G << 16, I_B | Ny << 16 | Nz << 24} is what a pass rewrites (Ny, Nz copied through), so
// the ping-pong buffers are 8 B a pixel and a pass stores 8 B, not 16.  A tap is two 8-B loads;
// consecutive lanes read consecutive pixels of a row, 512 B contiguous per wave and load.  Neither
// the 16-B guide record nor the 16-B accumulation record is touched by a tap (the reasoning of
// rt_relight_kernel.hip's header, the other way round: there both words sit in one record).
//
// rt_denoise_pass (DN_PASS=1): pass k of P, stride 2^(k-1), 5 x 5 taps gathered around every
// geometry pixel from irr[(k-1) & 1] into irr[k & 1]; the last pass (RT_DN_TAG_LAST) remodulates
// by the base colour and stores the ARGB pixel to the framebuffer in use instead.  A 256-thread
// workgroup takes tiles of 64 x DN_TILE_H pixels, wave w rows (DN_THREADS / 64) s + w of the tile,
// lane l column l.  The pass is bound by instructions, not by bytes: a wave with a geometry pixel
// issues 48 8-B tap loads and about 1 350 vector and 530 scalar instructions for its 64 pixels, a
// wave without one loads, tests and stores (24 B a pixel).  Geometry clusters, so the launch ends
// when the workgroups on the geometry's tiles do: DN_TILE_H = 4 (one row per wave; 4 096 tiles at
// 1024^2) over 16 (four rows per wave in turn; the vertically adjacent rows of a step then sit in
// the CU's vector cache) measured 0.0346 against 0.0476 ms at stride 1 and 0.0341 against 0.0456 ms
// at stride 16 (tekkaman 1024^2, a tenth of the pixels geometry); 64- and 128-thread workgroups of
// one row per wave on grids of 16 to 64 per CU came to the same 0.031 - 0.035 ms.  The taps come
// from the vector cache and the XCD's L2 (a 1024^2 working set is 16 MiB of tap records, 4 MiB of
// L2 per XCD).  No LDS: staging the 64 x 16 tile with its halo (DN_LDS=1, Makefile variants/dn_lds)
// measured 2 % slower at stride 1 and 10 % at stride 2.  Grid: the module's 8
// workgroups per CU; larger frames stride over their tiles.
//
// Every sum fits 32 bits: the 25 kernel weights sum to 256, an edge weight is at most 256 and an
// irradiance at most 65535, so a numerator is at most 256 * 256 * 65535 and the rounding term
// den / 2 at most 32768 -- 256 * 256 * 65535 + 32768 < 2^32.
//
// Wave-uniform inputs: pass, last-pass flag and framebuffer in the launch tag (RT_DN_TAG_*), the
// two shifts in the launch words, buffers and size in the argument areas through the scalar cache.
#include <hip/hip_runtime.h>

#ifndef DN_PASS
#define DN_PASS 0
#endif
#ifndef DN_LDS
#define DN_LDS 0
#endif
#ifndef DN_THREADS
#define DN_THREADS 256
#endif
// (the gather keeps 5 workgroups on a CU: 96 VGPRs; the compiler's own choice was 98 and 4)
#ifndef DN_WAVES_PER_SIMD
#define DN_WAVES_PER_SIMD 5
#endif
#ifndef DN_TILE_H
#define DN_TILE_H 4
#endif
#define VX_BLOCK_THREADS DN_THREADS  // vx_spawn.h: the workgroup size as a constant
#include "vx_spawn.h"
#include "rt_common.h"

// workgroups per CU (hip_driver.cpp reads it): 2048 on the chip, the streaming kernels' cap
#ifndef DN_GRID_PER_CU
#define DN_GRID_PER_CU 8
#endif
__device__ __attribute__((used)) uint32_t __vx_grid_per_cu = DN_GRID_PER_CU;

namespace {

__device__ __forceinline__ uint32_t sgpr(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ void st_u2(const vx_arena& A, uint32_t off, uint2 v) {
  typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
  const u32x2 w = {v.x, v.y};
  __builtin_amdgcn_raw_buffer_store_b64(w, A.r, off, 0, 0);
}

#if DN_PASS
__device__ __forceinline__ uint32_t absdiff(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }

// The filtered irradiance of one geometry pixel from its own tap records (gp, ip) and 24 fetched
// ones: fetch(i, j, gq, iq) gives tap p + st * (i, j)'s records and whether it lies inside the
// image (a tap outside, or one without geometry, weighs 0).  Returns {R | G << 16, B}.
template <typename F>
__device__ __forceinline__ uint2 filter_pixel(const uint2 gp, const uint2 ip, uint32_t zsh, uint32_t ls, F&& fetch) {
  const uint32_t zp = gp.y & 0xffffffu, np = (gp.y >> 24) | ((ip.y >> 16) << 8);
  const uint32_t pr = ip.x & 0xffffu, pg = ip.x >> 16, pb = ip.y & 0xffffu;
  // the centre tap: h = 36, w = 256
  uint32_t den = 36u * 256u, sr = den * pr, sg = den * pg, sb = den * pb;
#pragma unroll
  for (int j = -2; j <= 2; ++j) {
    const uint32_t hj = j == 0 ? 6u : (j == -1 || j == 1) ? 4u : 1u;
#pragma unroll
    for (int i = -2; i <= 2; ++i) {
      if (i == 0 && j == 0) continue;
      uint2 gq, iq;
      const bool v = fetch(i, j, gq, iq);
      const uint32_t hi = i == 0 ? 6u : (i == -1 || i == 1) ? 4u : 1u;
      const uint32_t qr = iq.x & 0xffffu, qg = iq.x >> 16, qb = iq.y & 0xffffu;
      uint32_t wz = 256u, wn = 256u;
      if (gq.x != gp.x) {
        wz = rt_dn_stop(absdiff(zp, gq.y & 0xffffffu) >> zsh);
        wn = rt_dn_wn(np, (gq.y >> 24) | ((iq.y >> 16) << 8));
      }
      const uint32_t dl = max(max(absdiff(pr, qr), absdiff(pg, qg)), absdiff(pb, qb));
      const uint32_t wl = rt_dn_stop(dl >> ls);
      const uint32_t w = (v && gq.x != RT_DN_NO_GEOM) ? hi * hj * ((wz * wn * wl) >> 16) : 0u;
      den += w;
      sr += w * qr;
      sg += w * qg;
      sb += w * qb;
    }
  }
  // (256 * 256 * 65535 + 32768 < 2^32: the header)
  const uint32_t fr = (sr + (den >> 1)) / den, fg = (sg + (den >> 1)) / den, fb = (sb + (den >> 1)) / den;
  return make_uint2(fr | (fg << 16), fb);
}
#else
// one channel of rt_accum_resolve: the rounded mean (2 s + n) / (2 n), at most 255; 0 for n = 0
__device__ __forceinline__ uint32_t mean8(uint32_t s, uint32_t n) {
  if (n == 0) return 0u;
  const uint64_t m = (2u * (uint64_t)s + n) / (2u * (uint64_t)n);
  return m > 255u ? 255u : (uint32_t)m;
}
#endif

}  // namespace

VX_MAIN_BOUNDS(rt_kernel_arg_t, arg, __launch_bounds__(DN_THREADS, DN_WAVES_PER_SIMD)) {
  const vx_arena A = vx_arena::get();
  // the argument areas through the scalar cache (constant during the launch)
  const uint64_t ap = ((uint64_t)sgpr((uint32_t)((uint64_t)arg >> 32)) << 32) | sgpr((uint32_t)(uint64_t)arg);
  const auto* da = (const __attribute__((address_space(4))) rt_denoise_arg_t*)(ap + RT_DENOISE_ARG_OFFSET);
  const uint32_t W = da->width, H = da->height;
  const uint32_t tapg = (uint32_t)da->tapg_addr;
#if !DN_PASS
  const auto* ca = (const __attribute__((address_space(4))) rt_accum_arg_t*)(ap + sizeof(rt_kernel_arg_t));
  const uint32_t acc = (uint32_t)ca->accum_addr, guide = (uint32_t)da->guide_addr, base = (uint32_t)da->base_addr;
  const uint32_t irr = (uint32_t)da->irr_addr[0];
  const uint32_t npix = W * H;
  __vx_declare_tasks(npix);
  const uint32_t nwaves = gridDim.x * (DN_THREADS / 64u);
  const uint32_t wave = blockIdx.x * (DN_THREADS / 64u) + (threadIdx.x >> 6);
  for (uint32_t p0 = sgpr(wave * 64u); p0 < npix; p0 += nwaves * 64u) {
    const uint32_t p = p0 + (threadIdx.x & 63u);
    // (past the end: the last pixel's loads, results unused, no store)
    const uint32_t q = p < npix ? p : npix - 1u;
    const uint4 rec = A.ld_u4(acc + 16u * q), g = A.ld_u4(guide + 16u * q);
    const uint32_t a = A.ld_u32(base + 4u * q);
    uint2 t, i;
    if (g.y & RT_AOV_GEOM) {
      const uint32_t ir = rt_dn_demod(rec.x, rec.w, (a >> 16) & 0xffu);
      const uint32_t ig = rt_dn_demod(rec.y, rec.w, (a >> 8) & 0xffu);
      const uint32_t ib = rt_dn_demod(rec.z, rec.w, a & 0xffu);
      t = make_uint2(g.x, (g.y & 0xffffffu) | (g.z << 24));
      i = make_uint2(ir | (ig << 16), ib | (((g.z >> 8) & 0xffffu) << 16));
    } else {
      t = make_uint2(RT_DN_NO_GEOM, 0u);
      i = make_uint2((a & 0xff000000u) | (mean8(rec.x, rec.w) << 16) | (mean8(rec.y, rec.w) << 8) |
                         mean8(rec.z, rec.w), 0u);
    }
    if (p < npix) {
      st_u2(A, tapg + 8u * p, t);
      st_u2(A, irr + 8u * p, i);
    }
  }
#else
  const auto* ka = (const __attribute__((address_space(4))) rt_kernel_arg_t*)ap;
  const uint32_t tag = sgpr(vx_launch_tag);
  const uint32_t k = tag & RT_DN_TAG_K_MASK;  // 1..5 (rt_app checks)
  const bool last = (tag & RT_DN_TAG_LAST) != 0;
  const uint32_t zsh = sgpr(vx_launch_words.w[0]) + k - 1u, ls = sgpr(vx_launch_words.w[1]);
  const int32_t st = 1 << (k - 1u);
  const uint32_t src = (uint32_t)da->irr_addr[(k - 1u) & 1u], dst = (uint32_t)da->irr_addr[k & 1u];
  const uint32_t base = (uint32_t)da->base_addr;
  const uint32_t fb = (uint32_t)ka->cbuf_addr + ((tag & RT_DN_TAG_CBUF1) ? da->cbuf1_off : 0u);
  __vx_declare_tasks(W * H);
  const uint32_t ntx = (W + 63u) >> 6, nty = (H + DN_TILE_H - 1u) / DN_TILE_H;
  const uint32_t lane = threadIdx.x & 63u, row = threadIdx.x >> 6;
#if DN_LDS
  // the A/B variant (Makefile: variants/dn_lds): at strides 1 and 2 the workgroup stages its tile
  // with a halo of 2 st pixels in LDS, one 16-B entry per pixel (a pixel outside the image as one
  // without geometry), and the taps are LDS reads; strides 4 to 16 gather as the shipped image does
  __shared__ uint4 s_tile[(DN_TILE_H + 8) * (64 + 8)];
  const bool staged = st <= 2;
  const int32_t R = 2 * st;
  const uint32_t tw = 64u + 2u * (uint32_t)R, th = DN_TILE_H + 2u * (uint32_t)R;
#endif
  for (uint32_t tile = blockIdx.x; tile < ntx * nty; tile += gridDim.x) {
    const uint32_t ty = sgpr(tile / ntx), tx = tile - ty * ntx;
    const uint32_t x = (tx << 6) + lane;
#if DN_LDS
    if (staged) {
      for (uint32_t ly = row; ly < th; ly += DN_THREADS / 64u)
        for (uint32_t lx = lane; lx < tw; lx += 64u) {
          const int32_t gy = (int32_t)(ty * DN_TILE_H + ly) - R, gx = (int32_t)((tx << 6) + lx) - R;
          const bool ok = gy >= 0 && gy < (int32_t)H && gx >= 0 && gx < (int32_t)W;
          const uint32_t q = ok ? (uint32_t)gy * W + (uint32_t)gx : 0u;
          const uint2 g = A.ld_u2(tapg + 8u * q), v = A.ld_u2(src + 8u * q);
          s_tile[ly * tw + lx] = ok ? make_uint4(g.x, g.y, v.x, v.y) : make_uint4(RT_DN_NO_GEOM, 0u, 0u, 0u);
        }
      __syncthreads();
    }
#endif
    for (uint32_t s = 0; s < DN_TILE_H / (DN_THREADS / 64u); ++s) {
      const uint32_t y = sgpr(ty * DN_TILE_H + (DN_THREADS / 64u) * s + row);
      if (y >= H) break;  // (wave-uniform; the barriers stand outside this loop)
      const bool in = x < W;
      // (a lane right of the image works on the row's last pixel and stores nothing)
      const uint32_t cx = in ? x : W - 1u;
      const uint32_t pc = y * W + cx;
      const uint2 gp = A.ld_u2(tapg + 8u * pc), ip = A.ld_u2(src + 8u * pc);
      const bool geom = gp.x != RT_DN_NO_GEOM;
      uint2 out = ip;  // a pixel without geometry: its resolved word, carried through
      if (__ballot(geom) != 0) {
        const bool rows[5] = {(int32_t)y - 2 * st >= 0, (int32_t)y - st >= 0, true, y + st < H, y + 2 * st < H};
        auto gather = [&](int i, int j, uint2& gq, uint2& iq) {
          // (a tap off the image loads the centre's row or column instead: in bounds, weight 0)
          const bool vy = rows[j + 2];  // wave-uniform
          const int32_t qx = (int32_t)cx + st * i;
          const bool vx = qx >= 0 && qx < (int32_t)W;
          const uint32_t q = (uint32_t)((int32_t)y + (vy ? st * j : 0)) * W + (uint32_t)(vx ? qx : (int32_t)cx);
          gq = A.ld_u2(tapg + 8u * q);
          iq = A.ld_u2(src + 8u * q);
          return vy && vx;
        };
        uint2 f;
#if DN_LDS
        if (staged) {
          const uint32_t c0 = ((DN_THREADS / 64u) * s + row + (uint32_t)R) * tw + lane + (uint32_t)R;
          f = filter_pixel(gp, ip, zsh, ls, [&](int i, int j, uint2& gq, uint2& iq) {
            const uint4 e = s_tile[(int32_t)c0 + st * j * (int32_t)tw + st * i];
            gq = make_uint2(e.x, e.y);
            iq = make_uint2(e.z, e.w);
            return true;  // (outside the image: staged as a pixel without geometry)
          });
        } else
#endif
          f = filter_pixel(gp, ip, zsh, ls, gather);
        if (geom) {
          if (last) {
            const uint32_t a = A.ld_u32(base + 4u * pc);
            out.x = (a & 0xff000000u) | (rt_dn_remod(f.x & 0xffffu, (a >> 16) & 0xffu) << 16) |
                    (rt_dn_remod(f.x >> 16, (a >> 8) & 0xffu) << 8) | rt_dn_remod(f.y, a & 0xffu);
          } else {
            out = make_uint2(f.x, f.y | (ip.y & 0xffff0000u));
          }
        }
      }
      if (in) {
        if (last) A.st_u32(fb + 4u * pc, out.x);
        else st_u2(A, dst + 8u * pc, out);
      }
    }
#if DN_LDS
    if (staged) __syncthreads();  // the tile is read out before the next one is staged
#endif
  }
#endif
  return 0;
}
