// bg_tier.h -- how a primary + shadow frame's workgroups are split between the
// geometry and the background tier (kernels/rt_kernel.hip RT_BG_TIER,
// DESIGN.md 4.1 r12).
//
// The frame's chunks (64 pixel tasks each) stand in work order, heaviest 32x32
// tile first, 16 chunks a tile.  `heavy` tiles have weight > 0, so the chunks
// from first = 16 * heavy on have empty block lists (the background).  A
// tiered launch keeps its grid and deals it in two:
//   * workgroups [0, tg): the geometry tier.  Its tg * waves waves share the
//     chunks [0, first): wave w takes w, w + tg * waves, ...
//   * workgroups [tg, grid): the background tier.  Its (grid - tg) * waves
//     waves share the chunks [first, chunks) the same way.
// tg travels in the launch's tag; 0 means untiered -- wave w of the grid's
// waves takes chunks w, w + grid * waves, ... of them all.
//
// The split gives the tiers waves in proportion to G * rho : B (G, B the
// tiers' chunks, rho the cost of a geometry chunk in background chunks), with
// at least one workgroup each and no geometry wave without a chunk
// (tg * waves <= G).
//
// Host-only, no HIP types: a plain C++ program can sweep it
// (tests/test_bg_tier_cpu.py).  wave_range() restates the kernel's deal.
#ifndef VX_RUNTIME_BG_TIER_H
#define VX_RUNTIME_BG_TIER_H

#include <cstdint>

namespace vxtier {

constexpr uint32_t kChunksPerTile = 16;
// rho when env RT_BG_COST does not say: measured
constexpr double kDefaultCost = 3.0;

// what keeps a frame untiered whatever its tiles are
struct Config {
  bool block_lists = true;   // the configuration renders from per-block candidate lists
  bool chunk_table = true;   // and has the chunk descriptor table ...
  uint32_t cdesc_first = 0;  // ... which covers every chunk (no split / quad tier in front)
  bool compact = false, sharded = false, path = false;
};

inline bool eligible(const Config& c) {
  return c.block_lists && c.chunk_table && c.cdesc_first == 0 && !c.compact && !c.sharded && !c.path;
}

// the first background chunk of a frame of `chunks` chunks
inline uint32_t first_bg_chunk(uint32_t chunks, uint32_t heavy) {
  const uint64_t f = (uint64_t)heavy * kChunksPerTile;
  return f < chunks ? (uint32_t)f : chunks;
}

// The geometry tier's workgroups (the launch tag) of a launch of `grid`
// workgroups of `waves` waves; 0: untiered.  Untiered when the configuration
// is not eligible, when a tier would have no chunk (heavy 0, or every tile
// heavy), when the grid cannot hold a workgroup of each (grid < 2) and when
// a workgroup has more waves than the geometry tier has chunks.
inline uint32_t tier_groups(const Config& c, uint32_t chunks, uint32_t heavy, uint32_t grid,
                            uint32_t waves, double rho) {
  if (!eligible(c) || grid < 2 || waves == 0) return 0;
  const uint32_t G = first_bg_chunk(chunks, heavy);
  const uint32_t B = chunks - G;
  if (G == 0 || B == 0 || G < waves) return 0;
  if (!(rho > 0.0)) rho = 1.0;
  const double g = (double)G * rho;
  uint64_t tg = (uint64_t)((double)grid * g / (g + (double)B) + 0.5);
  if (tg > G / waves) tg = G / waves;  // no geometry wave without a chunk
  if (tg > grid - 1) tg = grid - 1;    // a workgroup for the background
  if (tg < 1) tg = 1;
  return (uint32_t)tg;
}

// The chunks of wave `wave` of workgroup `block`: first, first + stride, ...
// below end (the kernel's deal, restated).
struct Range {
  uint32_t first, end, stride;
};
inline Range wave_range(uint32_t tg, uint32_t chunks, uint32_t first_bg, uint32_t grid, uint32_t waves,
                        uint32_t block, uint32_t wave) {
  if (tg == 0) return {block * waves + wave, chunks, grid * waves};
  if (block < tg) return {block * waves + wave, first_bg < chunks ? first_bg : chunks, tg * waves};
  return {first_bg + (block - tg) * waves + wave, chunks, (grid - tg) * waves};
}

}  // namespace vxtier

#endif
