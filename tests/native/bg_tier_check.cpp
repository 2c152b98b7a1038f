// Sweep of the background tier's split (skybox_rt_amd/csrc/runtime/bg_tier.h):
// a stand-alone program, no GPU.  For chunk counts 1..600, every heavy-tile
// count 0..tiles, grids from 1 up to the chunk count (every grid for the
// small frames, a spread of them including the lane grid and both ends for
// the large ones), 1 / 2 / 4 waves per workgroup and several rho:
//   * every chunk is dealt to exactly one wave;
//   * geometry chunks go to workgroups < tg only, background chunks to the rest;
//   * a tiered launch has no empty tier and no geometry wave without a chunk;
//   * tag 0 comes back exactly when the frame must stay untiered.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "bg_tier.h"

static long failures = 0, cases = 0, tiered_cases = 0;

#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (failures < 20) {                       \
        std::printf("FAIL %s: ", #cond);         \
        std::printf(__VA_ARGS__);                \
        std::printf("\n");                       \
      }                                          \
      ++failures;                                \
    }                                            \
  } while (0)

static void check_deal(uint32_t tg, uint32_t chunks, uint32_t heavy, uint32_t grid, uint32_t waves) {
  static std::vector<uint8_t> seen;
  seen.assign(chunks, 0);
  const uint32_t first = vxtier::first_bg_chunk(chunks, heavy);
  bool geo_any = false, bg_any = false, idle_geo = false;
  for (uint32_t b = 0; b < grid; ++b)
    for (uint32_t w = 0; w < waves; ++w) {
      const vxtier::Range r = vxtier::wave_range(tg, chunks, first, grid, waves, b, w);
      CHECK(r.stride > 0, "stride 0 (tg %u grid %u)", tg, grid);
      if (r.stride == 0) return;
      bool any = false;
      for (uint32_t c = r.first; c < r.end; c += r.stride) {
        CHECK(c < chunks, "chunk %u of %u", c, chunks);
        if (c >= chunks) return;
        ++seen[c];
        any = true;
        if (tg != 0) {
          const bool geo = c < first;
          CHECK(geo == (b < tg), "chunk %u (first bg %u) dealt to workgroup %u, tg %u", c, first, b, tg);
          (geo ? geo_any : bg_any) = true;
        }
      }
      if (tg != 0 && b < tg && !any) idle_geo = true;
    }
  for (uint32_t c = 0; c < chunks; ++c)
    CHECK(seen[c] == 1, "chunk %u dealt %u times (chunks %u heavy %u grid %u waves %u tg %u)", c, seen[c], chunks,
          heavy, grid, waves, tg);
  if (tg != 0) {
    CHECK(tg < grid, "no background workgroup: tg %u grid %u", tg, grid);
    CHECK(geo_any && bg_any, "an empty tier (chunks %u heavy %u grid %u waves %u tg %u)", chunks, heavy, grid, waves,
          tg);
    CHECK(!idle_geo, "a geometry wave without a chunk (chunks %u heavy %u grid %u waves %u tg %u)", chunks, heavy,
          grid, waves, tg);
  }
}

int main() {
  const double rhos[] = {0.001, 1.0, 3.0, 1000.0};
  const uint32_t wvs[] = {1, 2, 4};
  for (uint32_t chunks = 1; chunks <= 600; ++chunks) {
    const uint32_t tiles = (chunks + 15) / 16;
    for (uint32_t waves : wvs) {
      std::set<uint32_t> grids;
      if (chunks <= 48) {
        for (uint32_t g = 1; g <= chunks; ++g) grids.insert(g);
      } else {
        for (uint32_t g = 1; g <= chunks; g = g < 4 ? g + 1 : g * 3 + 1) grids.insert(g);
        grids.insert((chunks + 2 * waves - 1) / (2 * waves));  // the lane grid
        grids.insert((chunks + 3 * waves - 1) / (3 * waves));
        grids.insert(chunks - 1);
        grids.insert(chunks);
      }
      for (uint32_t heavy = 0; heavy <= tiles; ++heavy)
        for (uint32_t grid : grids) {
          uint32_t tgs[8] = {0u};  // (the untiered deal of the same launch first)
          uint32_t ntg = 1;
          for (double rho : rhos) {
            const uint32_t tg = vxtier::tier_groups(vxtier::Config{}, chunks, heavy, grid, waves, rho);
            ++cases;
            // untiered exactly when a tier would be empty or the grid cannot hold both
            const uint32_t G = vxtier::first_bg_chunk(chunks, heavy);
            const bool must_untier = heavy == 0 || G == chunks || grid < 2 || G < waves;
            CHECK((tg == 0) == must_untier, "chunks %u heavy %u grid %u waves %u rho %g: tg %u", chunks, heavy, grid,
                  waves, rho, tg);
            bool known = false;
            for (uint32_t i = 0; i < ntg; ++i) known = known || tgs[i] == tg;
            if (!known) tgs[ntg++] = tg;
          }
          for (uint32_t i = 0; i < ntg; ++i) {
            if (tgs[i]) ++tiered_cases;
            check_deal(tgs[i], chunks, heavy, grid, waves);
          }
        }
    }
  }
  // more geometry cost never takes workgroups from the geometry tier
  for (uint32_t heavy = 1; heavy < 64; ++heavy) {
    uint32_t last = 0;
    for (double rho : rhos) {
      const uint32_t tg = vxtier::tier_groups(vxtier::Config{}, 1024, heavy, 256, 2, rho);
      CHECK(tg >= last, "rho %g: tg %u < %u", rho, tg, last);
      last = tg;
    }
  }
  // the configurations that are never tiered
  {
    vxtier::Config c;
    auto tg = [&](const vxtier::Config& k) { return vxtier::tier_groups(k, 1024, 10, 256, 2, 3.0); };
    CHECK(tg(c) != 0, "the eligible frame is tiered");
    vxtier::Config k = c; k.block_lists = false; CHECK(tg(k) == 0, "no block lists");
    k = c; k.chunk_table = false; CHECK(tg(k) == 0, "no chunk table");
    k = c; k.cdesc_first = 32; CHECK(tg(k) == 0, "cdesc_first != 0");
    k = c; k.compact = true; CHECK(tg(k) == 0, "compact");
    k = c; k.sharded = true; CHECK(tg(k) == 0, "sharded");
    k = c; k.path = true; CHECK(tg(k) == 0, "path");
    CHECK(vxtier::tier_groups(c, 1024, 0, 256, 2, 3.0) == 0, "heavy 0");
    CHECK(vxtier::tier_groups(c, 1024, 64, 256, 2, 3.0) == 0, "every tile heavy");
    // the flagship frame: 16 384 chunks, 194 heavy tiles, grid 4 096, 2 waves
    const uint32_t f = vxtier::tier_groups(c, 16384, 194, 4096, 2, 3.0);
    CHECK(f > 0 && f * 2 <= 194 * 16 && f < 4096, "flagship split %u", f);
  }
  std::printf("%ld cases, %ld tiered deals checked, %ld failure(s)\n", cases, tiered_cases, failures);
  return failures ? 1 : 0;
}
