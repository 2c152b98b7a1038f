// fused_chunk.h -- whether a configuration's frames carry RT_FLAG_FUSED (kernels/rt_common.h): image
// rt_kernel then traces a wave's last geometry chunk's shadow rays in place (kernels/rt_kernel.hip
// fused_chunk).  The host only sets the bit; what a frame needs besides it -- lists
// that hold for its light, the wave's last chunk, a winner in the wave -- the kernel sees for itself,
// wave by wave, so a frame behind a moved light (RT_LW_NO_SLIST) takes the queue and the drain with the
// bit set.  Header-only, no dependency on the app: tests/native/fused_chunk_check.cpp builds it alone.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace rtfused {

// env RT_FUSED_CHUNK, read at configure like the other frame knobs: unset, empty or any number but 0: on
inline bool knob(const char* env) { return !(env && *env && std::atoi(env) == 0); }

struct Conf {
  bool shadows;  // RT_RENDER_SHADOWS
  bool path, flat, raster;  // RT_RENDER_PATH / _FLAT / _RASTER: other kernels
  bool tail;  // a scene with an ordered tail: image rt_om
};

// the bit for rt_kernel_arg_t.flags (bit: RT_FLAG_FUSED), or 0.  Only the one-light primary+shadow
// frame has the path; the images that configuration may also run (rt_kernel_stats, rt_lights, rt_bvh,
// the deep ones) are built without it and ignore the bit.
inline uint32_t flag(const Conf& c, const char* env, uint32_t bit) {
  if (!knob(env)) return 0u;
  if (!c.shadows || c.path || c.flat || c.raster || c.tail) return 0u;
  return bit;
}

}  // namespace rtfused
