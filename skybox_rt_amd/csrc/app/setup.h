// setup.h -- host-side scene preparation for the RT kernel.
//
//  * PrimSetup: the per-primitive part of graphics::Binning
//    (sim/common/gfxutil.cpp:131-251): clip -> 2D-homogeneous device
//    coordinates, edge equations, half-pixel offset, Q15.16 edges, Q7.24
//    attribute deltas -> rt_prim_t (the fixed-point shading record).
//  * DrawcallState: the draw3d host state setup (draw3d/main.cpp:286-344)
//    reduced to what shading needs -> rt_dcstate_t.
//  * cocogfx CGLTrace enum mapping (inferred; pinned by the golden images
//    through the oracle, see oracle/gfx.h).
#pragma once

#include <cstdint>
#include <vector>

#include "VX_types.h"
#include "../kernels/rt_common.h"
#include "cgltrace.h"

namespace rt {

// CGLTrace -> VX enum mapping (gfxutil.cpp:280-346 case order)
uint32_t ToVXCompare(int32_t cgl_compare);
int32_t ToVXFormat(int32_t cgl_format);
uint32_t FormatStride(int32_t vx_format);

constexpr int32_t kCglFilterNearest = 1;
constexpr int32_t kCglAddressWrap = 0;
constexpr int32_t kCglEnvModeModulate = 3;

enum SetupStatus { kSetupOk = 0, kSetupDegenerate = 1, kSetupCulled = 2 };

// Fills `out` (edges/attribs) for one triangle at width x height.
int PrimSetup(const std::array<Vertex, 3>& v, uint32_t width, uint32_t height, float znear,
              float zfar, rt_prim_t* out);

// Shading state of a drawcall (texture address filled by the caller).
rt_dcstate_t DrawcallState(const DrawCall& dc, const Scene& scene);

// Screen bounding box of a triangle at width x height (gfxutil.cpp:168-192);
// returns kSetupCulled (and an empty box) when it misses the viewport.
int PrimBBox(const std::array<Vertex, 3>& v, uint32_t width, uint32_t height, rt_bbox_t* out);

// Output-merger state of a drawcall (raster pipeline).
rt_omstate_t OmState(const DrawCall& dc);

// The chunk descriptor table of the whole-block tier (rt_common.h
// rt_cdesc_t; kernels/rt_setup.hip phase_cdesc builds it on the device):
// record i is work-order position pos0 + i / 16, block i % 16.  `order`
// (null: identity) and `bidx` (first, count per local block; null: no lists
// in use, every header (0, 0)) as the setup left them.
std::vector<rt_cdesc_t> ChunkDescs(uint32_t width, uint32_t tiles_x, uint32_t shard_index,
                                   uint32_t shard_count, bool compact, uint32_t pos0,
                                   uint32_t local_tiles, const uint32_t* order, const uint32_t* bidx);

// The background-layer table (rt_common.h rt_bglayer_t) restated on the host (kernels/rt_setup.hip
// phase_bglayer builds it on the device): record i is chunk first_chunk + i of an unsharded frame's
// whole-block chunks (work-order position c / 16, block c % 16), up to local_tiles * 16.  The
// block's pixels are painted with the layer records in drawing order (`layers` is last drawn
// first, as vlayers; each covering layer overwrites), then compared.  `prims`: rt_prim_t by pid.
std::vector<rt_bglayer_t> BgLayers(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t local_tiles,
                                   const uint32_t* order, uint32_t first_chunk, const rt_vtri_t* layers,
                                   uint32_t num_layers, const rt_prim_t* prims, uint32_t num_prims);

// The block lists trimmed to their winners (kernels/setup_common.h rt_btrim_arg_t;
// kernels/rt_btrim_kernel.hip builds them on the device), restated on the host: for every local
// 8x8 block of the shard, each of its pixels inside the image is resolved over the block's whole
// list by the frames' per-pixel test (rt_trace.h vis_test: covered rectangle, the three edge
// values, the shader's depth word, vis_better under the scene's tie rule), and the entries whose
// primitive wins a pixel are compacted to the front of the list's slots, unchanged and in order.
// `bidx` (first, count per local block), `blist` (entries + RT_BLIST_PAD) and `vgeom` as the setup
// left them.  *btrim: blist's copy with the kept entries moved up; *btidx: (bidx's first, the kept
// count) per block; *kept / *blocks: the kept entries in total, the blocks that keep any.
void TrimBlockLists(uint32_t width, uint32_t height, uint32_t tiles_x, uint32_t shard_index,
                    uint32_t shard_count, uint32_t local_tiles, bool tie_high, const uint32_t* bidx,
                    const rt_bentry_t* blist, uint64_t entries, const rt_vtri_t* vgeom,
                    std::vector<uint32_t>* btidx, std::vector<rt_bentry_t>* btrim, uint64_t* kept,
                    uint32_t* blocks);

}  // namespace rt
