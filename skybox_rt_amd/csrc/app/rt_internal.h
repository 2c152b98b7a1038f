// rt_internal.h -- the RT host app's scene / renderer state (librtapp.so
// internals shared by rt_app.cpp and device_setup.cpp; not part of the ABI).
#pragma once

#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "app_util.h"
#include "bvh.h"
#include "cgltrace.h"
#include "frame_image.h"
#include "rt_common.h"
#include "vortex.h"
#include "vortex_hip.h"
#include "vx_rt.h"

struct rt_scene {
  rt::Scene scene;
  rt::Bvh bvh;                    // the host build: on request only (host_bvh)
  std::vector<rt::BuildTri> build_tris;  // its input: the depth-tested triangles, clip (x, y, w)
  bool bvh_built = false;
  std::vector<int32_t> geometry;  // depth-tested prims (BVH input), ascending
  std::vector<int32_t> layers;    // screen-layer prims, descending pid
  std::string unsupported;        // non-empty: the RT path cannot render it
  bool tie_high = false;
  // RT_SCENE_OM_LAYERS: the ordered tail -- the first drawcall the RT path
  // cannot trace and every drawcall after it; geometry / layers / build_tris /
  // tie_high then describe the drawcalls before it (the traced head) only
  uint32_t first_tail_dc = 0;       // = the drawcall count when there is no tail
  std::vector<int32_t> tail_prims;  // the tail's prims in submission order (ascending, consecutive)
  double parse_ms = 0, bvh_ms = 0;
};

// a device buffer of the setup that persists across configurations and only
// grows (device_setup.cpp ensure)
struct DevScratch {
  vx_buffer_h h = nullptr;
  uint64_t addr = 0;
};
// the device setup's argument block, status words and scratch arrays
struct SetupScratch {
  DevScratch args, status, parent, count, weight, hist, bcnt, bpart, btmp;
  DevScratch scnt, spart, sproj, soff, skey, stmp;
  DevScratch sah, sah_args;  // the SAH build's arrays (one buffer) and argument block
  uint64_t bcap = 0;   // block-list entry capacity of btmp / blist
  uint32_t scap = 0;   // shadow-list entry capacity of stmp / slist
  uint64_t sah_bytes = 0;
  void release() {
    for (DevScratch* d : {&args, &status, &parent, &count, &weight, &hist, &bcnt, &bpart, &btmp, &scnt, &spart,
                          &sproj, &soff, &skey, &stmp, &sah, &sah_args})
      if (d->h) {
        vx_mem_free(d->h);
        d->h = nullptr;
      }
  }
};

// One set of light-space shadow lists (device_setup.cpp slist_args .. settle_lists work on a
// set): the index and entry buffers, the entry capacity, the light they were built for and
// what became of them.  Set 0 is the renderer's own state (sidx / slist, su.scap, sl_*: the
// single light of every path before rt_renderer_set_lights), named through this view; the sets
// of a several-light frame are LightSet::own.
struct ListSet {
  vx_buffer_h *sidx, *slist;
  uint64_t *sidx_addr, *slist_addr;
  uint32_t* cap;       // entry capacity of slist (and of the chain's stmp scratch while it builds)
  float* light;        // the light the lists were built for
  bool *built, *rejected;
  uint64_t* entries;
};
// a light of rt_renderer_set_lights with the storage of its set
struct LightSet {
  vx_buffer_h sidx = nullptr, slist = nullptr;
  uint64_t sidx_addr = 0, slist_addr = 0;
  uint32_t cap = 0;
  float light[3] = {0, 0, 0};
  bool built = false, rejected = false;
  uint64_t entries = 0;
  ListSet set() { return ListSet{&sidx, &slist, &sidx_addr, &slist_addr, &cap, light, &built, &rejected, &entries}; }
};

struct rt_renderer {
  rt_scene* sc = nullptr;
  vx_device_h dev = nullptr;
  // the kernel images (frame_image.h), uploaded a group at a time by rtapp::load_images: the
  // modes' at creation, the deep ones (then in place of the regular rt / pt ones) when a tree
  // needs them, the others by the first call that runs them
  vx_buffer_h img[rtimg::IMG_COUNT] = {};
  void free_image(int i) {
    if (img[i]) vx_mem_free(img[i]);
    img[i] = nullptr;
  }
  // several lights (vx_rt.h rt_renderer_set_lights, rt_renderer_set_path_lights): the lights'
  // list sets (kept across calls: their buffers only grow) and the number in use -- 0: one
  // light, the renderer's own state, every path as before
  std::vector<LightSet> lsets;
  uint32_t nlights = 0;
  ListSet set0() {
    return ListSet{&sidx, &slist, &arg.sidx_addr, &arg.slist_addr, &su.scap, sl_light, &sl_built, &sl_rejected,
                   &sl_entries};
  }
  // scenes with an ordered tail (rt_om, plain and shadow frames): the per-block tail lists
  // and the tail's rt_vtri_t records (host-built per configure)
  vx_buffer_h oidx = nullptr, olist = nullptr, ovtris = nullptr;
  uint64_t olist_entries = 0;
  vx_buffer_h pathq = nullptr, pathq_ctr = nullptr;
  bool pq = false;          // the configuration runs the two-kernel path tracer
  // progressive accumulation (vx_rt.h rt_renderer_accum_begin): the record buffer (rt_common.h
  // rt_accum_arg_t: 16 B per framebuffer pixel) of the current configuration, named in the
  // argument buffer behind rt_kernel_arg_t
  vx_buffer_h accum = nullptr;
  uint64_t accum_bytes = 0;
  bool accum_on = false;     // between accum_begin and the next configure
  bool accum_reset = false;  // the next accumulation launch carries RT_LW_ACCUM_RESET
  uint32_t accum_n = 0;      // samples queued since the last reset: the records' n once they ran
  // visibility records (vx_rt.h rt_render_aov_start): the rt_aov image, loaded by the first call
  // that runs it and kept for the renderer's life -- not an image a frame runs, so not in img[]
  // -- and the record buffer of the current configuration (rt_common.h rt_aov_arg_t: 16 B per
  // framebuffer pixel), named in the argument buffer behind the light table
  vx_buffer_h aov_img = nullptr, aov = nullptr;
  uint64_t aov_bytes = 0;
  // relighting (vx_rt.h rt_relight_capture_start / rt_render_relight_start): the rt_aov_base and
  // rt_relight images, loaded and kept the same way, and the base-colour buffer of the current
  // configuration (rt_common.h rt_relight_arg_t: 4 B per framebuffer pixel) beside the records.
  // relight_n: the lights in use at the last capture, 0 while the records and base colours
  // describe no lights in use -- before a capture, and after a configure or any call that
  // changes the lights
  vx_buffer_h aov_base_img = nullptr, relight_img = nullptr, relight_base = nullptr;
  uint64_t relight_base_bytes = 0;
  uint32_t relight_n = 0;
  // denoising (vx_rt.h rt_denoise_capture_start / rt_render_denoise_start): the rt_aov_guide,
  // rt_denoise_prep and rt_denoise_pass images, loaded and kept the same way, and one buffer of the
  // current configuration holding, per framebuffer pixel, the guide record (16 B), the tap guide
  // (8 B), the two irradiance buffers (8 B each) and the base colour (4 B), in that order
  // (rt_common.h rt_denoise_arg_t names each part).  dn_captured: a capture was queued since the
  // last configure
  vx_buffer_h dn_guide_img = nullptr, dn_prep_img = nullptr, dn_pass_img = nullptr, dn_buf = nullptr;
  uint64_t dn_bytes = 0;
  bool dn_captured = false;
  // ambient occlusion (vx_rt.h rt_renderer_ao_begin / rt_render_ao_start / rt_render_ao_resolve_start):
  // the rt_ao and rt_ao_resolve images, loaded and kept the same way, and the count buffer of the
  // current configuration (rt_common.h rt_ao_arg_t: 4 B per framebuffer pixel)
  vx_buffer_h ao_img = nullptr, ao_resolve_img = nullptr, ao_buf = nullptr;
  uint64_t ao_bytes = 0;
  bool aov_launched = false;  // a record launch was queued since the last configure
  bool ao_on = false;         // between ao_begin and the next configure
  bool ao_reset = false;      // the next tracing launch carries RT_AO_LW_RESET
  uint32_t ao_n = 0;          // samples queued since the last reset: the counts' N once they ran
  rt_ao_params_t ao_params{};
  // soft shadows (vx_rt.h rt_renderer_soft_begin / rt_render_soft_start / rt_render_soft_resolve_start):
  // the rt_soft and rt_soft_resolve images, loaded and kept the same way, and the count planes of the
  // session (rt_common.h rt_soft_arg_t: 2 B per light in use and framebuffer pixel)
  vx_buffer_h soft_img = nullptr, soft_resolve_img = nullptr, soft_buf = nullptr;
  uint64_t soft_bytes = 0;
  bool soft_on = false;        // between soft_begin and the next configure or change of lights
  bool soft_reset = false;     // the next tracing launch carries RT_SOFT_LW_RESET
  uint32_t soft_n = 0;         // samples queued since the last reset: the counts' N once they ran
  uint32_t soft_lights = 0;    // the session's lights
  uint32_t soft_seed = 0;
  // caller-supplied rays (vx_rt.h rt_query_reserve / rt_query_trace_start / rt_query_keys_start): the
  // rt_query and rt_query_keys images, loaded and kept the same way, and the one buffer of the reserve
  // (rt_common.h rt_query_arg_t: rays, hits, skip words, permutation and keys, 52 B per ray) -- kept
  // across configures, with its argument area
  vx_buffer_h q_img = nullptr, q_keys_img = nullptr, q_buf = nullptr;
  uint64_t q_cap = 0;        // rays reserved; 0: no reserve
  bool q_pending = false;    // a query launch was started and no wait has returned since
  float q_box[6] = {0, 0, 0, 0, 0, 0};  // the key grid's box: the geometry corners' bounds
  vx_buffer_h nodes = nullptr, nodes4 = nullptr, tris = nullptr, layers = nullptr, dcs = nullptr, tex = nullptr;
  vx_buffer_h ptris = nullptr, geom = nullptr, oms = nullptr, bbox = nullptr, zbuf = nullptr;
  vx_buffer_h order = nullptr;
  vx_buffer_h vnodes = nullptr, vtris = nullptr, vlayers = nullptr, vgeom = nullptr;
  vx_buffer_h blist = nullptr, bidx = nullptr;  // per-block candidate lists (rt_bentry_t)
  // the block lists trimmed to their winners (setup_common.h rt_btrim_arg_t; device_setup.cpp block_trim,
  // rt_app.cpp host_block_trim): btrim / btidx beside blist / bidx, which stay the untrimmed lists;
  // while trim_on the render arguments' list and header addresses are btrim's and btidx's.  The
  // rt_btrim image is loaded at creation and kept (not an image a frame runs, so not in img[]);
  // btrim_args: its argument buffer, whose last words count the kept entries and blocks
  vx_buffer_h btrim = nullptr, btidx = nullptr, btrim_img = nullptr, btrim_args = nullptr;
  bool trim_on = false;
  bool trim_counted = false;     // setup.btrim_entries / btrim_blocks hold this configuration's counts
  vx_buffer_h cdesc = nullptr;   // chunk descriptor table (rt_cdesc_t, device_setup.cpp chunk_desc)
  uint32_t cdesc_n = 0;          // its records (0: none in this configuration)
  vx_buffer_h bglayer = nullptr; // background-layer table (rt_bglayer_t, device_setup.cpp bg_layers)
  uint32_t bglayer_n = 0;        // its records (0: none: untiered, or env RT_BG_LAYERS=0)
  vx_buffer_h sidx = nullptr, slist = nullptr;  // light-space shadow lists (built for sl_light)
  bool sl_mode = false;     // this configuration's shadow rays use the light-space lists
  bool sl_pending = false;  // lists queued by rt_renderer_set_light, status not read yet
  // the moving light (rt_renderer_set_list_policy): after a light change the
  // frames trace their shadow rays by the BVH packet walk (slist_on = 0, no
  // wait for lists) until the light has stayed for sl_defer frames; then the
  // lists are queued before the next frame.  0: set_light queues them at once
  uint32_t sl_defer = 8;
  bool sl_stale = false;    // the light moved since the lists were built; lists not queued yet
  uint32_t sl_static = 0;   // frames started since that light change
  SetupScratch su;
  vx_hip_copy_to_dev_async_t copy_async = nullptr;
  vx_hip_set_launch_tag_t set_tag = nullptr;
  vx_hip_set_launch_words_t set_words = nullptr;  // a frame's light + flags (RT_LW_*)
  vx_hip_host_mem_t host_mem = nullptr;
  volatile uint32_t* stat_host = nullptr;  // pinned status words (+ nonce) of the setup sequences
  uint64_t stat_dev = 0;
  uint32_t stat_nonce = 0;
  uint32_t stat_pending = 0;  // nonce of the last sequence issued with the pinned status copy (0: none)
  float sl_light[3] = {0, 0, 0};
  uint32_t sl_n = 0;        // the cube-map resolution they were built at
  bool sl_built = false;
  bool sl_rejected = false;  // built for sl_light / sl_n and too large (block_lists_fit)
  uint64_t sl_entries = 0;
  vx_buffer_h gather_recv = nullptr, gather_image = nullptr;  // rank 0 of rt_render_gather
  vx_buffer_h prims = nullptr, cbuf = nullptr, args = nullptr;
  // device-side setup (device_setup.cpp, kernels/rt_setup.hip): the
  // resolution-independent inputs uploaded once at creation, and the
  // per-primitive visibility records of the current configuration
  vx_buffer_h verts = nullptr, pdc = nullptr, dcz = nullptr;
  vx_buffer_h layer_list = nullptr, geometry_list = nullptr, vis = nullptr;
  uint64_t cbuf_bytes = 0;
  // frame overlap (vx_rt.h rt_render_start): while `lanes` is set, frame n
  // renders into framebuffer n mod 2 (cbuf, cbuf1) on the driver's launch
  // lane n mod 2, so frames sharing a buffer share a lane and stay ordered.
  // cur_buf: the buffer of the last started frame (-1: none since the
  // configure); prev_buf: of the frame before it (-1: none, or one buffer)
  vx_buffer_h cbuf1 = nullptr;
  uint64_t cbuf1_bytes = 0;
  uint32_t cbuf1_off = 0;   // cbuf1's arena offset minus cbuf's, mod 2^32 (RT_LW_CBUF_MASK bits)
  bool lanes = false;
  int cur_buf = -1, prev_buf = -1;
  // setup launches were queued since the last frame (queue_lists): the next
  // frame runs behind them as an ordinary launch -- with a rebuild before
  // every frame nothing could overlap, and a lane per frame would only buy
  // a cross-lane event each way
  bool lane_break = false;
  vx_hip_set_launch_lane_t set_lane = nullptr;
  // the grid, in workgroups, of a frame that goes to a launch lane (0: the image's grid):
  // overlapped frames keep the chip full, so their waves take two chunks each and half as
  // many waves pay the per-wave prologue and exit; a frame rendered alone keeps a wave per
  // chunk on the image's grid
  // (worked out from the image's workgroup size by the first frame that needs it, or by
  // rt_renderer_setup_stats: asking the driver loads the image, which a configure must not pay)
  uint32_t lane_grid = 0;
  uint32_t lane_chunks = 0;  // chunks per wave of such a frame; 0: the configuration has no lane grid
  bool lane_grid_known = false;
  vx_hip_set_launch_grid_t set_grid = nullptr;
  vx_hip_image_launch_shape_t launch_shape = nullptr;
  // the background tier (runtime/bg_tier.h): a frame of an eligible
  // configuration carries the number of its geometry-tier workgroups as its launch tag
  // (rt_kernel deals the workgroups behind them the chunks from bg_first on, which it renders
  // by a lean body); the grid stays the frame's
  uint32_t bg_mode = 0;      // env RT_BG_TIER: 0 never, 1 frames on a launch lane, 2 every frame
  bool bg_stale = false;     // env RT_BG_STALE=1: also frames whose light-space lists are stale
  double bg_cost = 0.0;      // env RT_BG_COST: a geometry chunk's cost in background chunks
  bool bg_ok = false;        // this configuration may be tiered
  uint32_t bg_first = 0;     // its first background chunk (16 * heavy tiles)
  uint32_t img_block[2] = {0, 0}, img_grid[2] = {0, 0};  // rt_kernel / rt_kernel_stats' launch shape
  bool img_shape_known[2] = {false, false};
  rt_render_params_t params{};
  rt_kernel_arg_t arg{};
  bool configured = false;
  uint32_t local_tiles = 0;
  vx_hip_mem_ptr_t mem_ptr = nullptr;
  vx_hip_stream_t stream = nullptr;
  vx_hip_last_run_t last_run = nullptr;
  vx_hip_mpm_rows_t mpm_rows = nullptr;
  vx_hip_run_totals_t run_totals = nullptr;
  vx_hip_set_counters_t set_counters = nullptr;
  vx_hip_launch_group_t launch_group = nullptr;
  vx_hip_set_timing_t set_timing = nullptr;
  std::string kdir;         // kernel directory (images missing there come from lib_dir)
  bool deep = false;        // generic RT/PT images (every BVH layout, 32-entry stack)
  // the configured tree runs the generic images: not the binary16 BVH4 the others walk
  bool generic_tree() const { return rtimg::generic_tree(deep, (arg.flags & RT_FLAG_BVH4H) != 0); }
  // the primary rays' tree of the current configuration (rt_renderer_export_vis_tree;
  // host setup only -- after a device setup it is read back on request)
  std::vector<std::array<int32_t, 4>> vis_refs;
  std::vector<int32_t> vis_pids;
  bool use_bvh4 = true;     // the configured traversal reads the BVH4
  bool gpu_bvh = false;     // nodes/tris were built on the device (rt_renderer_build_bvh)
  bool gpu_bvh4 = false;    // ... and collapsed to a BVH4 there whose stack fits the images
  uint32_t num_tris = 0;    // leaf triangle records (without the 3 padding records)
  rt_setup_stats_t setup{};  // the last configuration's setup (rt_renderer_setup_stats)
  rt_bvh_build_stats_t bvh_stats{};  // how the current tree was built (rt_renderer_bvh_stats)

  ~rt_renderer() {
    for (int i = 0; i < rtimg::IMG_COUNT; ++i) free_image(i);
    vx_buffer_h* bufs[] = {&nodes, &nodes4, &tris, &layers, &dcs, &tex, &ptris, &geom, &oms, &bbox, &zbuf,
                           &order, &vnodes, &vtris, &vlayers, &vgeom, &gather_recv, &gather_image, &prims,
                           &cbuf, &cbuf1, &args, &verts, &pdc, &dcz, &layer_list, &geometry_list, &vis,
                           &blist, &bidx, &btrim, &btidx, &btrim_img, &btrim_args, &cdesc, &bglayer, &sidx, &slist, &pathq, &pathq_ctr, &oidx, &olist, &ovtris,
                           &accum, &aov, &aov_img, &relight_base, &aov_base_img, &relight_img,
                           &dn_guide_img, &dn_prep_img, &dn_pass_img, &dn_buf, &ao_img, &ao_resolve_img, &ao_buf, &soft_img, &soft_resolve_img, &soft_buf,
                           &q_img, &q_keys_img, &q_buf};
    for (auto* b : bufs) {
      if (*b) vx_mem_free(*b);
      *b = nullptr;
    }
    for (LightSet& l : lsets)
      for (vx_buffer_h* b : {&l.sidx, &l.slist})
        if (*b) {
          vx_mem_free(*b);
          *b = nullptr;
        }
    su.release();
    if (dev) vx_dev_close(dev);
  }
};

namespace rtapp {

// the scene's host BVH (app/bvh.cpp), built on first use: the renderer
// builds its tree on the device (bvh_sah.hip) unless env RT_BVH=host
int host_bvh(rt_scene* s);

// (re)allocate *buf (size bytes, or 64 when 0), copy `data` when given; the
// device address must lie below 4 GiB (the kernels' 32-bit arena offsets)
int upload(vx_device_h dev, const void* data, uint64_t size, vx_buffer_h* buf, uint64_t* addr);
// the images of `group` (frame_image.h) that are not loaded yet, by their source rules; -2 and
// a message "`who`: no <file> next to <anchor>" when one is not next to its anchor, -1 (and
// none of the group loaded) when an upload fails
int load_images(rt_renderer* r, rtimg::Group group, const char* who = "");
// `size` bytes at `src` into buffer h at `offset`: in stream order behind the queued launches
// where the driver has the asynchronous copy, else vx_copy_to_dev; the copy's return code
inline int write_buf(rt_renderer* r, vx_buffer_h h, uint64_t offset, const void* src, uint64_t size) {
  return r->copy_async ? r->copy_async(h, src, offset, size) : vx_copy_to_dev(h, src, offset, size);
}
// the same into an area of the render argument buffer (rt_common.h RT_*_ARG_OFFSET)
inline int write_args(rt_renderer* r, uint64_t offset, const void* src, uint64_t size) {
  return write_buf(r, r->args, offset, src, size);
}

struct DevBuf {  // scratch buffer freed at scope exit
  vx_buffer_h h = nullptr;
  uint64_t addr = 0;
  ~DevBuf() {
    if (h) vx_mem_free(h);
  }
};

// device_setup.cpp: the resolution-independent inputs of the device setup
// and the triangle records built from them (ptris, geom) at renderer creation
int device_ingest(rt_renderer* r, bool records);
// the per-resolution records of rt_renderer_configure on the device: prims
// (+ bbox, zbuf clear for raster), vis / vtris / vlayers / vgeom / vnodes,
// the tile order (heavy = local tiles with weight > 0), the cleared cbuf.
// r->arg holds the layout fields (tiles, shard, flags, the tree); the
// record buffers grow as needed and their addresses are set in r->arg.
// lists: also the per-block candidate lists (rt_bentry_t, the bidx / blist
// buffers and arg.blist_blocks; 0 when they do not fit, block_lists_fit);
// slists: the light-space shadow lists for a.light unless current (kept
// while the light is unchanged; arg.slist_on 0 when they do not fit).  One
// stream-ordered launch sequence, one status read-back.
// the chunk descriptor table of the whole-block tier (rt_common.h
// rt_cdesc_t), one more launch of the setup image behind the configure's
// sequence; called once the tiers are known, when the block lists are in use
int chunk_desc(rt_renderer* r, uint32_t* launches);
// the block lists trimmed to their winners (kernels/rt_btrim_kernel.hip), one launch behind the
// configure's sequence and ahead of chunk_desc's: btrim / btidx built from blist / bidx, and the
// render arguments' list and header addresses pointed at them (r->trim_on).  Called when the
// lists are in use and final (after an overflow refill).
int block_trim(rt_renderer* r, uint32_t* launches);
// the background-layer table (rt_common.h rt_bglayer_t) of the chunks from `first` on, one more
// launch behind chunk_desc's once the heavy tiles are known; *addr 0 and no records when the
// configuration has no chunk table over every chunk
int bg_layers(rt_renderer* r, uint32_t first, uint64_t* addr, uint32_t* launches);
int device_setup(rt_renderer* r, bool raster, bool order_on, bool lists, bool slists, uint32_t* heavy,
                 uint32_t* launches);
// rt_renderer_set_light: the new light into the render arguments and, when
// the configuration uses them, its shadow lists -- all queued on the
// driver's stream behind the in-flight frames, no host wait
int set_light(rt_renderer* r, const float light[3], uint32_t* launches);
// the shadow lists for the current light, queued on the driver's stream (the
// set_light policy 0, or a deferred build once the light stays)
int queue_lists(rt_renderer* r, uint32_t* launches);
// read the status of lists queued by set_light (waits for the device): their
// size, an overflow refill, r->sl_built
int settle_lists(rt_renderer* r);
// rt_renderer_set_lights: one list set per light (r->lsets[0 .. n)), each by the chain
// queue_lists runs for set 0 -- the chains share the setup's scratch and are stream-ordered;
// each set's status is read (an overflow refilled at its exact size) before the next chain
// starts, so the call waits for the device.  lists false: no set is built (slist_on 0).
int build_light_sets(rt_renderer* r, const float (*lights)[3], uint32_t n, bool lists, uint32_t* launches);
// whether lists with this longest list and this many entries are built
// (RT_BLIST_MAX_LIST, the device sort's limit; env RT_BLIST_MAX_ENTRIES,
// default 16 M entries = 512 MiB of list and sort buffers)
bool block_lists_fit(uint64_t longest, uint64_t entries);

}  // namespace rtapp
