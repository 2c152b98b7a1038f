/*
 * vx_rt.h -- C-ABI of the ray-tracing host app (librtapp.so).
 *
 * This is the host side of the north-star "tests/regression RT app": the
 * analog of tests/regression/draw3d/main.cpp (scene load, per-frame state
 * setup, upload, vx_start/vx_ready_wait, framebuffer read-back), built on the
 * public vortex.h API and therefore on whatever driver VORTEX_DRIVER selects
 * (libvortex-hip.so on MI355X).  The rtapp executable is its CLI with
 * draw3d's flags; Python (skybox_rt_amd.rt) and bench.py bind it via ctypes.
 *
 * All functions return 0 on success and a negative value on error; the last
 * error message of the calling thread is available from rt_last_error().
 */
#ifndef VX_RT_H
#define VX_RT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_scene* rt_scene_h;
typedef struct rt_renderer* rt_renderer_h;

typedef struct {
  uint32_t num_drawcalls, num_prims, num_geometry, num_layer, num_textures;
  uint32_t bvh_nodes, bvh_tris, bvh_leaves, bvh_depth;
  uint32_t bvh4_nodes, bvh4_depth, bvh4_stack;  /* the 4-wide BVH collapsed from it */
  uint32_t bvh4_f16;  /* 1: BVH4 boxes rounded outward to binary16, the kernel reads 64-B nodes */
  double parse_ms, bvh_ms;
} rt_scene_info_t;

#define RT_RENDER_SHADOWS 0x1u
#define RT_RENDER_PATH 0x8u            /* diffuse path trace (pt_kernel), `bounces` segments */
#define RT_RENDER_FLAT 0x10u           /* flat triangle list, no BVH (config 2; rt_flat) */
#define RT_RENDER_RASTER 0x20u         /* the draw3d raster pipeline (raster_kernel): any
                                          scene incl. blending/stencil; shard_count 1 */
#define RT_RENDER_BVH2 0x40u           /* traverse the binary BVH (default: the 4-wide one;
                                          env RT_BVH_WIDTH=2 flips the default) */
#define RT_RENDER_INSTRUMENTED 0x100u  /* use the counting kernel variant */
#define RT_RENDER_COMPACT 0x200u       /* compact tile-order output (the shard layout,
                                          implied by shard_count > 1) for one shard too */
#define RT_RENDER_COUNTERS 0x400u      /* per-workgroup counter rows on (vx_hip_set_counters):
                                          rt_render_stats' ray / hit counts; implied by
                                          RT_RENDER_INSTRUMENTED.  Off, a frame writes only
                                          its framebuffer (and one task-count word) */
#define RT_RENDER_HOST_SETUP 0x800u    /* build the per-resolution records (shading and
                                          visibility records, primary tree, tile order,
                                          clears) with the host loops instead of on the
                                          device (kernels/rt_setup.hip, the default; env
                                          RT_SETUP=host does the same) */
#define RT_RENDER_COVERAGE 0x1000u     /* with RT_RENDER_RASTER: the raster regression app's
                                          coverage image (tests/regression/raster/kernel.cpp:
                                          covered pixels 0xffffffff, no shading, no OM state) */
#define RT_RENDER_BVH_WALK 0x2000u     /* primary+shadow / path frames without the per-block
                                          and light-space lists: primary visibility by the BVH4
                                          packet walk, shadow rays by the BVH (BASELINE config 3's
                                          "full BVH traversal"); primary+shadow frames run their
                                          own image (rt_bvh: entry vx_main_rt_bvh).  Env
                                          RT_BLOCK_LISTS=0 RT_SHADOW_LISTS=0 give the same frames
                                          on the default image */

typedef struct {
  uint32_t width, height;
  uint32_t flags;             /* RT_RENDER_* */
  float light[3];             /* point light, clip (x, y, w) space */
  uint32_t clear_color;       /* ARGB8888, 0xff000000 in draw3d */
  uint32_t shard_index;       /* this device renders 32x32 tiles t with */
  uint32_t shard_count;       /*   t % shard_count == shard_index */
  uint32_t bounces;           /* RT_RENDER_PATH: bounce segments per path (config 4: 4) */
  uint32_t seed;              /* RT_RENDER_PATH: RNG seed (config 4: 0x5EED) */
  uint32_t tile_logsize;      /* RT_RENDER_RASTER: binning tile side 2^k (draw3d / raster -k,
                                 gfxutil.cpp:237-250; 2..15), 0 = RASTER_TILE_LOGSIZE (5) */
} rt_render_params_t;

typedef struct {
  uint64_t primary_rays, shadow_rays, geometry_hits, occluded;      /* RT_RENDER_COUNTERS */
  uint64_t node_visits, tri_tests, layer_tests, shaded, texel_bytes; /* instrumented only */
  uint64_t tasks;             /* VX_CSR_MINSTRET */
  double kernel_ms;           /* HIP-event time of the last launch */
  uint32_t grid, block;       /* launch geometry chosen by the driver */
  uint32_t num_tasks, local_tiles;
  uint64_t bounce_rays;       /* RT_RENDER_PATH: bounce segments traced */
  uint64_t rect_tests;        /* RT_RENDER_FLAT, instrumented: list entries whose rectangle a
                                 wave tested (per wave, the work executed) */
  uint64_t edge_tests;        /* RT_RENDER_FLAT, instrumented: entries some lane of the wave
                                 lay in, whose edges and depth the wave evaluated */
} rt_stats_t;

const char* rt_last_error(void);

int rt_scene_load(const char* path, rt_scene_h* out);
/* draw3d's -s start / -e end (tests/regression/draw3d/main.cpp:179-181): only
 * drawcalls start <= d <= end are drawn (rt_scene_load = 0, 0xffffffff) */
int rt_scene_load_range(const char* path, uint32_t start_draw, uint32_t end_draw, rt_scene_h* out);
/* rt_scene_load_range with flags.  RT_SCENE_OM_LAYERS: a scene the RT path
 * cannot trace as a whole -- a drawcall blends, uses the stencil, masks colour
 * channels, tests depth without writing it or with another function than the
 * drawcalls before it, or is a depth-off layer after geometry -- is split at
 * the first such drawcall.  The drawcalls before it (the traced head) are what
 * the scene's geometry / layer sets, its BVH and rt_scene_info describe; that
 * drawcall and every one after it, whatever their states, are the ordered
 * tail.  Plain and RT_RENDER_SHADOWS frames of such a scene trace the head as
 * always (raster-exact primary visibility, layers, shading, one shadow ray per
 * geometry hit, the head's depth-tested primitives the only occluders) and then
 * fold every tail primitive that covers a pixel over the pixel's colour and
 * depth/stencil word in ascending primitive index through the output merger
 * (depth/stencil test, blending, write masks), one launch of rt_om_kernel.hip
 * that stores each pixel once.  Without shadows that is the raster pipeline's
 * frame of the whole scene; tail fragments cast no shadow rays and occlude
 * none.  A scene with an empty tail behaves as if loaded without the flag.
 * Without the flag (rt_scene_load, rt_scene_load_range) nothing changes: such
 * a scene is unsupported on the RT path and renders with RT_RENDER_RASTER. */
#define RT_SCENE_OM_LAYERS 0x1u
int rt_scene_load_ex(const char* path, uint32_t start_draw, uint32_t end_draw, uint32_t flags,
                     rt_scene_h* out);
/* the split of a scene loaded with RT_SCENE_OM_LAYERS: the first drawcall of
 * the ordered tail (num_drawcalls when the tail is empty or the flag was not
 * given) and the tail's primitive count */
int rt_scene_om_split(rt_scene_h scene, uint32_t* first_tail_drawcall, uint32_t* tail_prims);
int rt_scene_free(rt_scene_h scene);
int rt_scene_info(rt_scene_h scene, rt_scene_info_t* info);
/* flattened triangles, float[num_prims][3][10] (x,y,z,w, r,g,b,a, u,v) */
int rt_scene_export_prims(rt_scene_h scene, float* out, uint64_t count);
/* BVH arrays: float[bvh_nodes][16], float[bvh_tris][12] */
int rt_scene_export_bvh(rt_scene_h scene, float* nodes, float* tris);
/* 4-wide BVH nodes: float[bvh4_nodes][32] (rt_node4_t); leaves index the same tris */
int rt_scene_export_bvh4(rt_scene_h scene, float* nodes4);
/* fixed-point shading records (rt_prim_t) at width x height: int32[num_prims][32] */
int rt_scene_setup_prims(rt_scene_h scene, uint32_t width, uint32_t height, int32_t* out,
                         uint64_t count);
/* the background-layer table (RT_REC_BGLAYER) of a width x height frame on the host alone: uint32[2] per
 * 8x8-block chunk from `first_chunk` on, the 32x32 tiles in the order `order` gives (num_tiles entries;
 * NULL: row-major), 16 chunks a tile; count = records `out` holds, *size = records written */
int rt_scene_bg_layers(rt_scene_h scene, uint32_t width, uint32_t height, const uint32_t* order,
                       uint32_t first_chunk, uint32_t* out, uint64_t count, uint64_t* size);
/* the per-block candidate lists of a width x height frame and the same lists trimmed to their winners
 * (RT_REC_BIDX, RT_REC_BLIST, RT_REC_BTIDX, RT_REC_BTRIM of one shard), on the host alone: *entries =
 * the untrimmed lists' entries (blist and btrim hold entries + 3 padding records of uint32[4]), *blocks
 * = the shard's 8x8 blocks (bidx and btidx hold uint32[2] each).  NULL arrays: sizes only.  NO REFERENCE. */
int rt_scene_block_trim(rt_scene_h scene, uint32_t width, uint32_t height, uint32_t shard_index,
                        uint32_t shard_count, uint32_t* bidx, uint32_t* blist, uint32_t* btidx, uint32_t* btrim,
                        uint64_t* entries, uint64_t* blocks);
/* primary-visibility record of every primitive at width x height (the RT
 * kernels' raster-exact primary rays, rt_common.h): uint32[num_prims][3] =
 * covered-pixel rectangle x0 | x1 << 16, y0 | y1 << 16 (inclusive; empty:
 * 0x0000ffff) and the lower bound of its 24-bit depth word.  NO REFERENCE
 * (derived from draw3d's coverage rule; oracle/vis.c restates it). */
int rt_scene_setup_vis(rt_scene_h scene, uint32_t width, uint32_t height, uint32_t* out,
                       uint64_t count);
/* the screen-space BVH4 the primary rays walk at width x height (what
 * rt_renderer_configure builds; depth_scale 0 = the default 2D SAH):
 * int32 refs[num_nodes][4], leaf_pids[num_leaf], worst-case stack; NULL
 * arrays = counts only.  NO REFERENCE. */
int rt_scene_vis_tree(rt_scene_h scene, uint32_t width, uint32_t height, float depth_scale,
                      int32_t* refs, uint32_t* num_nodes, int32_t* leaf_pids, uint32_t* num_leaf,
                      uint32_t* stack4);
/* the ordered tail's per-block lists at width x height, one shard (what
 * rt_renderer_configure builds and uploads, app/vis.h BuildTailLists): for
 * every 8x8 block -- block (tile row * tiles per row + tile column) * 16 +
 * (by & 3) * 4 + (bx & 3), RT_REC_BIDX's numbering -- idx[2] = first entry and
 * count, ent = the primitive indices of the tail primitives whose
 * covered-pixel rectangle reaches the block, ascending.  NULL arrays: sizes
 * only.  NO REFERENCE. */
int rt_scene_setup_olists(rt_scene_h scene, uint32_t width, uint32_t height, uint32_t* idx, uint32_t* ent,
                          uint64_t* entries, uint64_t* blocks);

/* kernel_dir: directory holding rt_kernel.vxbin / rt_kernel_stats.vxbin
 * (NULL = next to librtapp.so).  Opens its own vortex device.  Scenes the
 * RT path cannot trace as a whole (blending, stencil, layers after geometry)
 * get a renderer that accepts only RT_RENDER_RASTER (configure returns -2
 * otherwise) -- unless the scene was loaded with RT_SCENE_OM_LAYERS: then
 * plain and RT_RENDER_SHADOWS frames (with RT_RENDER_COUNTERS, COMPACT,
 * HOST_SETUP and shards as usual) trace the head and fold the ordered tail
 * (image rt_om.vxbin; ordinary frames, one framebuffer, no frame overlap),
 * RT_RENDER_RASTER works as ever, and RT_RENDER_PATH / FLAT / BVH_WALK /
 * INSTRUMENTED, or a tree other than the binary16 BVH4 (the generic deep
 * images' layouts: RT_RENDER_BVH2, env RT_BVH_F16=0), return -2. */
int rt_renderer_create(rt_scene_h scene, const char* kernel_dir, rt_renderer_h* out);
int rt_renderer_free(rt_renderer_h r);
int rt_renderer_configure(rt_renderer_h r, const rt_render_params_t* params);
/* Start a frame without waiting for it.  Frames started back to back queue
 * on the device (the driver's VX_HIP_QUEUE_DEPTH).  A configuration whose
 * frame is one launch that writes only framebuffer pixels -- whole
 * (not compact / sharded) primary+shadow, flat or one-kernel path frames
 * without counters -- keeps two framebuffers: frame n renders into buffer
 * n mod 2 on the driver's launch lane n mod 2 (vortex_hip.h
 * vx_hip_set_launch_lane), so two consecutive frames may run on the device
 * at the same time (the first waves of one fill the slots the last waves of
 * the other leave empty) while frames sharing a buffer stay ordered.  Every
 * other frame, and everything that is not a frame (setup launches, list
 * rebuilds, uploads), runs behind the frames in flight on both lanes and
 * ahead of every frame started after it; so does the frame right behind a
 * list rebuild.  rt_render (start + wait) is such
 * an ordinary frame too: it renders into the buffer in use, the synchronous
 * path of the rounds before.  Env VX_HIP_OVERLAP=0: one lane, one
 * framebuffer, the frames run one after the other. */
int rt_render_start(rt_renderer_h r);
int rt_render_wait(rt_renderer_h r);
int rt_render(rt_renderer_h r);  /* start + wait */

/* Progressive path tracing: samples per pixel accumulated on the device.
 * NO REFERENCE (the reference has no path tracer, SURVEY.md 8(a) row A7;
 * none of the entry points below has a counterpart there).
 *
 * Sample i of a renderer configured with seed s0 is the RT_RENDER_PATH pixel
 * of seed (s0 + i) mod 2^32 as rt_render stores it (8 bits per channel; a
 * pixel that starts no path: its primary colour).  One 16-byte record per
 * framebuffer pixel, uint32 {sumR, sumG, sumB, n} at the pixel's framebuffer
 * index (the compact / sharded layout included): the per-channel sums of the
 * sample values and the number of samples in them.  An accumulation launch
 * of k samples (image pt_accum.vxbin) resolves primary visibility, layers
 * and shading once, reads each record, traces samples n .. n + k - 1, writes
 * the record back with n + k and stores alpha | mean(R) << 16 | mean(G) << 8
 * | mean(B) to the framebuffer in use, mean(c) = (2 * sum_c + n) / (2 * n) in
 * integer division (rt_accum_resolve) -- so n is the sample cursor, nothing
 * reaches the kernel between launches and launches queue back to back.  The
 * first launch after accum_begin, accum_reset or rt_renderer_set_light (a
 * moved light changes the integrand) treats every record as zero without
 * reading it: no clearing launch, no copy.  With RT_RENDER_COUNTERS a
 * launch's primary_rays / geometry_hits count once, shadow_rays / occluded /
 * bounce_rays are the sums over its k samples.
 *
 * Accumulation launches are ordinary launches (no lane, the image's grid):
 * they run behind overlapped frames in flight on both lanes.  Plain
 * rt_render_start / rt_render frames in between behave as ever and leave the
 * records alone.  rt_renderer_configure ends accumulation and frees the
 * records. */
/* on a configured RT_RENDER_PATH frame: allocate W*H*16 B (compact: local
 * tiles * 1024 * 16 B); the next launch resets.  -2 (rt_last_error): not a
 * path frame, RT_RENDER_INSTRUMENTED, the two-kernel queue form (env
 * RT_PT_QUEUE=1), a kernel directory with its own pt_kernel.vxbin and no
 * pt_accum.vxbin (pt_compact), a tree the generic (deep) images run.
 * RT_RENDER_COUNTERS, BVH_WALK, COMPACT, HOST_SETUP and shards accumulate.
 * NO REFERENCE. */
int rt_renderer_accum_begin(rt_renderer_h r);
/* the next launch resets; queues nothing.  NO REFERENCE. */
int rt_renderer_accum_reset(rt_renderer_h r);
/* one launch of `samples` (1..32) samples per pixel, no host wait; -2 for
 * samples out of range, before accum_begin, or when the launch would take n
 * past 2^24 (below that the u32 sums cannot overflow).  NO REFERENCE. */
int rt_render_accumulate_start(rt_renderer_h r, uint32_t samples);
int rt_render_accumulate(rt_renderer_h r, uint32_t samples);  /* start + wait.  NO REFERENCE. */
/* samples queued since the last reset (the records' n once the launches ran).  NO REFERENCE. */
int rt_renderer_accum_samples(rt_renderer_h r, uint32_t* n);
/* the records, uint32[count][4] in framebuffer order (waits for the device).  NO REFERENCE. */
int rt_read_accum(rt_renderer_h r, uint32_t* out, uint64_t count);
/* the host restatement of the resolve: alpha_argb's alpha over the rounded
 * means of rec = {sumR, sumG, sumB, n} (n = 0: alpha alone; a mean is clamped
 * to 255, which sums of 8-bit samples never exceed).  NO REFERENCE. */
uint32_t rt_accum_resolve(const uint32_t rec[4], uint32_t alpha_argb);

int rt_render_stats(rt_renderer_h r, rt_stats_t* stats);
/* HIP-event duration of the last launch only (no counter read-back) */
int rt_render_kernel_ms(rt_renderer_h r, double* kernel_ms);
/* waits for every started frame, then, since the renderer's device opened:
 * the summed HIP-event kernel time of the timed launches, their number, and
 * the number of all launches.  Back-to-back rt_render_start calls queue
 * behind the in-flight frame (the driver's VX_HIP_QUEUE_DEPTH) and are timed
 * one in VX_HIP_TIME_EVERY: kernel_ms_sum / timed is their average. */
int rt_render_run_totals(rt_renderer_h r, double* kernel_ms_sum, uint64_t* timed,
                         uint64_t* launches);
/* 1: launches timed by HIP events as above (the default); 0: untimed -- no
 * events and no queue bound, so a run of rt_render_start calls reaches the
 * GPU back to back (bench.py's stream clock: wall time of K such frames / K).
 * Waits for the in-flight frames. */
int rt_render_set_timing(rt_renderer_h r, int timed);
/* linear W*H framebuffer (shard_count == 1) or compact tile buffer
 * (local_tiles * 1024 pixels in task order) of the last started frame */
int rt_read_framebuffer(rt_renderer_h r, uint32_t* out, uint64_t count);
/* the frame started before it, while the configuration keeps two
 * framebuffers (rt_render_start) and two frames were started since the
 * configure; an error otherwise */
int rt_read_framebuffer_prev(rt_renderer_h r, uint32_t* out, uint64_t count);

/* RT_RENDER_RASTER: the depth/stencil buffer (stencil << 24 | depth), W*H */
int rt_read_depthbuffer(rt_renderer_h r, uint32_t* out, uint64_t count);

/* Build the BVH on the device (Morton codes, radix
 * sort, binary radix tree, bottom-up boxes -- kernels/bvh_build.hip) from
 * the scene's triangles and make it this renderer's tree (binary traversal;
 * a configured renderer is reconfigured).  Stats optional. */
typedef struct {
  uint32_t nodes, depth, launches;
  uint32_t stack4;      /* worst-case stack of the device BVH4 collapse (traversed by the
                           RT/PT kernels), RT_BVH_STACK4_UNUSED if it exceeds the deep
                           images' stack and the BVH2 is traversed instead */
  double build_ms;      /* host wall time of the whole build (upload + launches) */
  double kernel_ms;     /* LBVH: sum of the build kernels' HIP-event times; SAH: host wall time
                           of the launch sequence and its one read-back (per-launch event
                           times under env RT_SAH_TRACE) */
  uint32_t nodes4;      /* rt_node4_t records (LBVH: one per BVH2 index, zeros at absorbed nodes) */
  uint32_t depth4;      /* BVH4 depth (SAH build; 0 for the LBVH) */
  uint32_t method;      /* RT_BVH_BUILD_* */
  uint32_t pad;
} rt_bvh_build_stats_t;
int rt_renderer_build_bvh(rt_renderer_h r, rt_bvh_build_stats_t* stats);  /* = _ex(LBVH) */
/* RT_BVH_BUILD_LBVH: Morton codes + radix tree (kernels/bvh_build.hip, 19
 * launches, fastest build).  RT_BVH_BUILD_SAH: the host builder's binned-SAH
 * tree, BVH4 collapse and binary16 planes restated on the device
 * (kernels/bvh_sah.hip): one stream-ordered launch sequence -- the init, a
 * split launch per tree level for a budget of log2(n) + 4 levels, 7
 * finishing launches -- with one read-back at the end (a deeper tree
 * continues once per further budget); the same arrays as the scene's host
 * build, bit for bit.  The build image and its scratch stay with the
 * renderer, so a rebuild loads nothing. */
#define RT_BVH_BUILD_LBVH 0u
#define RT_BVH_BUILD_SAH 1u
#define RT_BVH_BUILD_HOST 2u  /* the scene's host build (app/bvh.cpp) uploaded: env RT_BVH=host */
int rt_renderer_build_bvh_ex(rt_renderer_h r, uint32_t method, rt_bvh_build_stats_t* stats);
/* How the renderer's current tree was built: rt_renderer_create builds it on
 * the device with RT_BVH_BUILD_SAH (the host builder's tree bit for bit;
 * RT_BVH_BUILD_HOST under env RT_BVH=host or for a scene without geometry),
 * or the last rt_renderer_build_bvh_ex. */
int rt_renderer_bvh_stats(rt_renderer_h r, rt_bvh_build_stats_t* stats);
#define RT_BVH_STACK4_UNUSED 0xFFFFFFFFu
/* the renderer's current BVH4 (float[num_nodes4][32], rt_node4_t: the host
 * tree's collapse, or after rt_renderer_build_bvh the device collapse --
 * BVH4 node i at the BVH2 index of every even-depth internal node, zeros
 * elsewhere).  NO REFERENCE. */
int rt_renderer_export_bvh4(rt_renderer_h r, float* nodes4, uint32_t* num_nodes4);
/* the same nodes as 64-B rt_node4h_t records (binary16 planes, the layout the
 * kernels read), num_nodes4 * 64 bytes */
int rt_renderer_export_bvh4h(rt_renderer_h r, void* nodes4h, uint32_t* num_nodes4);
/* the renderer's current BVH (float[num_nodes][16], float[num_tris][12]) */
int rt_renderer_export_bvh(rt_renderer_h r, float* nodes, float* tris, uint32_t* num_nodes,
                           uint32_t* num_tris);

/* the primary rays' tree of the current configuration (NO REFERENCE): child
 * references int32[num_nodes][4] (rt_node4_t child encoding; leaf refs index
 * leaf_pids) and the pid of every leaf record -- by default a per-resolution
 * screen-space BVH4 over the covered-pixel rectangles (app/vis.h
 * BuildScreenTree).  NULL arrays: counts only. */
int rt_renderer_export_vis_tree(rt_renderer_h r, int32_t* refs, uint32_t* num_nodes,
                                int32_t* leaf_pids, uint32_t* num_leaf);

/* How the last rt_renderer_configure built its per-resolution records.  The
 * reference builds them per drawcall on the host (draw3d/main.cpp:179-211 ->
 * graphics::Binning, gfxutil.cpp:103-276); here kernels/rt_setup.hip builds
 * them unless RT_RENDER_HOST_SETUP. */
typedef struct {
  uint32_t device;        /* 1: device setup, 0: host loops */
  uint32_t launches;      /* device setup launches */
  uint32_t heavy_tiles;   /* local tiles whose weight (covering geometry primitives) > 0 */
  uint32_t blist_blocks;  /* local 8x8 blocks with candidate lists (0: primary rays walk the tree) */
  double setup_ms;        /* host wall time of the record build (uploads / launches included) */
  double configure_ms;    /* host wall time of the whole rt_renderer_configure */
  uint64_t blist_entries; /* candidate-list entries (0 when not built) */
  uint32_t blist_max;     /* the longest list */
  uint32_t slist_on;      /* 1: shadow rays test the light-space lists (rt_common.h) */
  uint64_t slist_entries; /* light-space shadow list entries */
  uint32_t path_queue;    /* 1: RT_RENDER_PATH runs in two kernels (pt_primary + pt_queue: a
                             frame is one launch group of 2, vortex_hip.h) */
  uint32_t slist_built;   /* 1: the last configure / set_light built shadow lists for a new light
                             (0: the lists of an unchanged light were kept) */
  uint32_t slist_stale;   /* 1: the light moved since its lists were built and none are queued:
                             frames walk the BVH for their shadow rays (rt_renderer_set_list_policy) */
  uint32_t lane_grid;     /* workgroups of a frame started on a launch lane (rt_render_start with
                             frames overlapping): its waves take RT_LANE_CHUNKS (2) chunks each;
                             0: the image's grid, as every frame rendered alone by rt_render */
  uint32_t bg_first_chunk; /* the background tier: the first chunk of the work order behind the
                             tiles geometry reaches (16 * heavy_tiles); 0: the configuration is
                             never tiered */
  uint32_t tier_groups;   /* the geometry tier's workgroups (the launch tag) of a frame started
                             on a launch lane -- with env RT_BG_TIER=2 of a frame rendered alone
                             -- now; 0: that frame is untiered */
  uint64_t btrim_entries; /* the trimmed block lists (RT_REC_BTRIM) the frames scan: the entries kept --
                             0: no trim (no lists, RT_RENDER_INSTRUMENTED, env RT_BLIST_TRIM=0) */
  uint32_t btrim_blocks;  /* ... and the blocks that keep any */
  uint32_t fused_chunk;   /* 1: the frames carry RT_FLAG_FUSED -- image rt_kernel traces a wave's last
                             geometry chunk's shadow rays in place while the lists hold (env
                             RT_FUSED_CHUNK=0 at configure: 0) */
} rt_setup_stats_t;
/* (reads back the status of shadow lists queued by rt_renderer_set_light:
 * waits for the device) */
int rt_renderer_setup_stats(rt_renderer_h r, rt_setup_stats_t* stats);

/* Move the point light of the current configuration (primary+shadow or path
 * frames; clip (x, y, w)): the light in the render arguments, queued behind
 * the frames already started, with no host wait; the frames started after it
 * see the new light.  When the configuration's shadow rays use the
 * light-space lists, the lists for the new light are a stream-ordered chain
 * of setup launches (kernels/rt_setup.hip SPROJ .. SSORT, ~0.1 ms at 1024^2;
 * with overlapped frames the chain waits for the frames in flight on both
 * launch lanes before it overwrites the lists, and the frames started after
 * it wait for it on either lane)
 * whose last launch decides on the device whether they fit (else the frames'
 * shadow rays walk the BVH).  By default (rt_renderer_set_list_policy) the
 * chain is deferred: the frames after the change trace their shadow rays by
 * the BVH packet walk -- the same verdicts, no wait for lists -- and the
 * lists are queued once the light has stayed for `defer_frames` frames.  The
 * reference re-bins its scene on the host for every render
 * (tests/regression/draw3d/main.cpp:179-211 -> gfxutil.cpp:103-276); this
 * is the per-frame handling of the only light-dependent structure. */
int rt_renderer_set_light(rt_renderer_h r, const float light[3]);
/* When set_light queues a light's shadow lists: 0 = at once (set_light);
 * n > 0 = before the (n + 1)-th frame started with that light, the n frames
 * before walking the BVH for their shadow rays (default 8, env
 * RT_SLIST_DEFER; a build costs about as much as that many frames save).
 * NO REFERENCE. */
int rt_renderer_set_list_policy(rt_renderer_h r, uint32_t defer_frames);

/* Several point lights, traced in one launch.  NO REFERENCE (the reference
 * has one light; none of the entry points below has a counterpart there).
 *
 * A frame lit by lights L_0 .. L_{n-1} (1 <= n <= RT_MAX_LIGHTS) is, per
 * pixel and colour channel, the rounded mean of the n RT_RENDER_SHADOWS
 * frames of the single lights: mean = (2 * sum + n) / (2 * n) in integer
 * division (rt_accum_resolve on {sums, n}); the alpha byte is the primary
 * colour's.  A single-light frame stores a shadow ray's colour c or c >> 1
 * per channel, so with o = the lights that do not see the ray, sum = (n - o)
 * * c + o * (c >> 1) (rt_lights_resolve); a pixel without a shadow ray is c.
 * Primary visibility, layers, shading and texel reads run once per frame; in
 * the drain every packet of queued shadow rays is tested against each light
 * in turn, on that light's own light-space lists or, for a light whose lists
 * do not fit, by the BVH packet walk (images rt_lights / rt_lights_stats).
 *
 * rt_renderer_set_lights: valid on a configured plain RT_RENDER_SHADOWS
 * frame on the binary16 BVH4 (RT_RENDER_COUNTERS, INSTRUMENTED, COMPACT,
 * shards and HOST_SETUP as usual).  It builds one set of lists per light at
 * once -- no deferral; with env RT_SHADOW_LISTS=0 or under RT_RENDER_HOST_SETUP
 * none, every light walks the BVH -- reads each set's status and uploads the
 * light table: it WAITS FOR THE DEVICE, like a configure.  -2 (rt_last_error
 * says why) for n outside 1..16, a configuration without RT_RENDER_SHADOWS or
 * with RT_RENDER_PATH / FLAT / RASTER / BVH_WALK, a scene with a non-empty
 * ordered tail (RT_SCENE_OM_LAYERS), a tree the generic (deep) images run, a
 * kernel directory without rt_lights.vxbin.  With n >= 2 the frames after it
 * (rt_render, rt_render_start) are ordinary launches of the new image on its
 * own grid into the framebuffer in use -- no launch lane, no overlap.  n = 1
 * is rt_renderer_set_light under list policy 0.  rt_renderer_set_light and
 * rt_renderer_configure return to one light. */
#define RT_MAX_LIGHTS 16u
int rt_renderer_set_lights(rt_renderer_h r, const float (*lights)[3], uint32_t n);
typedef struct {
  float light[3];
  uint32_t slist_on;       /* 1: the light's shadow rays scan its light-space lists; 0: walk the BVH */
  uint64_t slist_entries;  /* entries of its lists (also when they did not fit) */
} rt_light_info_t;
/* the lights in use (one entry after set_light / configure), at most max; *n = their number */
int rt_renderer_lights_info(rt_renderer_h r, rt_light_info_t* out, uint32_t max, uint32_t* n);
/* light `light`'s list arrays, which = RT_REC_SIDX or RT_REC_SLIST, as
 * rt_renderer_export_records gives the single light's (out NULL = size query) */
int rt_renderer_export_light_lists(rt_renderer_h r, uint32_t light, uint32_t which, void* out, uint64_t bytes,
                                   uint64_t* size);
/* the host restatement of the device resolve: the pixel of a shadow ray of
 * primary colour argb that `occluded` of its k lights do not see */
uint32_t rt_lights_resolve(uint32_t argb, uint32_t occluded, uint32_t k);

/* Several point lights on a path-traced frame, traced in one launch.  NO
 * REFERENCE (the reference has neither a path tracer nor a second light).
 *
 * A path frame lit by lights L_0 .. L_{n-1} (1 <= n <= RT_MAX_PATH_LIGHTS) is,
 * per pixel and colour channel, the rounded mean (2 * sum + n) / (2 * n) in
 * integer division of the n single-light 8-bit RT_RENDER_PATH frames of the
 * same seed (rt_accum_resolve on {sums, n}; rt_path_lights_resolve), under
 * the primary colour's alpha; a pixel that starts no path is its primary
 * colour.  A path's vertices -- primary hit, bounce directions (keyed by
 * pixel, vertex and seed), albedos, throughput -- do not depend on the
 * light, so the kernel traces every bounce ray once and at each vertex one
 * shadow ray per light, on that light's own light-space lists, into one
 * radiance accumulator per light that takes the single-light frame's own
 * operations (images pt_lights / pt_lights_accum).  Counters
 * (RT_RENDER_COUNTERS): primary_rays, geometry_hits and bounce_rays are one
 * single-light frame's; shadow_rays and occluded are the sums over the n
 * single-light frames.
 *
 * rt_renderer_set_path_lights: valid on a configured RT_RENDER_PATH frame
 * that rt_renderer_accum_begin would accept -- the one-kernel per-lane form
 * on the binary16 BVH4, not RT_RENDER_INSTRUMENTED -- whose shadow rays scan
 * light-space lists (RT_RENDER_COUNTERS, COMPACT and shards as usual).  It
 * builds one set of lists per light at once, reads each set's status and
 * uploads the light table: it WAITS FOR THE DEVICE, like a configure.  With
 * n >= 2 the frames after it (rt_render, rt_render_start) launch pt_lights
 * and rt_render_accumulate[_start] launch pt_lights_accum, all as ordinary
 * launches on the image's grid into the framebuffer in use -- no launch
 * lane, no overlap.  Sample j of an accumulation is then the n-light frame of
 * seed s0 + j (an 8-bit value per channel); records and the sample cursor
 * keep their form.  n = 1 is rt_renderer_set_light under list policy 0.
 * While accumulation is on, the call starts the records over, as
 * rt_renderer_set_light does.  rt_renderer_set_light and
 * rt_renderer_configure return to one light; rt_renderer_lights_info and
 * rt_renderer_export_light_lists report the sets.
 * -2 (rt_last_error says why) for n outside 1..RT_MAX_PATH_LIGHTS, a
 * configuration without RT_RENDER_PATH or with RT_RENDER_INSTRUMENTED, one
 * without light-space lists (RT_RENDER_BVH_WALK, RT_RENDER_HOST_SETUP, env
 * RT_SHADOW_LISTS=0, a scene without geometry), the two-kernel queue (env
 * RT_PT_QUEUE=1), a tree the generic (deep) images run, a kernel directory
 * with a pt_kernel.vxbin of its own and no pt_lights.vxbin /
 * pt_lights_accum.vxbin, and any light whose lists do not fit (there is no
 * BVH fallback per light).  After a refusal the renderer is lit by its single
 * light, as after rt_renderer_set_light. */
#define RT_MAX_PATH_LIGHTS 8u
int rt_renderer_set_path_lights(rt_renderer_h r, const float (*lights)[3], uint32_t n);
/* the host restatement of the device mean: the pixel whose k single-light
 * values sum to sums[0..2] = {R, G, B}, under alpha_argb's alpha byte; k
 * outside 1..RT_MAX_PATH_LIGHTS or a sum above 255 * k: the alpha byte alone */
uint32_t rt_path_lights_resolve(const uint32_t sums[3], uint32_t k, uint32_t alpha_argb);

/* Per-pixel visibility records of a primary+shadow frame, in one launch.  NO
 * REFERENCE (the reference returns colours only; the oracle's rt_render gives
 * pid and t per pixel, its raster_render the depth words, and the records are
 * held to both bit for bit).
 *
 * What a frame resolves per pixel and drops at its store: one 16-byte record
 * per framebuffer pixel, at the pixel's framebuffer index -- linear W * H, or
 * for compact / sharded configurations local_tiles * 1024 in task order,
 * exactly as rt_read_framebuffer orders pixels.  The launch (image rt_aov,
 * kernels/rt_aov_kernel.hip) does primary visibility, the layer resolve and
 * one shadow ray per light in use, in place; it shades nothing and reads no
 * texel.  A k-light frame's pixel is a pure function of the unshadowed
 * frame's pixel and the record's mask (rt_aov_relight), so a client may dim,
 * colour or switch off single lights without rendering again.
 *
 * The lights in use: one light after rt_renderer_configure or
 * rt_renderer_set_light -- the argument block and the launch words exactly as
 * a frame has them: a moved light whose lists are deferred or stale walks the
 * BVH and gives the same verdicts -- and n lights after
 * rt_renderer_set_lights, each on its own lists or, where it has none, by the
 * BVH packet walk.
 *
 * rt_render_aov_start: valid on a configured primary+shadow-family frame --
 * with or without RT_RENDER_SHADOWS (without: masks and RT_AOV_SHADOW_RAY all
 * zero), RT_RENDER_BVH_WALK, COUNTERS, COMPACT, shards and HOST_SETUP as
 * usual.  -2 (rt_last_error says why) for RT_RENDER_PATH, FLAT, RASTER or
 * INSTRUMENTED, a scene with a non-empty ordered tail (RT_SCENE_OM_LAYERS), a
 * tree the generic (deep) images run.  The image (rt_aov.vxbin: the kernel
 * directory's, else the library's) is loaded by the first call and kept for
 * the renderer's life; the record buffer is allocated by the first call after
 * a configure (rt_renderer_configure and rt_renderer_free release it); later
 * calls queue one launch and no copy.  An ordinary launch, as an accumulation
 * launch is: no launch lane, the image's own grid, behind the frames in
 * flight on both lanes and ahead of everything started after it.  It writes
 * only its own buffer -- rt_read_framebuffer still returns the last frame --
 * rt_render_wait covers it, and rt_render_stats / rt_render_kernel_ms after
 * it describe it: with RT_RENDER_COUNTERS primary_rays and geometry_hits are
 * a frame's, shadow_rays is the sum over the lights and occluded the sum of
 * the masks' set bits. */
#define RT_AOV_GEOM 0x01000000u
#define RT_AOV_SHADOW_RAY 0x02000000u
typedef struct {
  int32_t  pid;          /* the shaded primitive: the depth-tested winner, else the last drawn
                            covering screen layer, else -1 (the oracle's rt_render pid) */
  uint32_t depth_flags;  /* bits 0-23: the winner's depth word (0xffffff without a geometry hit)
                            -- the raster pipeline's depth & 0xffffff; bit 24 RT_AOV_GEOM: a
                            geometry hit; bit 25 RT_AOV_SHADOW_RAY: shadow rays start here
                            (RT_RENDER_SHADOWS, a geometry hit, plane t finite and > 0); bits
                            26-31 zero */
  float    t;            /* plane t of the geometry winner as computed (also when not finite or
                            <= 0: then no shadow ray); 0 without a geometry hit (the oracle's t) */
  uint32_t light_mask;   /* bit i: light i of the lights in use does NOT see the pixel (its shadow
                            ray is occluded); 0 without RT_AOV_SHADOW_RAY; bits >= the light count 0 */
} rt_aov_t;
int rt_render_aov_start(rt_renderer_h r);   /* one launch, no host wait once image and buffer exist */
int rt_render_aov(rt_renderer_h r);         /* start + wait */
/* the records in framebuffer order, count >= the framebuffer's pixels (waits for the device) */
int rt_read_aov(rt_renderer_h r, rt_aov_t* out, uint64_t count);
/* = rt_lights_resolve(plain_argb, popcount(light_mask & (2^k - 1)), k): the k-light frame's
 * pixel from the unshadowed frame's pixel and the record's mask (k outside 1..RT_MAX_LIGHTS:
 * plain_argb) */
uint32_t rt_aov_relight(uint32_t plain_argb, uint32_t light_mask, uint32_t k);

/* Relighting a frame on the device from its visibility records.  NO REFERENCE
 * (the relit frame is defined from the oracle's single-light frames and held
 * to them bit for bit).
 *
 * Two launches.  The capture (image rt_aov_base: kernels/rt_aov_kernel.hip
 * built with RT_AOV_BASE) is the record launch above -- the same records, bit
 * for bit, in the same record buffer (rt_read_aov returns them) -- that also
 * shades every pixel without shadows and stores that ARGB word, the pixel's
 * base colour, into a buffer of 4 B per framebuffer pixel in framebuffer order:
 * by definition the pixel of the same configuration's frame without
 * RT_RENDER_SHADOWS.  The relight (image rt_relight, kernels/
 * rt_relight_kernel.hip) is a streaming pass with no scene and no tracing: per
 * framebuffer pixel it reads the record and the base colour and writes the
 * relit pixel into the framebuffer in use.
 *
 * The relit pixel.  n = the lights in use at capture time (1 after
 * rt_renderer_configure / rt_renderer_set_light, k after
 * rt_renderer_set_lights); light i weighs w_i in 0..255; W = sum of the w_i;
 * O = sum of the w_i of the lights whose bit in light_mask is set (bits at or
 * above n are ignored).  A pixel with RT_AOV_SHADOW_RAY is, per colour channel
 * c of its base colour, (2 * ((W - O) * c + O * (c >> 1)) + W) / (2 * W) in
 * integer division -- the weighted rounded mean of the single-light frames --
 * under the base colour's alpha byte; a pixel without it is its base colour.
 * With every w_i in {0, 1} that is rt_lights_resolve(base, popcount(mask &
 * enabled), popcount(enabled)): the rt_renderer_set_lights frame of the
 * enabled lights.
 *
 * rt_relight_capture_start: the validity rules and -2 refusals of
 * rt_render_aov_start, and -2 without RT_RENDER_SHADOWS (nothing to relight).
 * An ordinary launch as that one is (no lane, behind the frames in flight on
 * both lanes), the same launch words and tag.  rt_aov_base.vxbin and
 * rt_relight.vxbin (the kernel directory's, else the library's) are loaded by
 * the first call and kept; the record and base-colour buffers are allocated by
 * the first call after a configure (rt_renderer_configure and
 * rt_renderer_free release them).
 *
 * rt_render_relight_start(r, weights, n): one launch of rt_relight into the
 * framebuffer in use -- rt_read_framebuffer returns it, rt_render_wait covers
 * it, rt_render_kernel_ms describes it (it counts nothing: rt_render_stats'
 * counters are 0) -- with no host wait and no copy: the weights travel in the
 * launch words.  Launches queue back to back.  -2 (rt_last_error says why)
 * when there is no capture since the last rt_renderer_configure /
 * rt_renderer_set_light / rt_renderer_set_lights /
 * rt_renderer_set_path_lights (those calls end the session: the masks describe
 * other lights), when n is not the capture's light count, when every weight
 * is 0.  Frames rendered in between leave records and base colours alone. */
int rt_relight_capture_start(rt_renderer_h r);
int rt_relight_capture(rt_renderer_h r);    /* start + wait */
int rt_render_relight_start(rt_renderer_h r, const uint8_t* weights, uint32_t n);
int rt_render_relight(rt_renderer_h r, const uint8_t* weights, uint32_t n);  /* start + wait */
/* the capture's base colours in framebuffer order, count >= the framebuffer's pixels (waits
 * for the device) */
int rt_read_relight_base(rt_renderer_h r, uint32_t* out, uint64_t count);
/* the relit pixel restated on the host, from a pixel's base colour and its record's depth_flags
 * and light_mask; base_argb when n is outside 1..RT_MAX_LIGHTS or W = 0 */
uint32_t rt_relight_resolve(uint32_t base_argb, uint32_t depth_flags, uint32_t light_mask, const uint8_t* weights,
                            uint32_t n);

/* Denoising accumulated path frames on the device, guided by visibility.  NO
 * REFERENCE (the reference has no path tracer; the filter is defined here in
 * integer arithmetic and held bit for bit to a numpy restatement of this text,
 * tests/denoise_reference.py).
 *
 * An edge-avoiding a-trous filter over the accumulation records: the mean
 * radiance is demodulated by the primary albedo, filtered over P passes of a
 * 5 x 5 B3-spline kernel at strides 1, 2, 4, 8, 16 under four edge stops
 * (primitive, depth, geometric normal, irradiance), remodulated and stored to
 * the framebuffer in use.  The records are only read: accumulation goes on.
 *
 * Per pixel p.  Inputs: the accumulation record {s_R, s_G, s_B, n}, n >= 1;
 * the guide pid, z (the 24-bit depth word) and geom (RT_AOV_GEOM), exactly
 * rt_aov_t's pid and depth_flags of the primary+shadow configuration of the
 * same scene and size; the base colour A (ARGB: the pixel shaded without
 * shadows, the path's starting throughput); the guide normal N, three signed
 * bytes.
 *   Normal: e1, e2 of pid's RT_REC_PTRIS record; n = cross(e1, e2), len =
 *   sqrtf(dot(n, n)), n / len in binary32 (kernels/rt_path.h tri_normal's first
 *   three statements, no facing flip); N_i = (int)rintf(n_i * 127.0f); N = 0
 *   when len is 0 or not finite.  0 for a pixel without geom.
 *   Demodulate (geom pixels), per channel c: d = n * max(A_c, 1), I_c =
 *   min(65535, (256 * s_c + d / 2) / d) in integer division (64 bits).
 *   Pass k = 1..P, stride st = 2^(k-1), geom pixels: taps q = p + st * (i, j),
 *   i, j in -2..2, inside the image and with geom(q); h(i, j) = b_i * b_j, b =
 *   (1, 4, 6, 4, 1); w(p, p) = 256, else w = (wz * wn * wl) >> 16 with
 *     pid_q == pid_p: wz = wn = 256; otherwise
 *     wz = E(|z_p - z_q| >> (zs + k - 1)),
 *     c = min(256, |N_p . N_q| >> 6), wn = (c * c) >> 8, then wn = (wn * wn) >> 8;
 *     wl = E(max_c |I_c(p) - I_c(q)| >> ls) on the pass's input;
 *     E(e) = e >= 9 ? 0 : 256 >> e.
 *   I'_c(p) = (sum h * w * I_c(q) + den / 2) / den, den = sum h * w.  Every sum
 *   fits 32 bits: 256 * 256 * 65535 + 32768 < 2^32.
 *   Store.  A geom pixel: alpha(A) | min(255, (I_c * A_c + 128) >> 8) per
 *   channel; any other pixel: rt_accum_resolve(record, A).
 * Parameters: passes 1..5; depth_shift zs 0..23; color_shift ls 0..16 (16: no
 * irradiance difference reaches 2^16, the irradiance stop is off).
 * RT_DENOISE_DEFAULT_* is what tests/test_gpu_denoise.py's error test runs.
 *
 * rt_denoise_capture_start: one launch (image rt_aov_guide: kernels/
 * rt_aov_kernel.hip built with RT_AOV_BASE=2) writing, per framebuffer pixel,
 * the guide record and the base colour into buffers of its own; it writes
 * neither the framebuffer nor an accumulation record.  Valid on a
 * configuration rt_renderer_accum_begin accepts (before or after that call)
 * with a linear framebuffer: -2 (rt_last_error says why) for everything
 * rt_renderer_accum_begin refuses, for RT_RENDER_COMPACT or shards, for a
 * scene with a non-empty ordered tail.  (rt_render_aov_start stays refused on
 * path frames.)  The guide depends on view and resolution only: it survives
 * rt_renderer_set_light, rt_renderer_set_path_lights, rt_renderer_accum_reset
 * and further accumulation; rt_renderer_configure and rt_renderer_free release
 * it.  An ordinary launch as a record launch is (no lane, behind the frames
 * in flight on both lanes).  The three images (the kernel directory's, else
 * the library's) are loaded by the first call and kept.
 *
 * rt_render_denoise_start: -2 without a capture since the last configure,
 * without an accumulated sample (rt_renderer_accum_samples = 0), or with a
 * parameter out of range.  It queues 1 + passes ordinary launches with no host
 * wait and no copy -- prepare (rt_denoise_prep: demodulate, pack the taps'
 * records), then the passes (rt_denoise_pass), the last of which remodulates
 * and stores -- no launch lane, behind the frames in flight on both lanes;
 * the parameters travel in launch words and tag.  It writes the framebuffer in
 * use, as a relight launch does: rt_read_framebuffer returns the denoised
 * frame, rt_render_wait covers it, rt_render_kernel_ms describes its last
 * launch.  Frames of several path lights are admitted: records and the sample
 * cursor keep their form. */
typedef struct {
  int32_t  pid;          /* rt_aov_t::pid */
  uint32_t depth_flags;  /* rt_aov_t::depth_flags without RT_AOV_SHADOW_RAY: the depth word, RT_AOV_GEOM */
  uint32_t normal;       /* N: signed bytes x | y << 8 | z << 16 (bits 24-31 zero) */
  uint32_t reserved;     /* 0 */
} rt_denoise_guide_t;
typedef struct {
  uint32_t passes;       /* 1..5 */
  uint32_t depth_shift;  /* zs, 0..23 */
  uint32_t color_shift;  /* ls, 0..16 */
} rt_denoise_params_t;
#define RT_DENOISE_DEFAULT_PASSES 2u
#define RT_DENOISE_DEFAULT_DEPTH_SHIFT 2u
#define RT_DENOISE_DEFAULT_COLOR_SHIFT 3u
int rt_denoise_capture_start(rt_renderer_h r);
int rt_denoise_capture(rt_renderer_h r);    /* start + wait */
int rt_render_denoise_start(rt_renderer_h r, const rt_denoise_params_t* params);
int rt_render_denoise(rt_renderer_h r, const rt_denoise_params_t* params);  /* start + wait */
/* the capture's guide records and base colours in framebuffer order (either may be NULL), count >=
 * the framebuffer's pixels (waits for the device).  NO REFERENCE. */
int rt_read_denoise_guide(rt_renderer_h r, rt_denoise_guide_t* guide, uint32_t* base, uint64_t count);
/* Restore an accumulation, for checkpoint and resume: rec = uint32[count][4] in framebuffer order
 * as rt_read_accum returns them, count >= the framebuffer's pixels; every record's n must equal
 * `n` in 1..2^24, else -2.  Sets the sample cursor to n: the next accumulation launch continues
 * with sample n and does not reset.  After rt_renderer_accum_begin only; waits for the device.
 * NO REFERENCE. */
int rt_write_accum(rt_renderer_h r, const uint32_t* rec, uint64_t count, uint32_t n);

/* Ambient occlusion on the device from a frame's visibility records.  NO
 * REFERENCE (the definition below composes the path tracer's own pinned
 * routines; tests/ao_reference.py restates it from the oracle's primitives and
 * the device is held to that bit for bit).
 *
 * Framebuffer.  Linear W x H only; pixel p = y * W + x; rec[p] is the rt_aov_t
 * the last rt_render_aov / rt_relight_capture since rt_renderer_configure
 * wrote.
 * Ray pixel.  (depth_flags & RT_AOV_GEOM) and t > 0 && t < +inf.  This does not
 * depend on RT_RENDER_SHADOWS (RT_AOV_SHADOW_RAY is not read).
 * A ray pixel's rays -- the path tracer's first vertex, op for op, in binary32:
 *   d = the pixel's primary direction ((x + 0.5) * 2 / W - 1, (y + 0.5) * 2 / H
 *   - 1, 1); P = d * (t * 0.999755859375f); n = tri_normal(e1, e2 of pid's
 *   RT_REC_PTRIS record, d) (kernels/rt_path.h); sample c -- the 0-based cursor
 *   since rt_renderer_ao_begin or rt_renderer_ao_reset -- has direction
 *   bounce_dir(n, pt_key(seed + c mod 2^32, p, 0)).  The sample is occluded iff
 *   some geometry triangle other than pid meets the ray (Moeller-Trumbore as the
 *   frames' rays, tmin = 0) at t < radius; radius is a positive float or +inf.
 *   The verdict does not depend on traversal order.
 * Record.  One uint32 per framebuffer pixel: the occluded samples so far; 0 for
 * a pixel that is not a ray pixel.  N, the sample cursor, is the renderer's.
 * Resolve.  rt_ao_resolve(argb, o, N) keeps the alpha byte and returns per
 * colour channel c (2 * c * (N - o) + N) / (2 * N) in integer division; argb
 * when N = 0.  N <= 65535.
 *
 * rt_renderer_ao_begin(r, params): valid where rt_render_aov_start is, with a
 * linear framebuffer and after a record launch: -2 (rt_last_error says why) for
 * everything rt_render_aov_start refuses, for RT_RENDER_COMPACT or shards, when
 * no record launch ran since the last configure, for a radius that is NaN or
 * not positive.  It allocates the count buffer (W * H * 4 B; rt_renderer_
 * configure and rt_renderer_free release it and end the session) and loads
 * rt_ao.vxbin and rt_ao_resolve.vxbin (the kernel directory's, else the
 * library's) on the first call; the next tracing launch resets.
 * rt_renderer_ao_reset: the cursor back to 0, the next launch resets -- no
 * clearing launch and no copy, the reset travels in the launch words.
 * rt_renderer_set_light / rt_renderer_set_lights do not end the session: pid
 * and t do not depend on lights.
 *
 * rt_render_ao_start(r, samples): one launch of rt_ao (kernels/
 * rt_ao_kernel.hip) tracing samples = 1..64 rays per ray pixel, with no host
 * wait and no copy; -2 for samples out of range or a cursor that would pass
 * 65535.  An ordinary launch as a record launch is: no lane, behind the frames
 * in flight.  It writes only the counts -- neither the framebuffer nor the
 * visibility records -- rt_render_wait covers it, and with RT_RENDER_COUNTERS
 * rt_render_stats after it gives shadow_rays = the rays traced and occluded =
 * the sum of their verdicts (every other counter 0).
 *
 * rt_render_ao_resolve_start(r, mode, weights, n): one launch of rt_ao_resolve
 * (kernels/rt_ao_resolve_kernel.hip), a streaming pass into the framebuffer in
 * use, as a relight launch goes.  RT_AO_GREY writes rt_ao_resolve(0xffffffff,
 * o, N); weights and n are ignored.  RT_AO_MODULATE writes rt_ao_resolve(
 * rt_relight_resolve(base, depth_flags, light_mask, weights, n), o, N), the
 * relit pixel times the ambient term; with weights NULL the colour is the base
 * colour itself.  -2 for N = 0, for an unknown mode, for RT_AO_MODULATE without
 * a live relight capture (rt_render_relight_start's rule), with n not the
 * capture's light count or with every weight 0. */
typedef struct {
  float    radius;   /* > 0, or +inf */
  uint32_t seed;     /* sample c is keyed by seed + c */
} rt_ao_params_t;
#define RT_AO_DEFAULT_SEED 0x5EEDu   /* rtapp -K's, and the Python layer's default */
#define RT_AO_GREY 0u
#define RT_AO_MODULATE 1u
int rt_renderer_ao_begin(rt_renderer_h r, const rt_ao_params_t* params);
int rt_renderer_ao_reset(rt_renderer_h r);
int rt_render_ao_start(rt_renderer_h r, uint32_t samples);
int rt_render_ao(rt_renderer_h r, uint32_t samples);            /* start + wait */
int rt_renderer_ao_samples(rt_renderer_h r, uint32_t* n);       /* the sample cursor N */
/* the counts in framebuffer order, count >= the framebuffer's pixels (waits for the device) */
int rt_read_ao(rt_renderer_h r, uint32_t* out, uint64_t count);
int rt_render_ao_resolve_start(rt_renderer_h r, uint32_t mode, const uint8_t* weights, uint32_t n);
int rt_render_ao_resolve(rt_renderer_h r, uint32_t mode, const uint8_t* weights, uint32_t n);  /* start + wait */
/* the resolved pixel restated on the host (occluded above n counts as n) */
uint32_t rt_ao_resolve(uint32_t argb, uint32_t occluded, uint32_t n);

/* Caller-supplied rays against the scene's tree: closest-hit and any-hit
 * queries, batched, on the device.  NO REFERENCE (the walks are rt_trace.h's
 * trace<false> / trace<true>, which tests/test_gpu_ray_kat.py holds to the exact
 * model; tests/test_gpu_query.py holds this entry point to the same answers).
 *
 * Space.  Rays are in the space the scene is traced in: clip (x, y, w), the eye
 * at the origin -- rt_renderer_set_light's space, and the space of the
 * triangles' corners.  pid is the scene's primitive index, the visibility
 * records' pid.  Only geometry primitives (depth-tested drawcalls: the tree's
 * triangles) can be hit.
 *
 * RT_QUERY_CLOSEST.  Of the triangles k != skip that Moeller-Trumbore (mt_hit,
 * inclusive coverage on the edges) meets at tmin < t < tmax, both strict -- the
 * limits as trace<false> applies them: mt_hit's t > tmin, and a best hit that
 * starts at tmax and is replaced by t < best -- the one with the smallest t; at
 * equal t the lowest pid (tie_high = false).  t is mt_hit's value, bit for bit.
 * RT_QUERY_ANY.  A miss iff no such triangle exists; else
 * the pid and t of the occluder the fixed-order any-hit walk (trace<true>)
 * finds first: deterministic for a given tree, but not the closest -- the
 * caller may rely on pid >= 0 only.
 * A miss is {-1, 0.0f}.
 * Malformed rays.  A ray is a miss, and walks nothing, when its direction is
 * all zero (+-0), when any of its 8 words is NaN, or when its origin or its
 * direction has an infinite component.  tmax = +inf is admitted.  The other
 * lanes of its wave are not affected.
 * skip.  One int32 per ray, -1 for none: the primitive the ray does not meet
 * (the frames' own secondary rays avoid their origin's triangle this way).
 * Without RT_QUERY_SKIP the buffer is not read and no ray skips.
 * RT_QUERY_PERM.  Slot q of the launch traces ray perm[q] and stores its hit
 * at hits[perm[q]]: results stay at the rays' own indices, only the assignment
 * of rays to waves changes (a wave takes 64 consecutive slots).  perm must be a
 * permutation of [0, n); a slot whose entry is >= n traces and stores nothing.
 *
 * The coherence key of a ray, a uint32 (rt_query_key; every operation is one
 * binary32 operation, in the order written, none fused):
 *   malformed ray: 0xFFFFFFFF.
 *   bits 31, 30, 29: the sign bits of d.x, d.y, d.z (the words' bit 31).
 *   bits 28..8: the 21-bit Morton code of the origin's cell, 128 cells per axis
 *     over box = {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z}, axis a's 7 bits c_a at
 *     key bits 8 + a + 3 i (x lowest):
 *       inv_a = hi_a > lo_a ? 128.0f / (hi_a - lo_a) : 0.0f   (once, on the host)
 *       c_a = (uint32_t)fminf(fmaxf((o_a - lo_a) * inv_a, 0.0f), 127.0f)
 *     (fmaxf of a NaN and 0 is 0: an overflowing difference on a flat axis).
 *   bits 7..4 / 3..0: the direction's cell, with s = (|d.x| + |d.y|) + |d.z|:
 *       (uint32_t)fminf((|d.y| / s) * 16.0f, 15.0f)  /  the same of |d.x|.
 * The launches' box is the bounding box of the geometry triangles' corners
 * (rt_query_buffers_t::box; all zero for a scene without geometry), which the
 * tree's root box encloses.
 *
 * rt_query_reserve(r, max_rays): one arena allocation of 52 B per ray -- rays,
 * hits, skip words, permutation, keys -- for max_rays = 1 .. 2^24 rays, and its
 * addresses into the argument block in stream order.  The renderer must be
 * configured (the kernels read the scene through its argument block); the
 * reserve then survives rt_renderer_configure, rt_renderer_set_light and
 * rt_renderer_set_lights, until the next reserve or rt_renderer_free.  -2 when
 * the arena cannot hold the buffers (the old reserve is kept), when max_rays
 * is out of range, or when launches using a previous reserve were started and
 * not waited for (rt_render_wait).  Loads rt_query.vxbin and
 * rt_query_keys.vxbin (the kernel directory's, else the library's) on the
 * first call.  The buffers' contents are undefined until written.
 * rt_query_buffers: the true device pointers, as rt_framebuffer_device gives
 * the framebuffer's, for code on the renderer's stream (rt_device_stream):
 * ordinary launches -- the query launches among them -- run on that stream.
 * rt_query_write_*: host uploads in stream order behind the queued launches
 * (copies above the driver's staging slot wait for the device first); first +
 * n <= the capacity.
 * rt_query_trace_start(r, n, mode, flags): one launch of rt_query (kernels/
 * rt_query_kernel.hip) over rays [0, n) -- under RT_QUERY_PERM over slots [0, n)
 * -- with no host wait and no copy; rt_render_wait covers it.  It writes
 * hits [0, n) only: no framebuffer, no record buffer, no counter.  Any frame
 * kind may be configured as long as the tree is the binary16 BVH4 (a scene
 * without geometry: every ray a miss).  -2: not configured, no reserve, n = 0
 * or above the capacity, an unknown mode or flag, a tree of another layout, a
 * driver without launch words.
 * rt_query_keys_start(r, n): one launch of rt_query_keys (kernels/
 * rt_query_keys_kernel.hip) writing keys [0, n): 32 B in, 4 B out per ray,
 * nothing traced.  Sorting is the caller's: a stable sort of the keys gives the
 * permutation for RT_QUERY_PERM.
 * rt_query_read_*: wait for the device, then copy out. */
typedef struct { float o[3], tmin, d[3], tmax; } rt_ray_t;   /* 32 B */
typedef struct { int32_t pid; float t; } rt_hit_t;           /* 8 B; a miss is {-1, 0.0f} */
#define RT_QUERY_CLOSEST 0u
#define RT_QUERY_ANY 1u
#define RT_QUERY_SKIP 0x1u   /* flags: read the skip buffer */
#define RT_QUERY_PERM 0x2u   /* flags: slot q traces ray perm[q] */
#define RT_QUERY_MAX_RAYS (1u << 24)
typedef struct {
  void*    rays;      /* rt_ray_t [capacity] */
  void*    hits;      /* rt_hit_t [capacity] */
  void*    skip;      /* int32_t  [capacity] */
  void*    perm;      /* uint32_t [capacity] */
  void*    keys;      /* uint32_t [capacity] */
  uint64_t capacity;  /* rays */
  float    box[6];    /* the key grid's box: lo.xyz, hi.xyz */
} rt_query_buffers_t;
int rt_query_reserve(rt_renderer_h r, uint64_t max_rays);
int rt_query_buffers(rt_renderer_h r, rt_query_buffers_t* out);
int rt_query_write_rays(rt_renderer_h r, const rt_ray_t* rays, uint64_t first, uint64_t n);
int rt_query_write_skip(rt_renderer_h r, const int32_t* skip, uint64_t first, uint64_t n);
int rt_query_write_perm(rt_renderer_h r, const uint32_t* perm, uint64_t first, uint64_t n);
int rt_query_trace_start(rt_renderer_h r, uint64_t n, uint32_t mode, uint32_t flags);
int rt_query_trace(rt_renderer_h r, uint64_t n, uint32_t mode, uint32_t flags);   /* start + wait */
int rt_query_keys_start(rt_renderer_h r, uint64_t n);
int rt_query_keys(rt_renderer_h r, uint64_t n);                                   /* start + wait */
int rt_query_read_hits(rt_renderer_h r, rt_hit_t* out, uint64_t first, uint64_t n);
int rt_query_read_keys(rt_renderer_h r, uint32_t* out, uint64_t first, uint64_t n);
/* a ray's key restated on the host */
uint32_t rt_query_key(const rt_ray_t* ray, const float box[6]);

/* Soft shadows from area lights, sampled on the device from a frame's
 * visibility records.  NO REFERENCE (the definition below composes routines
 * that are pinned already; tests/soft_reference.py restates it from the
 * oracle's primitives and the device is held to that bit for bit).
 *
 * Framebuffer, pixel index p, rec[p] and "ray pixel" are the ambient-occlusion
 * block's above: linear W x H only; (depth_flags & RT_AOV_GEOM) and t > 0 && t
 * < +inf; RT_AOV_SHADOW_RAY is not read.
 * Lights.  The n lights in use when the session begins, by the relight
 * capture's rule: 1 after rt_renderer_configure or rt_renderer_set_light, k
 * after rt_renderer_set_lights.  Light i has its position L_i and a radius R_i,
 * a finite float >= 0.
 * A ray pixel's sample c -- the 0-based cursor since rt_renderer_soft_begin or
 * rt_renderer_soft_reset -- has one ray per light i, computed in binary32,
 * every operation a single one in the order written, fused only where fmaf is
 * written:
 *   1. P = d * (t * 0.999755859375f), d the pixel's primary direction (the
 *      ambient-occlusion block's P, the frames' shadow origin);
 *   2. m_k = P_k - L_i,k;
 *   3. len = sqrtf(dot3(m, m)) (dot3 as kernels/rt_trace.h: fmaf(m2, m2,
 *      fmaf(m1, m1, m0 * m0)));
 *   4. if len is 0 or not finite the sample is not occluded and walks nothing;
 *   5. m_k = m_k / len;
 *   6. u = bounce_dir(m, pt_key(seed + c mod 2^32, p, 64 + i)) (kernels/
 *      rt_path.h; the oracle's pt_bounce_dir): a cosine-weighted point of the
 *      unit hemisphere about m -- the side of the light's sphere that faces P,
 *      uniform over its projected disc.  Vertex index 64 + i keeps these
 *      streams apart from the path tracer's and ambient occlusion's;
 *   7. target_k = fmaf(R_i, u_k, L_i,k);
 *   8. the ray has origin P and direction target - P; it is occluded iff some
 *      geometry triangle other than pid meets it (Moeller-Trumbore as the
 *      frames' rays) at 0 < t < 1.  The verdict does not depend on traversal
 *      order.
 * With R_i = 0 the target is L_i exactly, and every sample's verdict is the
 * frame's own hard-shadow verdict for that light (the record's light_mask bit).
 * Record.  One uint16 per (light, pixel), stored as planes: index i * W * H + p;
 * the occluded samples so far, 0 for a pixel that is not a ray pixel.  N, the
 * sample cursor, is the renderer's, and N <= 1024.
 * Resolve.  rt_soft_resolve(base_argb, depth_flags, counts[n], N, weights[n],
 * n): w_i in 0..255, D = N * sum w_i, O = sum w_i * o_i with o_i clamped to N.
 * A pixel with RT_AOV_GEOM (a ray pixel's counts; any other pixel's are 0) is
 * per colour channel c of the base colour (2 * ((D - O) * c + O * (c >> 1)) +
 * D) / (2 * D) in integer division, under the base colour's alpha byte; any
 * other pixel is its base colour.  base_argb is returned unchanged when N = 0,
 * N > 1024, n is outside 1..RT_MAX_LIGHTS or sum w_i = 0.
 *   - N <= 1024 keeps the numerator, at most 2 * 255 * D + D = 511 * D <= 511 *
 *     1024 * (16 * 255 = 4080) = 2 134 917 120, below 2^32: uint32 arithmetic
 *     suffices on the host and on the device.
 *   - When every o_i is 0 or N, O = N * O' with O' the sum of the weights of
 *     the lights at N, and D = N * W: numerator 2 * N * ((W - O') * c + O' * (c
 *     >> 1)) + N * W and denominator 2 * N * W both carry the factor N, so the
 *     value is rt_relight_resolve's under the mask of the lights at N.
 *
 * rt_renderer_soft_begin(r, params): valid where rt_renderer_ao_begin is, with
 * its refusals (-2, rt_last_error says why), and refused too when n is not the
 * count of lights in use, when a radius is NaN, negative or infinite, or when
 * the arena cannot hold the planes' n * W * H * 2 B; a refused begin changes
 * nothing: a session already begun goes on.  It allocates the planes
 * (rt_renderer_configure and rt_renderer_free release them and end the
 * session), loads rt_soft.vxbin and rt_soft_resolve.vxbin (the kernel
 * directory's, else the library's) on the first call, and writes the launch's
 * argument area -- planes, radii, the lights' positions -- in stream order; the
 * next tracing launch resets.  rt_renderer_set_light, rt_renderer_set_lights
 * and rt_renderer_set_path_lights end the session, unlike an ambient-occlusion
 * session: the counts describe other lights.
 * rt_renderer_soft_reset: the cursor back to 0, the next launch resets -- no
 * clearing launch and no copy, the reset travels in the launch words.
 *
 * rt_render_soft_start(r, samples): one launch of rt_soft (kernels/
 * rt_soft_kernel.hip) tracing samples = 1..64 rays per ray pixel and light,
 * with no host wait and no copy; -2 for samples out of range or a cursor that
 * would pass 1024.  An ordinary launch as an ambient-occlusion launch is.  It
 * writes only the planes; with RT_RENDER_COUNTERS rt_render_stats after it
 * gives shadow_rays = the rays traced and occluded = the sum of their verdicts
 * (every other counter 0).
 *
 * rt_render_soft_resolve_start(r, mode, weights, n): one launch of
 * rt_soft_resolve (kernels/rt_soft_resolve_kernel.hip), a streaming pass into
 * the framebuffer in use, as a relight launch goes.  RT_SOFT_LIT needs a live
 * relight capture (rt_render_relight_start's rule) and writes rt_soft_resolve(
 * base, depth_flags, counts, N, weights, n); weights NULL means unit weights.
 * RT_SOFT_GREY takes base 0xffffffff and unit weights and needs no capture.  -2
 * for N = 0, an unknown mode, n not the session's count (with weights), every
 * weight 0. */
typedef struct {
  const float* radii;   /* n radii, each finite and >= 0 */
  uint32_t n;           /* the lights in use */
  uint32_t seed;        /* sample c is keyed by seed + c */
} rt_soft_params_t;
#define RT_SOFT_DEFAULT_SEED 0x5EEDu   /* rtapp -E's, and the Python layer's default */
#define RT_SOFT_LIT 0u
#define RT_SOFT_GREY 1u
int rt_renderer_soft_begin(rt_renderer_h r, const rt_soft_params_t* params);
int rt_renderer_soft_reset(rt_renderer_h r);
int rt_render_soft_start(rt_renderer_h r, uint32_t samples);
int rt_render_soft(rt_renderer_h r, uint32_t samples);            /* start + wait */
int rt_renderer_soft_samples(rt_renderer_h r, uint32_t* n);       /* the sample cursor N */
/* the planes, light-major in framebuffer order, count >= lights * the framebuffer's pixels (waits for the device) */
int rt_read_soft(rt_renderer_h r, uint16_t* out, uint64_t count);
int rt_render_soft_resolve_start(rt_renderer_h r, uint32_t mode, const uint8_t* weights, uint32_t n);
int rt_render_soft_resolve(rt_renderer_h r, uint32_t mode, const uint8_t* weights, uint32_t n);  /* start + wait */
/* the resolved pixel restated on the host */
uint32_t rt_soft_resolve(uint32_t base_argb, uint32_t depth_flags, const uint16_t* counts, uint32_t N,
                         const uint8_t* weights, uint32_t n);

/* Read back one per-resolution record array of the current configuration
 * (layouts: kernels/rt_common.h; NO REFERENCE).  out NULL = size query
 * (*size = bytes). */
#define RT_REC_PRIMS 0u     /* rt_prim_t per primitive (128 B) */
#define RT_REC_BBOX 1u      /* rt_bbox_t per primitive (raster mode or device setup) */
#define RT_REC_VIS 2u       /* uint32[4] per primitive: rectangle x, y, depth bound, any */
#define RT_REC_VNODES 3u    /* rt_vnode_t per node of the primary rays' tree */
#define RT_REC_VTRIS 4u     /* rt_vtri_t per leaf record (+3 pads) */
#define RT_REC_VLAYERS 5u   /* rt_vtri_t per screen layer, last drawn first */
#define RT_REC_VGEOM 6u     /* rt_vtri_t per geometry primitive, ascending pid */
#define RT_REC_ORDER 7u     /* u32 per local tile: the work order */
#define RT_REC_PTRIS 8u     /* rt_tri_t per primitive (clip v0 + pid, e1, e2) */
#define RT_REC_GEOM 9u      /* rt_tri_t per geometry primitive */
#define RT_REC_BIDX 10u     /* uint32[2] per local 8x8 block: first list entry, count */
#define RT_REC_BLIST 11u    /* rt_bentry_t per list entry (+3 padding entries, RT_BLIST_PAD) */
#define RT_REC_SIDX 12u     /* uint32[2] per light-space cell: first entry, count */
#define RT_REC_SLIST 13u    /* rt_tri_t per light-space list entry (+1 padding record) */
#define RT_REC_CDESC 14u    /* rt_cdesc_t per chunk of the whole-block tier, as the device setup built it */
#define RT_REC_CDESC_HOST 15u /* the same table restated on the host from the work order and list headers */
#define RT_REC_OIDX 16u     /* ordered tail: uint32[2] per local 8x8 block: first list entry, count */
#define RT_REC_OLIST 17u    /* ordered tail: u32 primitive index per entry (+2 padding entries, RT_OLIST_PAD) */
#define RT_REC_BGLAYER 18u  /* background tier: uint32[2] per chunk from the first background chunk on, in work
                             * order, as the device setup built it: pid + 1 of the one screen layer covering the
                             * chunk's 8x8 block (0xffffffff: none, 0: mixed or off the image), its drawcall */
#define RT_REC_BTIDX 20u    /* the trimmed block lists' headers: uint32[2] per local 8x8 block -- RT_REC_BIDX's
                             * first entry, the kept count */
#define RT_REC_BTRIM 21u    /* the trimmed block lists (RT_REC_BLIST's shape): per block the entries whose
                             * primitive wins a pixel of the block, moved to the front of the list's slots */
#define RT_REC_BTIDX_HOST 22u /* the same two arrays restated on the host from the device's untrimmed lists */
#define RT_REC_BTRIM_HOST 23u
#define RT_REC_BGLAYER_HOST 19u /* the same table restated on the host from the work order and the layer records */
int rt_renderer_export_records(rt_renderer_h r, uint32_t which, void* out, uint64_t bytes,
                               uint64_t* size);

/* raw per-workgroup counter rows of the last launch (16 u32 each; the
 * RT_STAMPS diagnostic images put wave timestamps in slots 12-15) */
int rt_launch_rows(rt_renderer_h r, uint32_t* rows, uint64_t max_rows, uint64_t* nrows);

/* Multi-GPU frame exchange for C hosts (include/rt_shard.h, librt_shard.so,
 * RCCL): after rt_render, gather every rank's compact tile buffer to rank 0
 * and assemble the frame there, on the renderer's stream; rank 0 copies it
 * to `image` (W*H ARGB8888, row 0 = NDC y = -1) when not NULL.  The
 * renderer must be configured with shard_index / shard_count = the
 * communicator's rank / size.  Collective.  NO REFERENCE. */
struct rt_shard_comm;
int rt_render_gather(rt_renderer_h r, struct rt_shard_comm* comm, uint32_t* image);

/* device pointer + byte size of the output buffer (for RCCL gathers) and the
 * HIP stream the kernel runs on (for stream-ordered consumers).  The pointer
 * names the last started frame's buffer; from this call to the next
 * configure every frame renders into that one buffer on lane 0, the stream
 * rt_device_stream returns (no frame overlap, rt_render_start). */
int rt_framebuffer_device(rt_renderer_h r, void** device_ptr, uint64_t* bytes);
int rt_device_stream(rt_renderer_h r, void** hip_stream);
int rt_device_caps(rt_renderer_h r, uint64_t caps[8]);

#ifdef __cplusplus
}
#endif

#endif /* VX_RT_H */
