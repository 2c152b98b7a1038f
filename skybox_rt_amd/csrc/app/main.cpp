// main.cpp -- rtapp (and, built with -DRT_APP_RASTER, rasterapp): the
// command-line regression apps over librtapp.so.
//
// rtapp takes draw3d's command line unchanged (tests/regression/draw3d/
// main.cpp:80-135): -t trace, -s/-e first/last drawcall drawn, -o output,
// -r reference (tolerance-1 compare, "PASSED!"/"FAILED! N errors."), -w/-h
// size, -k tile log size (binning granularity), -u/-x/-y software texture /
// raster / OM switches and -z (accepted; one pipeline serves both here, so
// the output is the same), -? usage.  Files resolve like ResolveFilePath
// (gfxutil.cpp:348-363): as given, else in each directory of the
// comma-separated RT_ASSETS_PATHS (the reference compiles its source
// directory in as ASSETS_PATHS), a scene also as <name>.gz.  The kernel images
// come from the library directory, or from env RT_KERNEL_DIR.
//
// Mode: primary rays by default (raster-exact, draw3d's own output); a scene
// the RT path does not support (blending, stencil, partial colour writes,
// mixed depth functions: DESIGN.md "Scope") and any -k other than the
// RASTER_TILE_LOGSIZE 5 the RT path bins at render through the draw3d raster
// pipeline instead, which is what draw3d itself runs.  Extensions: -S shadow
// rays, -L x,y,w light, -M x,y,w one more light (repeatable: with -S the
// frame is lit by the light of -L and every -M, rt_renderer_set_lights; with -P and no -S the path frame is,
// rt_renderer_set_path_lights, also under -A), -P N path tracing with N bounces, -F flat triangle
// list, -R raster pipeline, -n N repeat launches, -B lbvh|sah device BVH
// build, -H host-loop setup, -O load the scene with RT_SCENE_OM_LAYERS (a
// scene the RT path cannot trace as a whole renders on the RT path all the
// same: its head traced, its ordered tail folded through the output merger,
// vx_rt.h); -A samples, with -P: that many samples per pixel accumulated on
// the device (rt_render_accumulate: launches of 32, then one for the rest)
// and their mean written, -r comparing as usual; -D passes[,zs,ls], with -A:
// after the samples a guide capture (rt_denoise_capture) and the edge-avoiding
// filter over the records (rt_render_denoise: passes 1..5, depth shift zs and
// irradiance shift ls, by default RT_DENOISE_DEFAULT_*), whose frame is the one
// written to -o, and one line "Denoise: <passes> passes, zs <zs>, ls <ls>, capture <ms> ms, filter <ms> ms host wall";
// -V file: after the frame one
// visibility-record launch (rt_render_aov) of the same configuration and
// lights, written as a 16-byte header ('RTAV', width, height, 16) and the
// rt_aov_t records in framebuffer order (with -G: this rank's compact tiles),
// and one line "AOV: <geometry pixels> geometry, <shadow rays> shadow rays,
// <occluded> occluded"; -W w0,w1,...: with -S, one weight 0..255 per light of
// -L / -M -- after the frame a relight capture (rt_relight_capture) and one
// relight launch under the weights (rt_render_relight), whose frame is the one
// written to -o, and one line "Relight: <n> lights, weights w0,w1,...";
// -K samples[,radius]: with -S, after the frame a relight capture and that many
// ambient-occlusion samples per ray pixel (rt_render_ao: launches of 64, then
// one for the rest; rays of at most `radius`, by default unbounded; seed
// RT_AO_DEFAULT_SEED), then the modulate resolve (rt_render_ao_resolve) under
// -W's weights, or unit weights -- the relit frame times the ambient term,
// written to -o -- and one line "AO: <samples> samples, radius <r>";
// -E samples[,radius]: with -S, after the frame a relight capture and that many
// soft-shadow samples per ray pixel and light of -L / -M (rt_render_soft:
// launches of 64, then one for the rest; every light a sphere of `radius`, by
// default 1; seed RT_SOFT_DEFAULT_SEED), then the lit resolve
// (rt_render_soft_resolve) under -W's weights, or unit weights -- the frame
// with penumbrae, written to -o -- and one line "Soft: <samples> samples,
// radius <r>" (not with -K);
// multi-GPU (one process per GPU over
// librt_shard.so / RCCL): -G rank,ranks -I idfile -- this process renders
// 32x32 tiles t with t % ranks == rank, rank 0 writes the RCCL communicator
// id to `idfile` (the others wait for it), every frame ends with
// rt_render_gather to rank 0, which writes / checks the assembled frame.
//
// rasterapp takes the raster regression app's command line
// (tests/regression/raster/main.cpp:66-107: -t -o -r -w -h -k -z) and writes
// its coverage image (covered pixels white over 0xff000000, raster/
// kernel.cpp:35-45) through the raster pipeline.
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include <array>

#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <thread>

#include "assets.h"
#include "png.h"
#include "rt_shard.h"
#include "vx_rt.h"

namespace {

const char* trace_file = "triangle.cgltrace";
const char* output_file = "output.png";
const char* reference_file = nullptr;
uint32_t width = 128, height = 128, repeat = 1;
uint32_t start_draw = 0, end_draw = 0xffffffffu;
int tile_log = -1;  // -k (-1: RASTER_TILE_LOGSIZE)
bool shadows = false, raster = false, flat = false;
int bounces = -1;  // >= 0: path tracing
float light[3] = {0.0f, 60.0f, 80.0f};
int rank = -1, ranks = 1;            // -G rank,ranks
const char* id_file = "rt_shard.id";  // -I
const char* build = nullptr;          // -B lbvh|sah: build the BVH on the device
bool host_setup = false;              // -H: per-resolution records by the host loops
bool om_layers = false;               // -O: RT_SCENE_OM_LAYERS
uint32_t accum_samples = 0;           // -A: with -P, accumulate this many samples per pixel
std::vector<std::array<float, 3>> more_lights;  // -M: lights beside the one of -L
const char* aov_file = nullptr;       // -V: write the frame's visibility records
const char* weights_arg = nullptr;    // -W: relight the frame under these per-light weights
const char* denoise_arg = nullptr;    // -D: with -A, denoise the accumulated frame
const char* ao_arg = nullptr;         // -K: with -S, the frame times its ambient occlusion
const char* soft_arg = nullptr;       // -E: with -S, the frame under area lights

#ifdef RT_APP_RASTER
const char* kOpts = "t:i:o:r:w:h:k:n:z?";
void usage() {
  std::printf("Vortex rasterizer Test.\n"
              "Usage: [-t trace] [-o output] [-r reference] [-w width] [-h height] [-z no_hw] "
              "[-k tilelogsize] [-n repeat]\n");
}
#else
const char* kOpts = "t:s:e:i:o:r:w:h:k:n:L:M:P:G:I:B:A:V:W:D:K:E:uxyzSRFHO?";
void usage() {
  std::printf("Vortex 3D Rendering Test (MI355X).\n"
              "Usage: [-t trace] [-s startdraw] [-e enddraw] [-o output] [-r reference] [-w width] "
              "[-h height] [-x s/w rast] [-y s/w om] [-u s/w tex] [-k tilelogsize]\n"
              "       [-S shadows] [-L x,y,w] [-M x,y,w one more light, repeatable: with -S or -P] [-n repeat] [-R raster | -P bounces | -F flat] "
              "[-G rank,ranks [-I idfile]] [-B lbvh|sah device BVH build] [-H host setup]\n"
              "       [-O trace the head, fold blended / stencil / masked drawcalls (RT_SCENE_OM_LAYERS)]\n"
              "       [-A samples: with -P, accumulate that many samples per pixel on the device and "
              "write their mean]\n"
              "       [-D passes[,zs,ls]: with -A, write the accumulated frame through the edge-avoiding filter]\n"
              "       [-V file: the frame's per-pixel visibility records (primary + shadow frames)]\n"
              "       [-W w0,w1,...: with -S, relight the frame under one weight 0..255 per light of -L / -M]\n"
              "       [-K samples[,radius]: with -S, the relit frame times that many samples of ambient occlusion]\n"
              "       [-E samples[,radius]: with -S, the frame's shadows from that many samples of lights of that radius]\n"
              "       env RT_KERNEL_DIR: kernel images; RT_ASSETS_PATHS: search directories\n");
}
#endif

#define RT_CHECK(_expr)                                                       \
  do {                                                                        \
    int _ret = (_expr);                                                       \
    if (_ret == 0) break;                                                     \
    std::printf("Error: '%s' returned %d! (%s)\n", #_expr, _ret, rt_last_error()); \
    std::exit(-1);                                                            \
  } while (false)

}  // namespace

int main(int argc, char** argv) {
  int c;
  while ((c = getopt(argc, argv, kOpts)) != -1) {
    switch (c) {
    case 't': trace_file = optarg; break;
    case 'o': output_file = optarg; break;
    case 'r': reference_file = optarg; break;
    case 'w': width = (uint32_t)std::atoi(optarg); break;
    case 'h': height = (uint32_t)std::atoi(optarg); break;
    case 'k': tile_log = std::atoi(optarg); break;
    case 'n': repeat = (uint32_t)std::atoi(optarg); break;
    case 'z': break;  // raster / om: software path -- same output here
#ifndef RT_APP_RASTER
    case 's': start_draw = (uint32_t)std::atoi(optarg); break;
    case 'e': end_draw = (uint32_t)std::atoi(optarg); break;
    case 'u': case 'x': case 'y': break;  // software tex / raster / OM: same output here
    case 'S': shadows = true; break;
    case 'R': raster = true; break;
    case 'F': flat = true; break;
    case 'P': bounces = std::atoi(optarg); break;
    case 'L': std::sscanf(optarg, "%f,%f,%f", &light[0], &light[1], &light[2]); break;
    case 'M': {
      std::array<float, 3> m = {0.0f, 0.0f, 0.0f};
      std::sscanf(optarg, "%f,%f,%f", &m[0], &m[1], &m[2]);
      more_lights.push_back(m);
      break;
    }
    case 'G': std::sscanf(optarg, "%d,%d", &rank, &ranks); break;
    case 'I': id_file = optarg; break;
    case 'B': build = optarg; break;
    case 'H': host_setup = true; break;
    case 'O': om_layers = true; break;
    case 'A': accum_samples = (uint32_t)std::atoi(optarg); break;
    case 'V': aov_file = optarg; break;
    case 'W': weights_arg = optarg; break;
    case 'D': denoise_arg = optarg; break;
    case 'K': ao_arg = optarg; break;
    case 'E': soft_arg = optarg; break;
#endif
    case '?': usage(); return 0;
    default: usage(); return -1;  // -i: in the reference's option string, never handled
    }
  }
  if (std::strcmp(output_file, "null") == 0 && reference_file) {
    std::printf("Error: the output file is missing for reference validation!\n");
    return 1;
  }
#ifdef RT_APP_RASTER
  raster = true;
#endif
  const bool rt_only = shadows || flat || bounces >= 0 || rank >= 0;  // modes only the RT path has
  if (tile_log >= 0 && tile_log != 5 && !raster) {
    if (rt_only) {
      std::printf("Error: -k %d: the ray-tracing modes bin at RASTER_TILE_LOGSIZE 5\n", tile_log);
      return 1;
    }
    std::printf("Tile log size %d: rendering through the draw3d raster pipeline\n", tile_log);
    raster = true;
  }
  // (-S decides when both are given: -M with -S behaves as without -P)
  const bool path_lights = !more_lights.empty() && !shadows && bounces >= 0;
  if (path_lights && more_lights.size() + 1 > RT_MAX_PATH_LIGHTS) {
    std::printf("Error: -M x,y,w with -P bounces: at most %u lights in all\n", RT_MAX_PATH_LIGHTS);
    return 1;
  }
  if (!more_lights.empty() && !path_lights && (!shadows || more_lights.size() + 1 > RT_MAX_LIGHTS)) {
    std::printf("Error: -M x,y,w needs -S (shadow rays, at most %u lights in all) or -P bounces (at most %u)\n",
                RT_MAX_LIGHTS, RT_MAX_PATH_LIGHTS);
    return 1;
  }
  if (accum_samples && (bounces < 0 || rank >= 0)) {
    std::printf("Error: -A samples needs -P bounces (path tracing), one rank\n");
    return 1;
  }
  rt_denoise_params_t dn = {RT_DENOISE_DEFAULT_PASSES, RT_DENOISE_DEFAULT_DEPTH_SHIFT,
                            RT_DENOISE_DEFAULT_COLOR_SHIFT};
  if (denoise_arg) {
    const int got = std::sscanf(denoise_arg, "%u,%u,%u", &dn.passes, &dn.depth_shift, &dn.color_shift);
    if (!accum_samples || (got != 1 && got != 3)) {
      std::printf("Error: -D passes[,zs,ls] needs -P bounces -A samples\n");
      usage();
      return 1;
    }
  }
  std::vector<uint8_t> weights;
  if (weights_arg) {
    bool ok = shadows && rank < 0 && *weights_arg != 0;
    for (const char* q = weights_arg; ok;) {
      char* end = nullptr;
      const long v = std::strtol(q, &end, 10);
      ok = end != q && v >= 0 && v <= 255 && (*end == ',' || *end == 0);
      if (ok) weights.push_back((uint8_t)v);
      if (!ok || *end == 0) break;
      q = end + 1;
    }
    if (!ok || weights.size() != more_lights.size() + 1) {
      std::printf("Error: -W w0,w1,... needs -S, one rank and one weight in 0..255 per light of -L / -M (%zu)\n",
                  more_lights.size() + 1);
      usage();
      return 1;
    }
  }
  uint32_t ao_samples = 0;
  rt_ao_params_t ao{__builtin_inff(), RT_AO_DEFAULT_SEED};
  if (ao_arg) {
    const int got = std::sscanf(ao_arg, "%u,%f", &ao_samples, &ao.radius);
    if (!shadows || rank >= 0 || got < 1 || ao_samples < 1 || ao_samples > 65535u || !(ao.radius > 0.0f)) {
      std::printf("Error: -K samples[,radius] needs -S, one rank, 1..65535 samples and a positive radius\n");
      usage();
      return 1;
    }
  }
  uint32_t soft_samples = 0;
  float soft_radius = 1.0f;
  if (soft_arg) {
    const int got = std::sscanf(soft_arg, "%u,%f", &soft_samples, &soft_radius);
    if (!shadows || rank >= 0 || ao_arg || got < 1 || soft_samples < 1 || soft_samples > 1024u ||
        !(soft_radius >= 0.0f) || soft_radius == __builtin_inff()) {
      std::printf("Error: -E samples[,radius] needs -S, one rank, no -K, 1..1024 samples and a finite radius >= 0\n");
      usage();
      return 1;
    }
  }
  const bool sharded = rank >= 0;
  if (sharded && (ranks < 1 || rank >= ranks || raster)) {
    std::printf("Error: -G rank,ranks needs 0 <= rank < ranks (ray-tracing modes)\n");
    return 1;
  }
  int device = 0;
  rt_shard_comm_h comm = nullptr;
  uint8_t id[RT_SHARD_ID_BYTES] = {};
  if (sharded) {
    // one process per GPU: rank r on device r % (visible devices)
    const int ndev = rt_shard_device_count();
    device = ndev > 0 ? rank % ndev : 0;
    setenv("VX_HIP_DEVICE", std::to_string(device).c_str(), 0);
    device = std::atoi(std::getenv("VX_HIP_DEVICE"));
    if (rank == 0) {  // the communicator id, published atomically
      RT_CHECK(rt_shard_unique_id(id));
      const std::string tmp = std::string(id_file) + ".tmp";
      std::ofstream(tmp, std::ios::binary).write((const char*)id, RT_SHARD_ID_BYTES);
      RT_CHECK(std::rename(tmp.c_str(), id_file));
    } else {
      struct stat sb;
      for (int i = 0; stat(id_file, &sb) != 0 || sb.st_size < RT_SHARD_ID_BYTES; ++i) {
        if (i > 6000) { std::printf("Error: no communicator id in %s\n", id_file); return 1; }
        std::this_thread::sleep_for(std::chrono::milliseconds(10));
      }
      std::ifstream(id_file, std::ios::binary).read((char*)id, RT_SHARD_ID_BYTES);
    }
  }
  const std::string trace = rt::ResolveAsset(trace_file, true);
  rt_scene_h scene = nullptr;
  RT_CHECK(rt_scene_load_ex(trace.c_str(), start_draw, end_draw, om_layers ? RT_SCENE_OM_LAYERS : 0u, &scene));
  rt_scene_info_t info;
  RT_CHECK(rt_scene_info(scene, &info));
  std::printf("CGL Trace: drawcalls=%u, primitives=%u, geometry=%u, layers=%u, textures=%u\n",
              info.num_drawcalls, info.num_prims, info.num_geometry, info.num_layer,
              info.num_textures);
  std::printf("BVH: nodes=%u, leaves=%u, depth=%u, build=%.3f ms (parse %.3f ms)\n",
              info.bvh_nodes, info.bvh_leaves, info.bvh_depth, info.bvh_ms, info.parse_ms);
  if (om_layers) {
    uint32_t first_tail = 0, tail_prims = 0;
    RT_CHECK(rt_scene_om_split(scene, &first_tail, &tail_prims));
    if (tail_prims)
      std::printf("Ordered tail: drawcalls %u-%u (%u primitives) folded over the traced head\n", first_tail,
                  info.num_drawcalls - 1, tail_prims);
  }
  rt_renderer_h r = nullptr;
  RT_CHECK(rt_renderer_create(scene, std::getenv("RT_KERNEL_DIR"), &r));
  if (build) {
    const uint32_t m = std::strcmp(build, "sah") == 0 ? RT_BVH_BUILD_SAH : RT_BVH_BUILD_LBVH;
    rt_bvh_build_stats_t bs;
    RT_CHECK(rt_renderer_build_bvh_ex(r, m, &bs));
    std::printf("Device BVH (%s): nodes=%u, depth=%u, bvh4 nodes=%u, stack4=%u, %u launches, "
                "%.3f ms (kernels %.3f ms)\n", m == RT_BVH_BUILD_SAH ? "sah" : "lbvh", bs.nodes,
                bs.depth, bs.nodes4, bs.stack4, bs.launches, bs.build_ms, bs.kernel_ms);
  }
  rt_render_params_t p;
  std::memset(&p, 0, sizeof(p));
  p.width = width;
  p.height = height;
  p.bounces = bounces >= 0 ? (uint32_t)bounces : 0u;
  p.seed = 0x5EED;
  std::memcpy(p.light, light, sizeof(light));
  p.clear_color = 0xff000000u;
  p.shard_count = 1;
  p.tile_logsize = tile_log >= 0 ? (uint32_t)tile_log : 0u;
  const uint32_t common = RT_RENDER_COUNTERS |  // the CLI prints ray counts
                          (host_setup ? RT_RENDER_HOST_SETUP : 0u);
  p.flags = common | (shadows ? RT_RENDER_SHADOWS : 0u) | (raster ? RT_RENDER_RASTER : 0u) |
            (flat ? RT_RENDER_FLAT : 0u) | (bounces >= 0 ? RT_RENDER_PATH : 0u);
#ifdef RT_APP_RASTER
  p.flags |= RT_RENDER_COVERAGE;
#endif
  if (sharded) {
    p.shard_index = (uint32_t)rank;
    p.shard_count = (uint32_t)ranks;
    p.flags |= RT_RENDER_COMPACT;
    RT_CHECK(rt_shard_comm_init(&comm, id, (uint32_t)rank, (uint32_t)ranks, device));
    uint32_t seen = 0;
    RT_CHECK(rt_shard_comm_info(comm, nullptr, &seen));
    std::printf("Shard: rank %d of %d on device %d (communicator: %u ranks)\n", rank, ranks, device,
                seen);
  }
  int rc = rt_renderer_configure(r, &p);
  if (rc == -2 && !raster && !rt_only) {
    // a scene the RT path does not support: draw3d's own pipeline renders it
    std::printf("RT path: %s; rendering through the draw3d raster pipeline\n", rt_last_error());
    raster = true;
    p.flags = common | RT_RENDER_RASTER;
    rc = rt_renderer_configure(r, &p);
  }
  RT_CHECK(rc);
  rt_setup_stats_t ss;
  RT_CHECK(rt_renderer_setup_stats(r, &ss));
  std::printf("Setup (%s): %.3f ms, configure %.3f ms\n", ss.device ? "device" : "host", ss.setup_ms,
              ss.configure_ms);
  if (!more_lights.empty()) {
    // the light of -L first, then every -M in order
    std::vector<float> ls(light, light + 3);
    for (const auto& m : more_lights) ls.insert(ls.end(), m.begin(), m.end());
    const uint32_t nl = (uint32_t)more_lights.size() + 1u;
    const auto* lp = reinterpret_cast<const float(*)[3]>(ls.data());
    RT_CHECK(path_lights ? rt_renderer_set_path_lights(r, lp, nl) : rt_renderer_set_lights(r, lp, nl));
    std::printf("Lights: %u, traced in one launch\n", nl);
  }
  double total = 0.0;
  rt_stats_t st;
  std::vector<uint32_t> gathered;
  if (sharded && rank == 0) gathered.resize((size_t)width * height);
  if (accum_samples) {
    // progressive path tracing: launches of 32 samples, then one for the rest;
    // the framebuffer holds the mean of all of them
    RT_CHECK(rt_renderer_accum_begin(r));
    rt_stats_t sum;
    std::memset(&sum, 0, sizeof(sum));
    uint32_t launches = 0;
    for (uint32_t left = accum_samples; left > 0; ++launches) {
      const uint32_t k = left < 32u ? left : 32u;
      RT_CHECK(rt_render_accumulate(r, k));
      RT_CHECK(rt_render_stats(r, &st));
      total += st.kernel_ms;
      sum.shadow_rays += st.shadow_rays;
      sum.bounce_rays += st.bounce_rays;
      sum.occluded += st.occluded;
      left -= k;
    }
    st.shadow_rays = sum.shadow_rays;
    st.bounce_rays = sum.bounce_rays;
    st.occluded = sum.occluded;
    std::printf("Accumulated %u samples per pixel in %u launches, %.4f ms in all\n", accum_samples, launches,
                total);
    repeat = 1;  // the line below: the time of all launches, the rays of all samples
    if (denoise_arg) {
      // the guide, then prepare + passes into the framebuffer in use; the sum of the launches' times
      RT_CHECK(rt_denoise_capture(r));
      double ms = 0.0, dms = 0.0;
      RT_CHECK(rt_render_kernel_ms(r, &ms));
      const auto t0 = std::chrono::steady_clock::now();
      RT_CHECK(rt_render_denoise(r, &dn));
      dms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      std::printf("Denoise: %u passes, zs %u, ls %u, capture %.4f ms, filter %.4f ms host wall\n", dn.passes,
                  dn.depth_shift, dn.color_shift, ms, dms);
    }
  }
  for (uint32_t i = 0; !accum_samples && i < repeat; ++i) {
    RT_CHECK(rt_render(r));
    RT_CHECK(rt_render_stats(r, &st));
    total += st.kernel_ms;
    if (sharded) RT_CHECK(rt_render_gather(r, comm, rank == 0 ? gathered.data() : nullptr));
  }
  if (raster) {
    std::printf("Elapsed time: %.4f ms/frame (grid %u x %u), pixels=%llu, fragments=%llu, "
                "%.1f Mpixels/s\n",
                total / repeat, st.grid, st.block, (unsigned long long)st.primary_rays,
                (unsigned long long)st.shaded, (double)st.primary_rays / (total / repeat) * 1e-3);
  } else {
    const double rays = (double)(st.primary_rays + st.shadow_rays + st.bounce_rays);
    std::printf("Elapsed time: %.4f ms/frame (grid %u x %u), rays=%.0f (primary %llu, shadow %llu, "
                "bounce %llu, occluded %llu), %.1f Mrays/s\n",
                total / repeat, st.grid, st.block, rays, (unsigned long long)st.primary_rays,
                (unsigned long long)st.shadow_rays, (unsigned long long)st.bounce_rays,
                (unsigned long long)st.occluded, rays / (total / repeat) * 1e-3);
  }
  if (aov_file) {
    // the visibility records of the frame just rendered: one more launch, its own buffer
    rt_stats_t as;
    RT_CHECK(rt_render_aov(r));
    RT_CHECK(rt_render_stats(r, &as));
    std::vector<rt_aov_t> rec(sharded ? (size_t)as.local_tiles * 1024u : (size_t)width * height);
    RT_CHECK(rt_read_aov(r, rec.data(), rec.size()));
    const uint32_t head[4] = {0x56415452u /* 'RTAV' */, width, height, (uint32_t)sizeof(rt_aov_t)};
    std::ofstream f(aov_file, std::ios::binary);
    f.write((const char*)head, sizeof(head));
    f.write((const char*)rec.data(), (std::streamsize)(rec.size() * sizeof(rt_aov_t)));
    f.close();
    if (!f) {
      std::printf("Error: cannot write %s\n", aov_file);
      return 1;
    }
    std::printf("AOV: %llu geometry, %llu shadow rays, %llu occluded\n", (unsigned long long)as.geometry_hits,
                (unsigned long long)as.shadow_rays, (unsigned long long)as.occluded);
  }
  if (weights_arg) {
    // the frame relit from its records and base colours: the framebuffer written below
    RT_CHECK(rt_relight_capture(r));
    RT_CHECK(rt_render_relight(r, weights.data(), (uint32_t)weights.size()));
    std::string ws;
    for (size_t i = 0; i < weights.size(); ++i) ws += (i ? "," : "") + std::to_string(weights[i]);
    std::printf("Relight: %zu lights, weights %s\n", weights.size(), ws.c_str());
  }
  if (ao_arg) {
    // the relit frame times its ambient term: the framebuffer written below
    if (!weights_arg) {
      weights.assign(more_lights.size() + 1, 1);
      RT_CHECK(rt_relight_capture(r));
    }
    RT_CHECK(rt_renderer_ao_begin(r, &ao));
    for (uint32_t left = ao_samples; left;) {
      const uint32_t k = left < 64u ? left : 64u;
      RT_CHECK(rt_render_ao_start(r, k));
      left -= k;
    }
    RT_CHECK(rt_render_ao_resolve(r, RT_AO_MODULATE, weights.data(), (uint32_t)weights.size()));
    std::printf("AO: %u samples, radius %g\n", ao_samples, (double)ao.radius);
  }
  if (soft_arg) {
    // the frame under area lights: the framebuffer written below
    if (!weights_arg) {
      weights.assign(more_lights.size() + 1, 1);
      RT_CHECK(rt_relight_capture(r));
    }
    const std::vector<float> radii(weights.size(), soft_radius);
    const rt_soft_params_t sp{radii.data(), (uint32_t)radii.size(), RT_SOFT_DEFAULT_SEED};
    RT_CHECK(rt_renderer_soft_begin(r, &sp));
    for (uint32_t left = soft_samples; left;) {
      const uint32_t k = left < 64u ? left : 64u;
      RT_CHECK(rt_render_soft_start(r, k));
      left -= k;
    }
    RT_CHECK(rt_render_soft_resolve(r, RT_SOFT_LIT, weights.data(), (uint32_t)weights.size()));
    std::printf("Soft: %u samples, radius %g\n", soft_samples, (double)soft_radius);
  }
  int errors = 0;
  if (std::strcmp(output_file, "null") != 0 && (!sharded || rank == 0)) {
    std::vector<uint32_t> fb((size_t)width * height);
    if (sharded) fb = gathered;  // the frame assembled from every rank's tiles
    else RT_CHECK(rt_read_framebuffer(r, fb.data(), fb.size()));
    RT_CHECK(rt::SavePngARGB(output_file, fb.data(), width, height));
    if (reference_file) {
      std::vector<uint32_t> out, ref;
      uint32_t ow, oh, rw, rh;
      RT_CHECK(rt::LoadPngARGB(output_file, &out, &ow, &oh));
      RT_CHECK(rt::LoadPngARGB(rt::ResolveAsset(reference_file), &ref, &rw, &rh));
      if (ow != rw || oh != rh) {
        std::printf("FAILED! size mismatch\n");
        errors = -1;
      } else {
        errors = (int)rt::CompareARGB(out.data(), ref.data(), out.size(), 1);
        if (errors == 0) std::printf("PASSED!\n");
        else std::printf("FAILED! %d errors.\n", errors);
      }
    }
  }
  rt_renderer_free(r);
  rt_scene_free(scene);
  if (comm) rt_shard_comm_free(comm);
  return errors;
}
