// frame_image.h -- the RT host app's kernel images as a table, and its two decisions about
// them as pure functions: where an image's file is taken from (resolve_group) and which image
// a frame runs (frame_images).  Nothing of the driver is included:
// tests/native/frame_image_check.cpp checks both on the CPU.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace rtimg {

// every image the renderer keeps (rt_renderer::img); an instrumented image follows its plain one
enum Image : int {
  IMG_NONE = -1,
  IMG_RT, IMG_RT_STATS, IMG_PT, IMG_PT_STATS,                      // primary+shadow, path trace
  IMG_RT_DEEP, IMG_RT_DEEP_STATS, IMG_PT_DEEP, IMG_PT_DEEP_STATS,  // their generic forms
  IMG_FLAT, IMG_FLAT_STATS, IMG_RASTER,
  IMG_PT_PRIMARY, IMG_PT_PRIMARY_STATS, IMG_PT_QUEUE, IMG_PT_QUEUE_STATS,  // path tracing in two kernels
  IMG_RT_BVH, IMG_RT_BVH_STATS,                                    // RT_RENDER_BVH_WALK frames
  IMG_RT_OM,                                                       // scenes with an ordered tail
  IMG_PT_ACCUM,                                                    // progressive accumulation
  IMG_RT_LIGHTS, IMG_RT_LIGHTS_STATS,  // several lights, primary+shadow frame
  IMG_PT_LIGHTS, IMG_PT_LIGHTS_ACCUM,  // several lights, path frame and its accumulation
  IMG_SETUP, IMG_SAH,                  // device setup, device BVH build
  IMG_COUNT
};
// where an image's file is taken from
enum Source {
  SRC_PER_FILE,  // the kernel directory's file when it exists, else the library directory's
  SRC_KDIR_ALL,  // the whole group from the kernel directory, or (a file missing there) none of it
  SRC_NEXT_TO    // the directory its anchor image is taken from; not there: a refusal (-2)
};
// the images loaded together
enum Group { GRP_REGULAR, GRP_DEEP, GRP_MODES, GRP_PQ, GRP_BVH, GRP_OM, GRP_ACCUM, GRP_LIGHTS, GRP_PLIGHTS,
             GRP_SETUP, GRP_SAH };

struct Desc {
  const char* file;
  Source source;
  Image anchor;  // SRC_NEXT_TO only
  Group group;
};

inline const Desc& desc(Image id) {
  static const Desc kTable[IMG_COUNT] = {
      {"rt_kernel.vxbin",            SRC_PER_FILE, IMG_NONE, GRP_REGULAR},
      {"rt_kernel_stats.vxbin",      SRC_PER_FILE, IMG_NONE, GRP_REGULAR},
      {"pt_kernel.vxbin",            SRC_PER_FILE, IMG_NONE, GRP_REGULAR},
      {"pt_kernel_stats.vxbin",      SRC_PER_FILE, IMG_NONE, GRP_REGULAR},
      {"rt_kernel_deep.vxbin",       SRC_PER_FILE, IMG_NONE, GRP_DEEP},
      {"rt_kernel_deep_stats.vxbin", SRC_PER_FILE, IMG_NONE, GRP_DEEP},
      {"pt_kernel_deep.vxbin",       SRC_PER_FILE, IMG_NONE, GRP_DEEP},
      {"pt_kernel_deep_stats.vxbin", SRC_PER_FILE, IMG_NONE, GRP_DEEP},
      {"rt_flat.vxbin",              SRC_PER_FILE, IMG_NONE, GRP_MODES},
      {"rt_flat_stats.vxbin",        SRC_PER_FILE, IMG_NONE, GRP_MODES},
      {"raster_kernel.vxbin",        SRC_PER_FILE, IMG_NONE, GRP_MODES},
      {"pt_primary.vxbin",           SRC_KDIR_ALL, IMG_NONE, GRP_PQ},
      {"pt_primary_stats.vxbin",     SRC_KDIR_ALL, IMG_NONE, GRP_PQ},
      {"pt_queue.vxbin",             SRC_KDIR_ALL, IMG_NONE, GRP_PQ},
      {"pt_queue_stats.vxbin",       SRC_KDIR_ALL, IMG_NONE, GRP_PQ},
      {"rt_bvh.vxbin",               SRC_PER_FILE, IMG_NONE, GRP_BVH},
      {"rt_bvh_stats.vxbin",         SRC_PER_FILE, IMG_NONE, GRP_BVH},
      {"rt_om.vxbin",                SRC_PER_FILE, IMG_NONE, GRP_OM},
      {"pt_accum.vxbin",             SRC_NEXT_TO,  IMG_PT,   GRP_ACCUM},
      {"rt_lights.vxbin",            SRC_NEXT_TO,  IMG_RT,   GRP_LIGHTS},
      {"rt_lights_stats.vxbin",      SRC_NEXT_TO,  IMG_RT,   GRP_LIGHTS},
      {"pt_lights.vxbin",            SRC_NEXT_TO,  IMG_PT,   GRP_PLIGHTS},
      {"pt_lights_accum.vxbin",      SRC_NEXT_TO,  IMG_PT,   GRP_PLIGHTS},
      {"rt_setup.vxbin",             SRC_PER_FILE, IMG_NONE, GRP_SETUP},
      {"bvh_sah.vxbin",              SRC_PER_FILE, IMG_NONE, GRP_SAH},
  };
  return kTable[id];
}

// SRC_PER_FILE for one file name
template <class Exists>
std::string resolve_file(const std::string& kdir, const std::string& libdir, const std::string& file, Exists exists) {
  const std::string path = kdir + "/" + file;
  return exists(path) ? path : libdir + "/" + file;
}

struct Found {
  Image id;
  std::string path;
};

// The files of a group: 0 and one path per image; 1 when a SRC_KDIR_ALL group is not wholly in
// the kernel directory -- nothing to load, no error; -2 when an image is not next to its anchor,
// *err naming the file and the directory.  (A SRC_PER_FILE path is not probed in the library
// directory: a file missing there too fails its upload.)
template <class Exists>
int resolve_group(const std::string& kdir, const std::string& libdir, Group group, Exists exists,
                  std::vector<Found>* out, std::string* err) {
  out->clear();
  for (int i = 0; i < IMG_COUNT; ++i) {
    const Desc& d = desc((Image)i);
    if (d.group != group) continue;
    const std::string anchor = d.source == SRC_NEXT_TO ? resolve_file(kdir, libdir, desc(d.anchor).file, exists) : "";
    const std::string path = d.source == SRC_PER_FILE   ? resolve_file(kdir, libdir, d.file, exists)
                             : d.source == SRC_KDIR_ALL ? kdir + "/" + d.file
                                                        : anchor.substr(0, anchor.rfind('/') + 1) + d.file;
    if (d.source != SRC_PER_FILE && !exists(path)) {
      out->clear();
      if (d.source == SRC_KDIR_ALL) return 1;
      *err = "no " + std::string(d.file) + " next to " + anchor;
      return -2;
    }
    out->push_back(Found{(Image)i, path});
  }
  return 0;
}

// the tree runs the generic (deep) images: the regular ones, and every image without a generic
// form, walk the binary16 BVH4 within the shallow stack only
inline bool generic_tree(bool deep, bool bvh4h) { return deep || !bvh4h; }

// a mode's own image: mode 0 primary+shadow, 1 path, 2 flat, 3 raster (no instrumented image)
inline Image mode_image(int mode, int k, bool deep) {
  const Image base[3] = {deep ? IMG_RT_DEEP : IMG_RT, deep ? IMG_PT_DEEP : IMG_PT, IMG_FLAT};
  return mode < 3 ? (Image)(base[mode] + k) : IMG_RASTER;
}

struct FrameIn {
  int mode;           // as mode_image
  bool instrumented;  // RT_RENDER_INSTRUMENTED
  uint32_t nlights;   // rt_renderer_set_lights / set_path_lights (0, 1: one light)
  uint32_t accum_k;   // > 0: an accumulation launch of that many samples
  bool pq, tail;      // the two-kernel path tracer; the scene has an ordered tail
  bool bvh_walk;      // RT_RENDER_BVH_WALK
  bool deep, bvh4h;   // the generic images are loaded; RT_FLAG_BVH4H
  bool rt_bvh;        // the rt_bvh pair is loaded
};
// second: IMG_NONE, or the second launch of a group of 2 (the two-kernel path tracer)
struct FrameImages {
  Image first, second;
};

// the frame reads its lights from the table of rt_renderer_set_lights / set_path_lights
inline bool several_lights(const FrameIn& in) { return in.nlights >= 2 && (in.mode == 1 || in.accum_k == 0); }

// The image(s) a frame runs.  The rule takes the admissions of rt_renderer_set_lights,
// set_path_lights and accum_begin for granted (several lights: a plain shadow frame without a
// tail, or a one-kernel path frame; accumulation: a one-kernel path frame) and answers every
// other input by the same chain.
inline FrameImages frame_images(const FrameIn& in) {
  const int k = in.instrumented && in.mode != 3 ? 1 : 0;
  const bool multi = several_lights(in);
  if (in.accum_k > 0) return {multi ? IMG_PT_LIGHTS_ACCUM : IMG_PT_ACCUM, IMG_NONE};
  if (multi && in.mode == 1) return {IMG_PT_LIGHTS, IMG_NONE};
  if (in.mode == 1 && in.pq) return {(Image)(IMG_PT_PRIMARY + k), (Image)(IMG_PT_QUEUE + k)};
  Image img = mode_image(in.mode, k, in.deep);
  // BVH-walk primary+shadow frames: their own image on the binary16 BVH4 (the deep images walk
  // every layout with the list code paths idle)
  if (in.mode == 0 && in.bvh_walk && !generic_tree(in.deep, in.bvh4h) && in.rt_bvh) img = (Image)(IMG_RT_BVH + k);
  if (multi) img = (Image)(IMG_RT_LIGHTS + k);
  // a scene with an ordered tail: head traced, tail folded, one launch
  if (in.mode == 0 && in.tail) img = IMG_RT_OM;
  return {img, IMG_NONE};
}

}  // namespace rtimg
