// The RT host app's image table and its two pure decisions
// (skybox_rt_amd/csrc/app/frame_image.h): a stand-alone program, no GPU, no driver.
//   (a) frame_images: known answers, one literal row per configuration the API can reach
//       (and the rule's answer for a few inputs it cannot);
//   (b) over the whole input product: one image, or two exactly for the two-kernel path
//       tracer's frame, and never an instrumented image for a frame that is not;
//   (c) resolve_group under a fake "file exists": the per-file fallback, the all-or-none
//       group of the kernel directory, the images next to an anchor and their refusal.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "frame_image.h"

using namespace rtimg;

static long failures = 0;

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

static void section(const char* name, long before) {
  std::printf("%s %s\n", failures == before ? "ok  " : "BAD ", name);
}

static bool is_stats(Image id) {
  const char* f = desc(id).file;
  const char* tail = "_stats.vxbin";
  return std::strlen(f) >= std::strlen(tail) && std::strcmp(f + std::strlen(f) - std::strlen(tail), tail) == 0;
}

struct Row {
  const char* what;
  FrameIn in;  // mode, instrumented, nlights, accum_k, pq, tail, bvh_walk, deep, bvh4h, rt_bvh
  Image first, second;
};

// a regular tree: the binary16 BVH4, the rt_bvh pair loaded at creation (.., 0, 1, 1); a deep
// one from creation on: no rt_bvh pair (.., 1, 0, 0) -- or deep since a later configure, the
// pair still loaded (.., 1, 1, 1).  Shadows are no input: a plain and a shadow frame run the same image.
static const Row kRows[] = {
    {"plain / shadow frame", {0, 0, 0, 0, 0, 0, 0, 0, 1, 1}, IMG_RT, IMG_NONE},
    {"plain / shadow frame, one light set", {0, 0, 1, 0, 0, 0, 0, 0, 1, 1}, IMG_RT, IMG_NONE},
    {"plain / shadow frame, deep", {0, 0, 0, 0, 0, 0, 0, 1, 0, 0}, IMG_RT_DEEP, IMG_NONE},
    {"plain / shadow frame, deep since a configure", {0, 0, 0, 0, 0, 0, 0, 1, 1, 1}, IMG_RT_DEEP, IMG_NONE},
    {"plain / shadow frame, instrumented", {0, 1, 0, 0, 0, 0, 0, 0, 1, 1}, IMG_RT_STATS, IMG_NONE},
    {"plain / shadow frame, deep, instrumented", {0, 1, 0, 0, 0, 0, 0, 1, 0, 0}, IMG_RT_DEEP_STATS, IMG_NONE},
    {"BVH_WALK", {0, 0, 0, 0, 0, 0, 1, 0, 1, 1}, IMG_RT_BVH, IMG_NONE},
    {"BVH_WALK, instrumented", {0, 1, 0, 0, 0, 0, 1, 0, 1, 1}, IMG_RT_BVH_STATS, IMG_NONE},
    {"BVH_WALK, no rt_bvh pair", {0, 0, 0, 0, 0, 0, 1, 0, 1, 0}, IMG_RT, IMG_NONE},
    {"BVH_WALK, no rt_bvh pair, instrumented", {0, 1, 0, 0, 0, 0, 1, 0, 1, 0}, IMG_RT_STATS, IMG_NONE},
    {"BVH_WALK, deep", {0, 0, 0, 0, 0, 0, 1, 1, 0, 0}, IMG_RT_DEEP, IMG_NONE},
    {"BVH_WALK, deep since a configure", {0, 1, 0, 0, 0, 0, 1, 1, 1, 1}, IMG_RT_DEEP_STATS, IMG_NONE},
    {"ordered tail", {0, 0, 0, 0, 0, 1, 0, 0, 1, 1}, IMG_RT_OM, IMG_NONE},
    {"ordered tail, instrumented", {0, 1, 0, 0, 0, 1, 0, 0, 1, 1}, IMG_RT_OM, IMG_NONE},
    {"ordered tail, BVH_WALK", {0, 0, 0, 0, 0, 1, 1, 0, 1, 1}, IMG_RT_OM, IMG_NONE},
    {"ordered tail, path frame", {1, 0, 0, 0, 0, 1, 0, 0, 1, 1}, IMG_PT, IMG_NONE},
    {"2 lights, shadow frame", {0, 0, 2, 0, 0, 0, 0, 0, 1, 1}, IMG_RT_LIGHTS, IMG_NONE},
    {"16 lights, shadow frame", {0, 0, 16, 0, 0, 0, 0, 0, 1, 1}, IMG_RT_LIGHTS, IMG_NONE},
    {"2 lights, shadow frame, instrumented", {0, 1, 2, 0, 0, 0, 0, 0, 1, 1}, IMG_RT_LIGHTS_STATS, IMG_NONE},
    {"path frame", {1, 0, 0, 0, 0, 0, 0, 0, 1, 1}, IMG_PT, IMG_NONE},
    {"path frame, instrumented", {1, 1, 0, 0, 0, 0, 0, 0, 1, 1}, IMG_PT_STATS, IMG_NONE},
    {"path frame, deep", {1, 0, 0, 0, 0, 0, 0, 1, 0, 0}, IMG_PT_DEEP, IMG_NONE},
    {"path frame, deep, instrumented", {1, 1, 0, 0, 0, 0, 0, 1, 0, 0}, IMG_PT_DEEP_STATS, IMG_NONE},
    {"path frame, two kernels", {1, 0, 0, 0, 1, 0, 0, 0, 1, 1}, IMG_PT_PRIMARY, IMG_PT_QUEUE},
    {"path frame, two kernels, one light set", {1, 0, 1, 0, 1, 0, 0, 0, 1, 1}, IMG_PT_PRIMARY, IMG_PT_QUEUE},
    {"path frame, two kernels, instrumented", {1, 1, 0, 0, 1, 0, 0, 0, 1, 1}, IMG_PT_PRIMARY_STATS,
     IMG_PT_QUEUE_STATS},
    {"path frame, 2 lights", {1, 0, 2, 0, 0, 0, 0, 0, 1, 1}, IMG_PT_LIGHTS, IMG_NONE},
    {"path frame, 8 lights", {1, 0, 8, 0, 0, 0, 0, 0, 1, 1}, IMG_PT_LIGHTS, IMG_NONE},
    {"accumulation, no light set", {1, 0, 0, 1, 0, 0, 0, 0, 1, 1}, IMG_PT_ACCUM, IMG_NONE},
    {"accumulation, 1 light", {1, 0, 1, 32, 0, 0, 0, 0, 1, 1}, IMG_PT_ACCUM, IMG_NONE},
    {"accumulation, 2 lights", {1, 0, 2, 1, 0, 0, 0, 0, 1, 1}, IMG_PT_LIGHTS_ACCUM, IMG_NONE},
    {"accumulation, 8 lights, 32 samples", {1, 0, 8, 32, 0, 0, 0, 0, 1, 1}, IMG_PT_LIGHTS_ACCUM, IMG_NONE},
    // cannot occur (accum_begin needs a path configuration and configure resets nlights): the
    // lights of a shadow configuration do not reach an accumulation launch
    {"accumulation, 2 lights left by a shadow frame", {0, 0, 2, 1, 0, 0, 0, 0, 1, 1}, IMG_PT_ACCUM, IMG_NONE},
    {"flat frame", {2, 0, 0, 0, 0, 0, 0, 0, 1, 1}, IMG_FLAT, IMG_NONE},
    {"flat frame, instrumented", {2, 1, 0, 0, 0, 0, 0, 0, 1, 1}, IMG_FLAT_STATS, IMG_NONE},
    {"flat frame, deep tree", {2, 0, 0, 0, 0, 0, 0, 1, 0, 0}, IMG_FLAT, IMG_NONE},
    {"raster frame", {3, 0, 0, 0, 0, 0, 0, 0, 1, 1}, IMG_RASTER, IMG_NONE},
    {"raster frame, instrumented", {3, 1, 0, 0, 0, 0, 0, 0, 1, 1}, IMG_RASTER, IMG_NONE},
    {"raster frame, ordered tail", {3, 0, 0, 0, 0, 1, 0, 1, 0, 0}, IMG_RASTER, IMG_NONE},
};

static void known_answers() {
  const long before = failures;
  for (const Row& row : kRows) {
    const FrameImages got = frame_images(row.in);
    CHECK(got.first == row.first && got.second == row.second, "%s: got %d, %d expected %d, %d", row.what,
          (int)got.first, (int)got.second, (int)row.first, (int)row.second);
  }
  section("known answers", before);
}

static void product() {
  const long before = failures;
  const uint32_t nl[] = {0, 1, 2, 16}, ak[] = {0, 1, 32};
  long cases = 0, pairs = 0;
  for (int mode = 0; mode < 4; ++mode)
    for (uint32_t n : nl)
      for (uint32_t k : ak)
        for (int bits = 0; bits < 128; ++bits) {
          const FrameIn in{mode,      (bits & 1) != 0,  n, k, (bits & 2) != 0, (bits & 4) != 0, (bits & 8) != 0,
                           (bits & 16) != 0, (bits & 32) != 0, (bits & 64) != 0};
          const FrameImages got = frame_images(in);
          ++cases;
          CHECK(got.first > IMG_NONE && got.first < IMG_COUNT, "mode %d bits %d n %u k %u: first %d", mode, bits, n, k,
                (int)got.first);
          CHECK(got.second >= IMG_NONE && got.second < IMG_COUNT, "second %d", (int)got.second);
          if (got.first <= IMG_NONE || got.first >= IMG_COUNT || got.second >= IMG_COUNT) continue;
          // two images precisely for the two-kernel path tracer's frame: a path frame of one
          // light that is no accumulation launch
          const bool two = k == 0 && mode == 1 && in.pq && n < 2;
          CHECK((got.second != IMG_NONE) == two, "mode %d bits %d n %u k %u: second %d", mode, bits, n, k,
                (int)got.second);
          pairs += two;
          if (!in.instrumented)
            CHECK(!is_stats(got.first) && (got.second == IMG_NONE || !is_stats(got.second)),
                  "mode %d bits %d n %u k %u: instrumented image %s", mode, bits, n, k, desc(got.first).file);
          // the frame's image is never one of the setup's
          CHECK(got.first != IMG_SETUP && got.first != IMG_SAH, "a setup image");
        }
  std::printf("%ld inputs, %ld of them launch two images\n", cases, pairs);
  section("input product", before);
}

// ---- the path resolver under a fake file system ---------------------------------------------

struct Fs {
  std::set<std::string> files;
  mutable std::vector<std::string> asked;
  bool operator()(const std::string& p) const {
    asked.push_back(p);
    return files.count(p) != 0;
  }
};

static Fs lib_with_everything() {
  Fs fs;
  for (int i = 0; i < IMG_COUNT; ++i) fs.files.insert(std::string("L/") + desc((Image)i).file);
  return fs;
}

static int resolve(const Fs& fs, Group g, std::vector<Found>* out, std::string* err) {
  fs.asked.clear();
  err->clear();
  // (by reference: the questions asked are part of what is checked)
  return resolve_group("K", "L", g, [&fs](const std::string& p) { return fs(p); }, out, err);
}

static std::string path_of(const std::vector<Found>& v, Image id) {
  for (const Found& f : v)
    if (f.id == id) return f.path;
  return "(none)";
}

static void table() {
  const long before = failures;
  std::set<std::string> names;
  for (int i = 0; i < IMG_COUNT; ++i) {
    const Desc& d = desc((Image)i);
    CHECK(d.file != nullptr && names.insert(d.file).second, "image %d: no file name of its own", i);
    CHECK((d.source == SRC_NEXT_TO) == (d.anchor != IMG_NONE), "image %d: anchor", i);
    if (d.anchor != IMG_NONE) CHECK(desc(d.anchor).source == SRC_PER_FILE, "image %d: its anchor's rule", i);
  }
  CHECK(names.size() == 25, "%zu images", names.size());
  CHECK(std::string(desc(IMG_RT_DEEP_STATS).file) == "rt_kernel_deep_stats.vxbin", "%s", desc(IMG_RT_DEEP_STATS).file);
  CHECK(std::string(desc(IMG_PT_QUEUE_STATS).file) == "pt_queue_stats.vxbin", "%s", desc(IMG_PT_QUEUE_STATS).file);
  CHECK(std::string(desc(IMG_PT_LIGHTS_ACCUM).file) == "pt_lights_accum.vxbin", "%s", desc(IMG_PT_LIGHTS_ACCUM).file);
  CHECK(std::string(desc(IMG_SAH).file) == "bvh_sah.vxbin", "%s", desc(IMG_SAH).file);
  section("image table", before);
}

static void rule_per_file() {
  const long before = failures;
  std::vector<Found> v;
  std::string err;
  // an A/B variant directory holding rt_kernel.vxbin only
  Fs fs = lib_with_everything();
  fs.files.insert("K/rt_kernel.vxbin");
  CHECK(resolve(fs, GRP_REGULAR, &v, &err) == 0 && v.size() == 4, "code / %zu paths", v.size());
  CHECK(path_of(v, IMG_RT) == "K/rt_kernel.vxbin", "%s", path_of(v, IMG_RT).c_str());
  CHECK(path_of(v, IMG_RT_STATS) == "L/rt_kernel_stats.vxbin", "%s", path_of(v, IMG_RT_STATS).c_str());
  CHECK(path_of(v, IMG_PT) == "L/pt_kernel.vxbin", "%s", path_of(v, IMG_PT).c_str());
  CHECK(path_of(v, IMG_PT_STATS) == "L/pt_kernel_stats.vxbin", "%s", path_of(v, IMG_PT_STATS).c_str());
  CHECK(resolve(fs, GRP_MODES, &v, &err) == 0 && v.size() == 3 && path_of(v, IMG_RASTER) == "L/raster_kernel.vxbin",
        "%s", path_of(v, IMG_RASTER).c_str());
  CHECK(resolve(fs, GRP_DEEP, &v, &err) == 0 && v.size() == 4 && path_of(v, IMG_PT_DEEP) == "L/pt_kernel_deep.vxbin",
        "%s", path_of(v, IMG_PT_DEEP).c_str());
  // a file in neither directory: the library's path (its upload fails), no refusal here
  fs.files.erase("L/rt_om.vxbin");
  CHECK(resolve(fs, GRP_OM, &v, &err) == 0 && v.size() == 1 && v[0].path == "L/rt_om.vxbin", "rt_om");
  fs.files.insert("K/bvh_sah.vxbin");
  CHECK(resolve(fs, GRP_SAH, &v, &err) == 0 && v.size() == 1 && v[0].path == "K/bvh_sah.vxbin", "bvh_sah");
  CHECK(resolve(fs, GRP_SETUP, &v, &err) == 0 && v.size() == 1 && v[0].path == "L/rt_setup.vxbin", "rt_setup");
  CHECK(resolve_file("K", "L", "bvh_build.vxbin", fs) == "L/bvh_build.vxbin", "bvh_build");
  section("rule 1: per-file fallback", before);
}

static void rule_kdir_all() {
  const long before = failures;
  std::vector<Found> v;
  std::string err;
  const Image pq[4] = {IMG_PT_PRIMARY, IMG_PT_PRIMARY_STATS, IMG_PT_QUEUE, IMG_PT_QUEUE_STATS};
  // every subset of the four in the kernel directory; the library directory holds them all
  for (int have = 0; have < 16; ++have) {
    Fs fs = lib_with_everything();
    for (int j = 0; j < 4; ++j)
      if (have & (1 << j)) fs.files.insert(std::string("K/") + desc(pq[j]).file);
    const int e = resolve(fs, GRP_PQ, &v, &err);
    if (have == 15) {
      CHECK(e == 0 && v.size() == 4, "all four: code %d, %zu paths", e, v.size());
      for (int j = 0; j < 4 && v.size() == 4; ++j)
        CHECK(v[j].id == pq[j] && v[j].path == std::string("K/") + desc(pq[j]).file, "%s", v[j].path.c_str());
    } else {
      CHECK(e == 1 && v.empty() && err.empty(), "subset %d: code %d, %zu paths, '%s'", have, e, v.size(), err.c_str());
    }
    for (const std::string& p : fs.asked) CHECK(p.compare(0, 2, "K/") == 0, "subset %d asked for %s", have, p.c_str());
  }
  section("rule 2: the whole group from the kernel directory or nothing", before);
}

static void rule_next_to() {
  const long before = failures;
  std::vector<Found> v;
  std::string err;
  // no path tracer in the kernel directory: the library's, and pt_accum next to it
  Fs fs = lib_with_everything();
  fs.files.insert("K/rt_kernel.vxbin");
  CHECK(resolve(fs, GRP_ACCUM, &v, &err) == 0 && v.size() == 1 && v[0].path == "L/pt_accum.vxbin", "library anchor");
  CHECK(resolve(fs, GRP_PLIGHTS, &v, &err) == 0 && v.size() == 2 && path_of(v, IMG_PT_LIGHTS) == "L/pt_lights.vxbin" &&
            path_of(v, IMG_PT_LIGHTS_ACCUM) == "L/pt_lights_accum.vxbin", "library anchor, pt_lights");
  // ... while rt_lights goes with the kernel directory's rt_kernel.vxbin: not there, refused
  CHECK(resolve(fs, GRP_LIGHTS, &v, &err) == -2 && v.empty(), "rt_lights next to K/rt_kernel.vxbin");
  CHECK(err == "no rt_lights.vxbin next to K/rt_kernel.vxbin", "'%s'", err.c_str());
  fs.files.insert("K/rt_lights.vxbin");
  CHECK(resolve(fs, GRP_LIGHTS, &v, &err) == -2 && v.empty(), "rt_lights_stats next to K/rt_kernel.vxbin");
  CHECK(err == "no rt_lights_stats.vxbin next to K/rt_kernel.vxbin", "'%s'", err.c_str());
  fs.files.insert("K/rt_lights_stats.vxbin");
  CHECK(resolve(fs, GRP_LIGHTS, &v, &err) == 0 && v.size() == 2 && path_of(v, IMG_RT_LIGHTS) == "K/rt_lights.vxbin" &&
            path_of(v, IMG_RT_LIGHTS_STATS) == "K/rt_lights_stats.vxbin" && err.empty(), "kernel directory's pair");
  // pt_compact: a kernel directory with a pt_kernel.vxbin of its own and no pt_accum.vxbin
  Fs pc = lib_with_everything();
  pc.files.insert("K/pt_kernel.vxbin");
  pc.files.insert("K/pt_kernel_stats.vxbin");
  CHECK(resolve(pc, GRP_ACCUM, &v, &err) == -2 && v.empty(), "pt_compact: pt_accum");
  CHECK(err == "no pt_accum.vxbin next to K/pt_kernel.vxbin", "'%s'", err.c_str());
  CHECK(resolve(pc, GRP_PLIGHTS, &v, &err) == -2 && v.empty(), "pt_compact: pt_lights");
  CHECK(err == "no pt_lights.vxbin next to K/pt_kernel.vxbin", "'%s'", err.c_str());
  // (its rt_lights comes from the library with the library's rt_kernel.vxbin)
  CHECK(resolve(pc, GRP_LIGHTS, &v, &err) == 0 && v.size() == 2 && v[0].path == "L/rt_lights.vxbin", "pt_compact: rt_lights");
  pc.files.insert("K/pt_accum.vxbin");
  CHECK(resolve(pc, GRP_ACCUM, &v, &err) == 0 && v.size() == 1 && v[0].path == "K/pt_accum.vxbin", "own pt_accum");
  // missing next to the library's anchor: refused as well
  Fs bare = lib_with_everything();
  bare.files.erase("L/pt_accum.vxbin");
  CHECK(resolve(bare, GRP_ACCUM, &v, &err) == -2 && err == "no pt_accum.vxbin next to L/pt_kernel.vxbin", "'%s'",
        err.c_str());
  section("rule 3: next to the anchor image, or refused", before);
}

int main() {
  table();
  known_answers();
  product();
  rule_per_file();
  rule_kdir_all();
  rule_next_to();
  std::printf("%zu known answers, %ld failure(s)\n", sizeof(kRows) / sizeof(kRows[0]), failures);
  return failures ? 1 : 0;
}
