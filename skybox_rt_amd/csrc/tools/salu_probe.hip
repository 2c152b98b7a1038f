// salu_probe.hip -- sustained scalar-ALU issue rate of a gfx950 CU, the
// ceiling the per-wave SALU counts of the RT kernels (profiles/pmc_*.json,
// DESIGN.md 4.1) are set against.
//
// Every wave runs a bounded loop over an unrolled stream of 128 independent
// scalar ALU operations (eight accumulators in SGPRs, round robin), alone
// ("salu") or interleaved 1:1 with independent VALU operations on eight
// VGPR accumulators ("mix").  A launch places exactly k waves on every SIMD
// of every CU: workgroups of 256 threads (one wave per SIMD), each with a
// dynamic LDS allocation sized so that k and no more fit a CU's 160 KiB, on
// a grid of k workgroups per CU -- all resident at once.  Each wave stamps
// the loop with s_memtime (shader cycles) and s_memrealtime (100 MHz) and
// records where it ran (HW_ID, XCC_ID); the host checks the placement and
// reports, per k, the scalar instructions per cycle per CU:
//   k * 4 waves * stream operations per wave / median wave cycles
// (the waves of a CU run the loop side by side, so a wave's cycles are the
// CU's), with the shader clock from the two stamps.  The loop's own
// counter / compare / branch (3 per 128) are not counted.
// Usage: salu_probe [iterations]   -- prints one JSON object.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#define CHECK(x)                                                                    \
  do {                                                                              \
    hipError_t e = (x);                                                             \
    if (e != hipSuccess) {                                                          \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));                   \
      std::exit(1);                                                                 \
    }                                                                               \
  } while (0)

// eight independent scalar operations, one per accumulator (a0..a7; k = a
// constant in an SGPR)
#define S0 "s_add_u32 %[a0], %[a0], %[k]\n"
#define S1 "s_xor_b32 %[a1], %[a1], %[k]\n"
#define S2 "s_lshl_b32 %[a2], %[a2], 1\n"
#define S3 "s_and_b32 %[a3], %[a3], %[k]\n"
#define S4 "s_add_u32 %[a4], %[a4], %[k]\n"
#define S5 "s_xor_b32 %[a5], %[a5], %[k]\n"
#define S6 "s_or_b32 %[a6], %[a6], %[k]\n"
#define S7 "s_sub_u32 %[a7], %[a7], %[k]\n"
// and eight independent vector operations, one per accumulator (v0..v7, each
// reading only itself and the constant kv)
#define V0 "v_add_u32 %[v0], %[v0], %[kv]\n"
#define V1 "v_xor_b32 %[v1], %[v1], %[kv]\n"
#define V2 "v_add_u32 %[v2], %[v2], %[kv]\n"
#define V3 "v_xor_b32 %[v3], %[v3], %[kv]\n"
#define V4 "v_add_u32 %[v4], %[v4], %[kv]\n"
#define V5 "v_xor_b32 %[v5], %[v5], %[kv]\n"
#define V6 "v_add_u32 %[v6], %[v6], %[kv]\n"
#define V7 "v_xor_b32 %[v7], %[v7], %[kv]\n"
#define SALU8 S0 S1 S2 S3 S4 S5 S6 S7
#define MIX8 S0 V0 S1 V1 S2 V2 S3 V3 S4 V4 S5 V5 S6 V6 S7 V7
#define X16(a) a a a a a a a a a a a a a a a a

constexpr uint32_t kStream = 128;  // scalar operations per loop iteration
constexpr uint32_t kRec = 8;       // words per wave record

template <bool MIX>
__global__ void __launch_bounds__(256) salu_stream(uint32_t iters, uint32_t seed, uint32_t* rec) {
  extern __shared__ uint32_t lds[];  // occupancy only
  uint32_t a0 = seed, a1 = seed + 1, a2 = seed + 2, a3 = seed + 3, a4 = seed + 4, a5 = seed + 5,
           a6 = seed + 6, a7 = seed + 7;
  a0 = __builtin_amdgcn_readfirstlane(a0); a1 = __builtin_amdgcn_readfirstlane(a1);
  a2 = __builtin_amdgcn_readfirstlane(a2); a3 = __builtin_amdgcn_readfirstlane(a3);
  a4 = __builtin_amdgcn_readfirstlane(a4); a5 = __builtin_amdgcn_readfirstlane(a5);
  a6 = __builtin_amdgcn_readfirstlane(a6); a7 = __builtin_amdgcn_readfirstlane(a7);
  const uint32_t k = __builtin_amdgcn_readfirstlane(seed | 1u);
  uint32_t v0 = threadIdx.x, v1 = v0 + 1, v2 = v0 + 2, v3 = v0 + 3, v4 = v0 + 4, v5 = v0 + 5,
           v6 = v0 + 6, v7 = v0 + 7;
  const uint32_t kv = threadIdx.x | 1u;
  __syncthreads();  // the workgroup's four waves start together
  const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
  const uint64_t c0 = __builtin_amdgcn_s_memtime();
  for (uint32_t i = 0; i < iters; ++i) {
    if constexpr (MIX) {
      asm volatile(X16(MIX8)
                   : [a0] "+s"(a0), [a1] "+s"(a1), [a2] "+s"(a2), [a3] "+s"(a3), [a4] "+s"(a4),
                     [a5] "+s"(a5), [a6] "+s"(a6), [a7] "+s"(a7), [v0] "+v"(v0), [v1] "+v"(v1),
                     [v2] "+v"(v2), [v3] "+v"(v3), [v4] "+v"(v4), [v5] "+v"(v5), [v6] "+v"(v6),
                     [v7] "+v"(v7)
                   : [k] "s"(k), [kv] "v"(kv)
                   : "scc");
    } else {
      asm volatile(X16(SALU8)
                   : [a0] "+s"(a0), [a1] "+s"(a1), [a2] "+s"(a2), [a3] "+s"(a3), [a4] "+s"(a4),
                     [a5] "+s"(a5), [a6] "+s"(a6), [a7] "+s"(a7)
                   : [k] "s"(k)
                   : "scc");
    }
  }
  const uint64_t c1 = __builtin_amdgcn_s_memtime();
  const uint64_t r1 = __builtin_amdgcn_s_memrealtime();
  const uint32_t hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));    // HW_ID
  const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));  // XCC_ID
  const uint32_t acc = a0 ^ a1 ^ a2 ^ a3 ^ a4 ^ a5 ^ a6 ^ a7 ^ v0 ^ v1 ^ v2 ^ v3 ^ v4 ^ v5 ^ v6 ^ v7;
  if ((threadIdx.x & 63u) == 0) {
    uint32_t* o = rec + kRec * (blockIdx.x * 4 + (threadIdx.x >> 6));
    o[0] = (uint32_t)(c1 - c0);
    o[1] = (uint32_t)(r1 - r0);
    o[2] = hw;
    o[3] = xcc;
    o[4] = (uint32_t)c0;
    o[5] = (uint32_t)c1;
    o[6] = acc;  // keeps the accumulators
    o[7] = lds[0] & 0u;
  }
}

static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.empty() ? 0.0 : v[v.size() / 2];
}

template <bool MIX>
static void run(int cus, uint32_t k, uint32_t iters, uint32_t* d_rec, bool last) {
  // k workgroups fit a CU's LDS and k + 1 do not
  const uint32_t cu_lds = 160u * 1024u;
  const uint32_t lds = (cu_lds / (k + 1) / 1024u + 1u) * 1024u;
  CHECK(hipFuncSetAttribute((const void*)salu_stream<MIX>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds));
  const uint32_t blocks = (uint32_t)cus * k, waves = blocks * 4;
  std::vector<uint32_t> h((size_t)waves * kRec);
  double ipc = 0, wave_ipc = 0, clock_mhz = 0, med_cyc = 0, spread = 0;
  bool placed = false;
  uint32_t max_per_simd = 0, simds = 0;
  for (int rep = 0; rep < 3; ++rep) {  // the last repetition is reported
    hipLaunchKernelGGL(salu_stream<MIX>, dim3(blocks), dim3(256), lds, 0, iters, 0x9e3779b9u + rep, d_rec);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(h.data(), d_rec, h.size() * 4, hipMemcpyDeviceToHost));
    std::vector<double> cyc, clk;
    std::map<uint32_t, uint32_t> per_simd;
    for (uint32_t w = 0; w < waves; ++w) {
      const uint32_t* o = &h[(size_t)w * kRec];
      cyc.push_back((double)o[0]);
      if (o[1]) clk.push_back((double)o[0] / (double)o[1] * 100.0);
      // SIMD of the chip: XCC, then HW_ID's se / sh / cu (bits 8-15) and simd (bits 4-5)
      ++per_simd[((o[3] & 0xfu) << 16) | (o[2] & 0xff30u)];
    }
    med_cyc = median(cyc);
    clock_mhz = median(clk);
    spread = (*std::max_element(cyc.begin(), cyc.end()) - *std::min_element(cyc.begin(), cyc.end())) / med_cyc;
    max_per_simd = 0;
    for (auto& kv : per_simd) max_per_simd = std::max(max_per_simd, kv.second);
    simds = (uint32_t)per_simd.size();
    placed = simds == (uint32_t)cus * 4 && max_per_simd == k;
    const double ops = (double)iters * kStream;
    wave_ipc = ops / med_cyc;
    ipc = wave_ipc * 4.0 * k;
  }
  std::printf("    {\"stream\": \"%s\", \"waves_per_simd\": %u, \"lds_bytes\": %u, \"waves\": %u, "
              "\"median_wave_cycles\": %.0f, \"wave_cycles_spread\": %.4f, \"clock_mhz\": %.0f, "
              "\"salu_per_cycle_per_wave\": %.4f, \"salu_per_cycle_per_cu\": %.4f, "
              "\"simds_seen\": %u, \"max_waves_on_a_simd\": %u, \"placement_ok\": %s}%s\n",
              MIX ? "mix" : "salu", k, lds, waves, med_cyc, spread, clock_mhz, wave_ipc, ipc, simds,
              max_per_simd, placed ? "true" : "false", last ? "" : ",");
}

int main(int argc, char** argv) {
  const uint32_t iters = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 0) : 2000u;
  if (iters == 0 || iters > 100000u) {
    std::fprintf(stderr, "iterations must be in 1..100000\n");
    return 2;
  }
  int cus = 0;
  CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
  const uint32_t ks[] = {1, 2, 4, 7, 8};
  uint32_t* d_rec = nullptr;
  CHECK(hipMalloc(&d_rec, (size_t)cus * 8 * 4 * kRec * 4));
  std::printf("{\"probe\": \"salu_probe\", \"cus\": %d, \"iterations\": %u, \"stream_ops_per_iteration\": %u,\n"
              " \"note\": \"mix = the same scalar stream interleaved 1:1 with independent VALU operations; "
              "rates count the stream's scalar operations only\",\n \"runs\": [\n",
              cus, iters, kStream);
  for (size_t i = 0; i < 5; ++i) run<false>(cus, ks[i], iters, d_rec, false);
  for (size_t i = 0; i < 5; ++i) run<true>(cus, ks[i], iters, d_rec, i == 4);
  std::printf(" ]}\n");
  CHECK(hipFree(d_rec));
  return 0;
}
