// ao_quot_check.cpp -- the resolve launch's two exact divisions (kernels/rt_common.h rt_ao_quot) on the
// host, as the kernel compiles them (binary32, no contraction), against integer division: rt_ao_mix
// for every N in 1..65535, seven counts each and every channel value, and rt_ao_relight_mix against
// rt_relight_mix for every W in 1..4080 over a ladder of O and every channel value.  Built and run
// by tests/test_ao_cpu.py.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>
#include <cstdio>

#include "rt_common.h"

int main() {
  unsigned long long checked = 0, bad = 0;
  for (uint32_t N = 1; N <= 65535u; ++N) {
    const float rd = 1.0f / (float)(2u * N);
    const uint32_t os[7] = {0u, 1u < N ? 1u : N, N / 3u, N / 2u, (2u * N) / 3u, N - 1u, N};
    for (uint32_t o : os) {
      for (uint32_t c = 0; c < 256u; ++c) {
        const uint32_t x = 2u * c * (N - o) + N, want = x / (2u * N);
        bad += rt_ao_quot(x, 2u * N, rd) != want;
        const uint32_t argb = 0xa5000000u | (c << 16) | ((255u - c) << 8) | c;
        const uint32_t w2 = (2u * (255u - c) * (N - o) + N) / (2u * N);
        bad += rt_ao_mix(argb, o, N, rd) != (0xa5000000u | (want << 16) | (w2 << 8) | want);
        checked += 2;
      }
    }
  }
  for (uint32_t W = 1; W <= 4080u; ++W) {
    const float rd = 1.0f / (float)(2u * W);
    const rt_relight_div_t d = rt_relight_div(W);
    const uint32_t step = W > 64u ? W / 37u + 1u : 1u;
    for (uint32_t O = 0; O <= W; O = (O < W && O + step > W) ? W : O + step) {
      for (uint32_t c = 0; c < 256u; ++c) {
        const uint32_t b = 0x5a000000u | (c << 16) | ((255u - c) << 8) | (c ^ 0x55u);
        bad += rt_ao_relight_mix(b, O, W, rd) != rt_relight_mix(b, O, W, d.s, d.m);
        const uint32_t x = 2u * ((W - O) * c + O * (c >> 1)) + W;
        bad += rt_ao_quot(x, 2u * W, rd) != x / (2u * W);
        checked += 2;
      }
    }
  }
  std::printf("%llu checked, %llu failure(s)\n", checked, bad);
  return bad != 0;
}
