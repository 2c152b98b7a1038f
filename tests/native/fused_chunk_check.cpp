// fused_chunk_check.cpp -- the conditions of RT_FLAG_FUSED (skybox_rt_amd/csrc/app/fused_chunk.h) over
// every configuration and knob value; a stand-alone program (tests/test_fused_chunk_cpu.py builds and
// runs it, with the sanitizers where the toolchain has them).  Prints "<n> case(s), <m> failure(s)".
#include <cstdio>

#include "fused_chunk.h"

static int failures = 0, cases = 0;

static void expect(bool ok, const char* what, int i = -1) {
  ++cases;
  if (!ok) {
    ++failures;
    std::printf("FAIL: %s (%d)\n", what, i);
  }
}

int main() {
  const uint32_t bit = 0x200u;
  // the knob: unset, empty and every number but 0 are on
  expect(rtfused::knob(nullptr), "unset is on");
  expect(rtfused::knob(""), "empty is on");
  expect(rtfused::knob("1"), "1 is on");
  expect(rtfused::knob("2"), "2 is on");
  expect(rtfused::knob("-1"), "-1 is on");
  expect(!rtfused::knob("0"), "0 is off");
  expect(!rtfused::knob("00"), "00 is off");
  expect(!rtfused::knob("off"), "a word reads as 0, as the other frame knobs read it");
  // the flag: the one-light primary+shadow frame alone, and only with the knob on
  const char* envs[] = {nullptr, "", "1", "0", "7"};
  for (int i = 0; i < 32; ++i) {
    const rtfused::Conf c = {(i & 1) != 0, (i & 2) != 0, (i & 4) != 0, (i & 8) != 0, (i & 16) != 0};
    const bool frame = c.shadows && !c.path && !c.flat && !c.raster && !c.tail;
    expect(frame == (i == 1), "one configuration of the 32 is the frame", i);
    for (const char* e : envs) {
      const uint32_t f = rtfused::flag(c, e, bit);
      expect(f == 0u || f == bit, "the bit or nothing", i);
      expect((f != 0u) == (frame && rtfused::knob(e)), "set exactly for the frame with the knob on", i);
    }
    expect(rtfused::flag(c, "0", bit) == 0u, "never with the knob off", i);
  }
  std::printf("%d case(s), %d failure(s)\n", cases, failures);
  return failures != 0;
}
