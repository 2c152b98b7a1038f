// Stand-alone check of the driver's lane / join decision
// (skybox_rt_amd/csrc/runtime/lanes.h), built and run by
// tests/test_frame_lanes_cpu.py.  Each case feeds LaneOrder a sequence of
// operations -- 'o' an ordinary one, '0' / '1' a launch that asked for that
// lane -- and compares the (lane, wait) steps it answers with.
#include <cstdio>
#include <string>
#include <vector>

#include "lanes.h"

namespace {

int failures = 0;

std::vector<vxlanes::Step> run(vxlanes::LaneOrder& o, const std::string& ops) {
  std::vector<vxlanes::Step> out;
  for (char c : ops) out.push_back(c == 'o' ? o.ordinary() : o.laned(c - '0'));
  return out;
}

// `want`: per operation "<lane><wait>" with wait '-' (none), '0' or '1'
void expect(const char* name, bool overlap, const std::string& ops, const std::string& want) {
  vxlanes::LaneOrder o(overlap);
  const std::vector<vxlanes::Step> got = run(o, ops);
  std::string s;
  for (const vxlanes::Step& g : got) {
    s += (char)('0' + g.lane);
    s += g.wait_for < 0 ? '-' : (char)('0' + g.wait_for);
  }
  if (s != want) {
    std::printf("FAIL %s: ops %s -> %s, expected %s\n", name, ops.c_str(), s.c_str(), want.c_str());
    ++failures;
  } else {
    std::printf("ok   %s\n", name);
  }
}

int count_waits(bool overlap, const std::string& ops) {
  vxlanes::LaneOrder o(overlap);
  int n = 0;
  for (const vxlanes::Step& g : run(o, ops)) n += g.wait_for >= 0;
  return n;
}

}  // namespace

int main() {
  // frames alternating 0, 1, 0, 1 on a fresh device: no join at all
  expect("alternating", true, "01010101", "0-1-0-1-0-1-0-1-");
  {
    std::string ops;
    for (int i = 0; i < 1000; ++i) ops += (char)('0' + (i & 1));
    if (count_waits(true, ops) != 0) {
      std::printf("FAIL steady state records events\n");
      ++failures;
    }
  }
  // an ordinary operation after laned launches: lane 0 waits for lane 1, once
  expect("ordinary joins lane 1 once", true, "0101ooo", "0-1-0-1-010-0-");
  // ... and not at all when only lane 0 held launches
  expect("ordinary after lane 0 only", true, "00o", "0-0-0-");
  // the first lane-1 launch after ordinary work waits for lane 0, once
  expect("lane 1 waits for ordinary work", true, "oo0101", "0-0-0-100-1-");
  expect("lane 0 needs no wait after ordinary work", true, "o00", "0-0-0-");
  // a list rebuild between overlapped frames: behind both lanes, ahead of both
  expect("setup between frames", true, "0101oo0101", "0-1-0-1-010-0-100-1-");
  expect("setup before a lane-1 frame", true, "010o101", "0-1-0-01100-1-");
  // the host saw both lanes run empty: nothing left to join
  {
    vxlanes::LaneOrder o(true);
    run(o, "o01o");  // the last ordinary operation joined lane 1 and is itself unjoined
    o.lane0_idle();
    o.lane1_idle();
    const vxlanes::Step a = o.laned(1);   // nothing ordinary left to wait for
    const vxlanes::Step b = o.ordinary();  // lane 1 holds a launch again
    vxlanes::LaneOrder o2(true);
    run(o2, "01");
    o2.lane1_idle();
    const vxlanes::Step c = o2.ordinary();  // lane 1 seen empty: no join
    if (a.lane != 1 || a.wait_for != -1 || b.wait_for != 1 || c.wait_for != -1) {
      std::printf("FAIL idle notifications\n");
      ++failures;
    } else {
      std::printf("ok   idle notifications\n");
    }
  }
  // overlap disabled: everything is lane 0, no wait ever
  expect("overlap off", false, "0101o1o0", "0-0-0-0-0-0-0-0-");
  // a lane out of range is an ordinary operation
  {
    vxlanes::LaneOrder o(true);
    run(o, "01");
    const vxlanes::Step s = o.laned(7);
    if (s.lane != 0 || s.wait_for != 1) {
      std::printf("FAIL lane out of range\n");
      ++failures;
    }
  }
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
