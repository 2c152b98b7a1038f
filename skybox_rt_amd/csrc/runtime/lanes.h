// lanes.h -- which cross-lane waits the driver's two launch lanes need.
//
// The HIP driver (hip_driver.cpp) runs its work on two streams: lane 0, the
// driver's stream since the first round, carries every ordinary operation
// (launches, copies) in issue order; a launch may ask for a lane
// (vx_hip_set_launch_lane) and is then ordered only behind earlier work of
// that lane -- two consecutive frames on lanes 0 and 1 may be resident on the
// device together.  What still has to be ordered across the lanes:
//   * an ordinary operation runs behind everything issued before it, so behind
//     lane 1's launches too: lane 0 waits for lane 1 (one event), once;
//   * a lane-1 launch runs behind every ordinary operation issued before it
//     (setup launches, uploads it reads): lane 1 waits for lane 0, once.
// Frames alternating 0, 1, 0, 1 need neither: no event in steady state.
//
// Host-only, no HIP types: LaneOrder takes the sequence of operations and
// answers with the lane each runs on and the wait to queue first, so a plain
// C++ program can test it (tests/test_frame_lanes_cpu.py).
#ifndef VX_RUNTIME_LANES_H
#define VX_RUNTIME_LANES_H

namespace vxlanes {

constexpr int kLanes = 2;

struct Step {
  int lane;       // the stream the operation is queued on
  int wait_for;   // -1, or the lane whose queued work `lane` must wait for first
};

class LaneOrder {
 public:
  explicit LaneOrder(bool overlap = true) : overlap_(overlap) {}
  // an ordinary operation: lane 0, behind everything issued so far
  Step ordinary() {
    Step s{0, -1};
    if (lane1_unjoined_) {
      s.wait_for = 1;
      lane1_unjoined_ = false;
    }
    ordinary_unjoined_ = true;
    return s;
  }

  // a launch that asked for `lane`: behind that lane's earlier work and
  // every ordinary operation, not behind the other lane's laned launches.
  // With overlap off (or a lane out of range) it is an ordinary operation.
  Step laned(int lane) {
    if (!overlap_ || lane < 0 || lane >= kLanes) return ordinary();
    Step s{lane, -1};
    if (lane == 1) {
      if (ordinary_unjoined_) {
        s.wait_for = 0;
        ordinary_unjoined_ = false;
      }
      lane1_unjoined_ = true;
    }
    // lane 0: stream order puts it behind the ordinary work; lane 1 has not
    // seen that work yet, so ordinary_unjoined_ stays as it is
    return s;
  }

  // the host saw lane 1 / lane 0 run empty: nothing of it is left to join
  void lane1_idle() { lane1_unjoined_ = false; }
  void lane0_idle() { ordinary_unjoined_ = false; }

 private:
  bool overlap_;
  bool lane1_unjoined_ = false;     // lane 1 holds launches lane 0 has not waited for
  bool ordinary_unjoined_ = false;  // lane 0 holds ordinary work lane 1 has not waited for
};

}  // namespace vxlanes

#endif
