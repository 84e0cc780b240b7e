// dcd_host.h — AeroL's data-carrier-detect countdown on the host (no HIP).
//
// The framing of continuous MSK channels and of the C channel never reads
// datacd, so its countdown need not run on the device: the host keeps it
// beside the frames' SU CRCs (engine.hip process_slot).  The C channel's has
// always lived here (+2 / -5 per SU, decode/aerol.cpp:2300-2315); with
// AERO_F_DCD_TICK_CONT the 1 s timer (updateDCD, :1043-1058) runs on it too,
// and an MSK channel's countdown (sync: datacd = true, countdown 12,
// :2010-2012; +2 / -3 per SU, :1545-1556) joins it.
//
// One pass of one channel delivers, in stream order: its Viterbi jobs in list
// order (a frame end carries the frame's SU CRCs), the MSK framing kernel's
// UW syncs, each with the number of jobs the channel listed in the pass
// before it (DevState::syncs), and last the tick, because a flagged demod
// launch ends at the sample that fires the timer.
#pragma once
#include <cstdint>

namespace aero {

struct DcdHost {
  int cd = 0, dcd = 0, edges = 0;  // datacdcountdown, datacd, changes of datacd
  void set(int v) {
    if (dcd != v) edges++;
    dcd = v;
  }
  // AeroL::updateDCD: a countdown of 2 goes to -1 and is clamped only at the next tick
  void tick() {
    if (cd > 0)
      cd -= 3;
    else if (cd < 0)
      cd = 0;
    if (dcd && !cd) set(0);
  }
  void sync() {
    set(1);
    cd = 12;
  }
  // one SU's CRC result; `down`: 3 (AeroL::Decode) or 5 (DecodeC)
  void su(bool ok, int down) {
    if (ok) {
      if (cd < 12) cd += 2;
    } else {
      if (cd > 0) cd -= down;
    }
    if (!dcd && cd > 2) set(1);
  }
};

// a channel's walk through one pass's sync word
struct DcdPass {
  uint64_t syncs = 0;
  int done = 0, listed = 0;
  int count() const { return (int)(syncs & 15); }
  int before(int k) const { return (int)((syncs >> (4 + 2 * k)) & 3); }
  // the syncs that precede the channel's next job of the pass, then that job is counted
  void job(DcdHost &d) {
    while (done < count() && before(done) <= listed) {
      d.sync();
      done++;
    }
    listed++;
  }
  // the pass's remaining syncs, then its tick
  void finish(DcdHost &d, bool tick) {
    while (done < count()) {
      d.sync();
      done++;
    }
    if (tick) d.tick();
  }
};

}  // namespace aero
