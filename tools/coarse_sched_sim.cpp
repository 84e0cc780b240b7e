// Host model of the persistent coarse kernel's channel schedule
// (aero-cli_amd/csrc/coarse_sched.h, walked as coarse.hip walks it): every
// workgroup of the launch scans its channels a batch at a time, one lane per
// channel, and visits the due ones from the lowest lane up; the state of the
// next due channel of the batch is loaded while the current one is worked on.
// tests/test_coarse_sched.py checks what it records.
#include <cstdint>

#include "../aero-cli_amd/csrc/coarse_sched.h"

using namespace aero;

// due[nch]: 1 where the channel's hop is due.  Outputs, per channel:
// visits[c] times visited, wg_of[c] the workgroup that looked at it in a
// batch scan (scans[c] times), seq[c] its place in that workgroup's walk,
// pre[c] 1 if its state was loaded under its predecessor's tail and 0 if it
// loaded it itself (-1: never visited).  Returns the number of workgroups,
// or -1 where the walk itself is inconsistent (a preload that is not used by
// the very next visit, a channel outside 0..nch-1).
extern "C" int coarse_sched_sim(int nch, int G, const uint8_t *due, int *visits, int *scans, int *wg_of, int *seq,
                                int *pre) {
  for (int c = 0; c < nch; ++c) {
    visits[c] = scans[c] = 0;
    wg_of[c] = seq[c] = pre[c] = -1;
  }
  const int wgs = csched::grid(nch, G);
  for (int wg = 0; wg < wgs; ++wg) {
    const int iters = csched::iters(nch, wgs, wg);
    int n = 0;
    for (int k0 = 0; k0 < iters; k0 += csched::BATCH) {
      unsigned long long mask = 0;  // the ballot
      for (int l = 0; l < csched::BATCH; ++l) {
        if (!csched::lane_has(iters, k0, l)) continue;
        const int c = csched::channel(wgs, wg, k0 + l);
        if (c < 0 || c >= nch) return -1;
        scans[c]++;
        wg_of[c] = wg;
        if (due[c]) mask |= 1ull << l;
      }
      int preloaded = -1;
      while (mask) {
        const int c = csched::channel(wgs, wg, k0 + csched::first(mask));
        mask = csched::rest(mask);
        if (c < 0 || c >= nch) return -1;
        if (preloaded >= 0 && preloaded != c) return -1;
        pre[c] = preloaded >= 0;
        visits[c]++;
        seq[c] = n++;
        preloaded = mask ? csched::channel(wgs, wg, k0 + csched::first(mask)) : -1;
      }
      if (preloaded >= 0) return -1;
    }
  }
  return wgs;
}
