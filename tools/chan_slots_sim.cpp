// Host walk of the channeliser's run-time VFO bookkeeping
// (aero-cli_amd/csrc/chan_slots.h) for tests/test_chan_start_model.py: a
// script of id takes / releases, a script of slot puts / takes per shape, and
// the settle bound.
#include <cstddef>

#include "../aero-cli_amd/csrc/chan_slots.h"

using namespace aero::cslots;

// ops[i] == -1: take an id (out[i] = the id); ops[i] >= 0: release that id
// (out[i] = 1 if it was in use).  counts[i] = one past the largest id in use
// after step i.
extern "C" void chan_ids_sim(const int *ops, int n, int *out, int *counts) {
  IdAlloc ids;
  for (int i = 0; i < n; ++i) {
    out[i] = ops[i] < 0 ? ids.take() : (int)ids.release(ops[i]);
    counts[i] = ids.count();
  }
}

// ops[i] = {op, slot, parent, k, late, spb, S, out_rate, filterbw}; op 0 puts
// `slot` on its shape's free list (out[i] = 0), op 1 takes one of that shape
// (out[i] = the slot or -1).  nfree[i] = free slots held after step i.
extern "C" void chan_pool_sim(const int *ops, int n, int *out, int *nfree) {
  SlotPool pool;
  for (int i = 0; i < n; ++i) {
    const int *o = ops + 9 * i;
    const Shape s{o[2], o[3], o[4], o[5], o[6], o[7], o[8]};
    if (o[0] == 0) {
      pool.put(s, o[1]);
      out[i] = 0;
    } else {
      out[i] = pool.take(s);
    }
    nfree[i] = (int)pool.free_count();
  }
}

extern "C" long long chan_settle_sim(int nusb, int nlate, int late, int k, int main_k) {
  return (long long)settle(nusb, nlate, late, k, main_k);
}
