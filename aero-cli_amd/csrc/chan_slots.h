/*
 * chan_slots.h — host bookkeeping of the channeliser's run-time VFOs
 * (chan.hip; walked on the CPU by tools/chan_slots_sim.cpp): the [vfos] id
 * allocator, the free lists of device slots per shape and the settle bound.
 * No HIP in here.
 */
#ifndef AERO_CHAN_SLOTS_H
#define AERO_CHAN_SLOTS_H

#include <cstddef>
#include <map>
#include <set>
#include <tuple>
#include <vector>

namespace aero {
namespace cslots {

// [vfos] ids: the smallest free one is given out, a released one again
class IdAlloc {
 public:
  int take() {
    int id;
    if (free_.empty()) {
      id = (int)used_.size();
      used_.push_back(1);
    } else {
      id = *free_.begin();
      free_.erase(free_.begin());
      used_[id] = 1;
    }
    return id;
  }
  bool release(int id) {
    if (!in_use(id)) return false;
    used_[id] = 0;
    free_.insert(id);
    // ids past the largest one in use are handed out by growth again
    while (!used_.empty() && !used_.back()) {
      free_.erase((int)used_.size() - 1);
      used_.pop_back();
    }
    return true;
  }
  bool in_use(int id) const { return id >= 0 && id < (int)used_.size() && used_[id]; }
  int count() const { return (int)used_.size(); }  // one past the largest id in use

 private:
  std::vector<char> used_;
  std::set<int> free_;
};

// Everything that sizes a sub-VFO's device slot or fills its constant data
// (Hilbert, late and audio taps).  The tap counts are functions of out_rate,
// late and filterbw (firfilter's compute_ntaps), so they need no field.
struct Shape {
  int parent, k, late, spb, S, out_rate, filterbw;
  std::tuple<int, int, int, int, int, int, int> key() const {
    return std::make_tuple(parent, k, late, spb, S, out_rate, filterbw);
  }
  bool operator<(const Shape &o) const { return key() < o.key(); }
  bool operator==(const Shape &o) const { return key() == o.key(); }
};

// free slots per shape, reused smallest index first
class SlotPool {
 public:
  void put(const Shape &s, int slot) { free_[s].insert(slot); }
  int take(const Shape &s) {  // -1: none of this shape
    auto it = free_.find(s);
    if (it == free_.end() || it->second.empty()) return -1;
    const int slot = *it->second.begin();
    it->second.erase(it->second.begin());
    return slot;
  }
  size_t free_count() const {
    size_t n = 0;
    for (auto &kv : free_) n += kv.second.size();
    return n;
  }

 private:
  std::map<Shape, std::set<int>> free_;
};

// Output samples after a start within which a sub-VFO may differ from one
// that was always there.  Every stage has finite memory: a half-band stage
// looks back 11 inputs plus the copy-back's one-early slot, at most 12
// samples of its own rate and so of any later one (k of the VFO, main_k of a
// main VFO that starts with it); the late FIR nlate inputs = ceil(nlate/late)
// outputs; the Hilbert transformer 124; the audio FIR nusb.
inline size_t settle(int nusb, int nlate, int late, int k, int main_k) {
  size_t n = 124 + (size_t)nusb + 12 * (size_t)(k + main_k);
  if (late > 0) n += ((size_t)nlate + late - 1) / late;
  return n;
}

}  // namespace cslots
}  // namespace aero
#endif
