// slot_copy.h — a channel slot's device state as one run of bytes, and back.
//
// The reset plan (slot_reset.h) lists every byte a slot owns in its group's
// pool.  Packed, a slot is those bytes in plan order: for an RS_COL entry its
// `rows` elements of `elem` bytes, row after row; for an RS_ROW entry its
// `elem` bytes.  slot_bytes() is the length of that run, the device section
// of a channel blob (chan_blob.h); neither depends on the pool's channel count
// or on where the arrays lie, so a slot packed from one pool unpacks into any
// slot of another pool of the same kind and flags (plan_fingerprint()).
//
// pack_slot_host / unpack_slot_host below are the plain statement of that
// mapping over a host copy of a pool; the kernels of slot_copy.hip do the
// same for a sorted list of slots and a staging buffer that holds the slots'
// runs one after the other (slot list order).  The host test entries
// aero_x_slot_pack / aero_x_slot_unpack run the host form (no GPU).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "slot_reset.h"

namespace aero {

// bytes one slot owns per plan entry / in all
inline unsigned long long seg_slot_bytes(const ResetSeg &s) {
  return s.kind == RS_COL ? (unsigned long long)s.rows * s.elem : (unsigned long long)s.elem;
}
inline unsigned long long slot_bytes(const std::vector<ResetSeg> &plan) {
  unsigned long long n = 0;
  for (const ResetSeg &s : plan) n += seg_slot_bytes(s);
  return n;
}

// FNV-1a over the plan's (kind, elem, rows, fill) sequence: what a packed slot
// means.  Offsets, pitches and the channel count are left out (they may differ
// between the pool a slot comes from and the one it goes to).
inline uint64_t plan_fingerprint(const std::vector<ResetSeg> &plan) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&h](uint32_t v) {
    for (int k = 0; k < 4; k++) {
      h ^= (v >> (8 * k)) & 0xFF;
      h *= 1099511628211ull;
    }
  };
  for (const ResetSeg &s : plan) {
    mix((uint32_t)s.kind);
    mix(s.elem);
    mix(s.rows);
    mix((uint32_t)s.fill);
  }
  return h;
}

// the copy plan the kernels read: the reset plan with each entry's offset in
// a packed slot (ResetSeg::bytes is not used by the copy, so it carries it)
inline std::vector<ResetSeg> copy_plan(const std::vector<ResetSeg> &plan) {
  std::vector<ResetSeg> out = plan;
  unsigned long long at = 0;
  for (ResetSeg &s : out) {
    s.bytes = at;
    at += seg_slot_bytes(s);
  }
  return out;
}

// slot `slot` of the pool -> blob (slot_bytes(plan) bytes)
inline void pack_slot_host(const std::vector<ResetSeg> &plan, const uint8_t *pool, int slot, uint8_t *blob) {
  for (const ResetSeg &s : plan) {
    if (s.kind == RS_COL) {
      for (unsigned r = 0; r < s.rows; r++) {
        memcpy(blob, pool + s.off + (unsigned long long)r * s.pitch + (unsigned long long)slot * s.elem, s.elem);
        blob += s.elem;
      }
    } else {
      memcpy(blob, pool + s.off + (unsigned long long)slot * s.elem, s.elem);
      blob += s.elem;
    }
  }
}

// blob -> slot `slot` of the pool; no other byte of the pool is written
inline void unpack_slot_host(const std::vector<ResetSeg> &plan, uint8_t *pool, int slot, const uint8_t *blob) {
  for (const ResetSeg &s : plan) {
    if (s.kind == RS_COL) {
      for (unsigned r = 0; r < s.rows; r++) {
        memcpy(pool + s.off + (unsigned long long)r * s.pitch + (unsigned long long)slot * s.elem, blob, s.elem);
        blob += s.elem;
      }
    } else {
      memcpy(pool + s.off + (unsigned long long)slot * s.elem, blob, s.elem);
      blob += s.elem;
    }
  }
}

// The device side of a group's exports and imports (slot_copy.hip): the copy
// plan and slot list on the device and the staging buffer, made on first use.
struct SlotCopier {
  std::vector<ResetSeg> plan;  // copy_plan() of the group's reset plan
  unsigned long long stride = 0;  // slot_bytes(plan)
  ResetSeg *d_plan = nullptr;
  int *d_slots = nullptr;  // [C]
  void *d_stage = nullptr;
  size_t stage_cap = 0;
  uint64_t launches = 0;  // aero_stat "slot_copies"
};

}  // namespace aero

struct ihipStream_t;

namespace aero {

// One launch of the pack (pool -> host) or unpack (host -> pool) kernel on
// stream st for the n sorted slots of a pool of C channels, with the one copy
// between the staging buffer and `host` (n x stride bytes, slot-list order);
// returns after the stream has finished.  kernel_ms (AERO_F_TIMING): the
// kernel's HIP-event time.  Returns an AERO_E_* code.
int slot_copier_run(SlotCopier &sc, ihipStream_t *st, bool pack, void *pool, int C,
                    const std::vector<ResetSeg> &reset_plan, const int *slots, int n, uint8_t *host,
                    float *kernel_ms);
void slot_copier_free(SlotCopier &sc);

}  // namespace aero
