// slot_reset.h — the reset plan of a group's device pool: which bytes belong
// to one channel slot, and what a new channel finds there.
//
// Both pool layouts (engine.hip layout(), burst_engine.hip burst_layout())
// carve their arrays through carve() below, which notes every array in a
// LayoutRec: its byte offset, how it is addressed per channel, and its fill.
// The per-channel entries of that record are the reset plan.  The reset
// kernel (slot_reset.hip) consumes the plan on the device; the host test
// entry aero_x_reset_plan reads the same record, so the addressing is pinned
// on the CPU (tests/test_channel_lifecycle_host.py).
//
// A per-channel array is addressed in one of two ways:
//   RS_COL  time-major [rows][C]: slot c owns `elem` bytes at
//           off + r * pitch + c * elem for every row r (pitch = elem * C);
//   RS_ROW  channel-major [C][len]: slot c owns the `elem` = len bytes at
//           off + c * elem (rows = 1).
// RS_SHARED arrays (tables, job lists, one-element placeholders of a mode
// that does not use the array) belong to no slot and are never reset.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace aero {

enum ResetKind : int { RS_SHARED = 0, RS_COL = 1, RS_ROW = 2 };
// RF_DS / RF_IS: row r is the double / int field r of the scalar init (ResetInit)
enum ResetFill : int { RF_ZERO = 0, RF_DS = 1, RF_IS = 2 };

struct ResetSeg {
  unsigned long long off;    // byte offset of the array in the pool
  unsigned long long pitch;  // bytes between a slot's rows (RS_COL), 0 for RS_ROW
  unsigned long long bytes;  // the whole array (every slot)
  unsigned elem;             // bytes a slot owns per row
  unsigned rows;
  int kind, fill;
};

// scalar init of a new channel (init_scalars / burst_open); a group holds one
// per variant (burst MSK: 600 and 1200 bps differ in one field)
constexpr int RESET_DS_MAX = 160, RESET_IS_MAX = 160;
struct ResetInit {
  double ds[RESET_DS_MAX];
  int is[RESET_IS_MAX];
};

struct LayoutRec {
  int C = 0;
  bool bad = false;  // an annotation that does not cover its array exactly
  std::vector<ResetSeg> segs;  // every carve, in pool order
  void add(size_t off, size_t bytes, int kind, size_t elem, size_t rows, int fill) {
    ResetSeg s{};
    s.off = off;
    s.bytes = bytes;
    s.kind = kind;
    s.fill = fill;
    if (kind == RS_COL) {
      s.elem = (unsigned)elem;
      s.rows = (unsigned)rows;
      s.pitch = (unsigned long long)elem * C;
      if (elem * rows * (size_t)C != bytes || off % elem) bad = true;
      if (elem != 2 && elem != 4 && elem != 8 && elem % 16) bad = true;
      if ((fill == RF_DS && (elem != 8 || rows > (size_t)RESET_DS_MAX)) ||
          (fill == RF_IS && (elem != 4 || rows > (size_t)RESET_IS_MAX)))
        bad = true;
    } else if (kind == RS_ROW) {
      s.elem = (unsigned)elem;
      s.rows = 1;
      if (elem * (size_t)C != bytes || fill != RF_ZERO) bad = true;
    }
    segs.push_back(s);
  }
};

// `count` elements of T from the pool, 256-byte aligned; noted in `rec`
template <class T>
T *carve(char *&p, char *base, size_t count, LayoutRec *rec = nullptr, int kind = RS_SHARED, size_t elem = 0,
         size_t rows = 0, int fill = RF_ZERO) {
  T *r = reinterpret_cast<T *>(p);
  if (rec) rec->add((size_t)(p - base), count * sizeof(T), kind, elem, rows, fill);
  p += (count * sizeof(T) + 255) & ~size_t(255);
  return r;
}

// the per-channel entries of a recorded layout
inline std::vector<ResetSeg> reset_plan(const LayoutRec &rec) {
  std::vector<ResetSeg> plan;
  for (const ResetSeg &s : rec.segs)
    if (s.kind != RS_SHARED && s.bytes) plan.push_back(s);  // (an array of no elements: a trace that is off)
  return plan;
}

// work items of the reset kernel's largest plan entry for n slots (its grid)
inline unsigned long long reset_items(const std::vector<ResetSeg> &plan, int n) {
  unsigned long long mx = 1;
  for (const ResetSeg &s : plan) {
    const unsigned long long per =
        s.kind == RS_COL ? (unsigned long long)s.rows * (s.elem < 16 ? 1 : s.elem / 16) : (unsigned long long)s.elem / 16 + 2;
    if (per * (unsigned long long)n > mx) mx = per * (unsigned long long)n;
  }
  return mx;
}

}  // namespace aero
