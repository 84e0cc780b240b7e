/*
 * slot_reset.hip — returns a batch of channel slots of one group's device
 * pool to a new channel's state in one launch: every per-channel array of the
 * reset plan (slot_reset.h) zeroed, the scalar fields set to their initial
 * values.  Used when a closed channel's slot (aero_channel_close, an MSK rate
 * change) is given back to the group.
 *
 * grid.y is the plan entry, grid.x strides over its work items:
 *   RS_COL (time-major [rows][C]): item = (row, slot index, 16-byte unit of
 *     the element), unit fastest, then the slot index.  The slot list is
 *     sorted, so neighbouring lanes write neighbouring slots of one row and a
 *     run of closed neighbours is one contiguous store per wave; a lone slot
 *     is one strided store per row.
 *   RS_ROW (channel-major [C][len]): item = (slot index, 16-byte chunk of the
 *     slot's run); the chunks are 16-byte aligned in the pool, the partial
 *     ones at the two ends of a run whose length or start is not a multiple
 *     of 16 (uint8 rows) are written byte by byte, so a neighbour's bytes are
 *     never touched.
 */
#include <hip/hip_runtime.h>

#include "slot_reset.h"

namespace aero {

namespace {

__global__ __launch_bounds__(256) void reset_slots_kernel(char *pool, const ResetSeg *segs, const int *slots,
                                                          const int *variant, int nslots, const ResetInit *inits) {
  const ResetSeg s = segs[blockIdx.y];
  const unsigned long long tid = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x;
  const unsigned long long nthr = (unsigned long long)gridDim.x * blockDim.x;
  if (s.kind == RS_COL) {
    const unsigned unit = s.elem < 16 ? s.elem : 16, nun = s.elem / unit;
    const unsigned long long per_row = (unsigned long long)nslots * nun, total = per_row * s.rows;
    for (unsigned long long k = tid; k < total; k += nthr) {
      const unsigned long long r = k / per_row, q = k - r * per_row;
      const unsigned j = (unsigned)(q / nun), u = (unsigned)(q - (unsigned long long)j * nun);
      char *dst = pool + s.off + r * s.pitch + (unsigned long long)slots[j] * s.elem + (unsigned long long)u * unit;
      if (unit == 16) {
        *reinterpret_cast<uint4 *>(dst) = make_uint4(0, 0, 0, 0);
      } else if (unit == 8) {
        *reinterpret_cast<double *>(dst) = s.fill == RF_DS ? inits[variant[j]].ds[r] : 0.0;
      } else if (unit == 4) {
        *reinterpret_cast<int *>(dst) = s.fill == RF_IS ? inits[variant[j]].is[r] : 0;
      } else {
        *reinterpret_cast<unsigned short *>(dst) = 0;
      }
    }
  } else if (s.kind == RS_ROW) {
    const unsigned long long W = (unsigned long long)s.elem / 16 + 2;  // aligned chunks a run can overlap
    const unsigned long long total = W * nslots;
    for (unsigned long long k = tid; k < total; k += nthr) {
      const unsigned long long j = k / W, i = k - j * W;
      const unsigned long long start = s.off + (unsigned long long)slots[j] * s.elem, end = start + s.elem;
      const unsigned long long lo = (start & ~15ull) + 16 * i, hi = lo + 16;
      if (lo >= end) continue;
      if (lo >= start && hi <= end) {
        *reinterpret_cast<uint4 *>(pool + lo) = make_uint4(0, 0, 0, 0);
      } else {
        const unsigned long long a = lo > start ? lo : start, b = hi < end ? hi : end;
        for (unsigned long long x = a; x < b; x++) pool[x] = 0;
      }
    }
  }
}

}  // namespace

// d_segs: the plan (nseg entries); d_slots / d_variant: nslots sorted slots
// and the index of each one's scalar init in d_inits
void launch_reset_slots(hipStream_t st, void *pool, const ResetSeg *d_segs, int nseg, const int *d_slots,
                        const int *d_variant, int nslots, const ResetInit *d_inits, unsigned long long max_items) {
  if (nseg <= 0 || nslots <= 0) return;
  const unsigned long long blocks = (max_items + 255) / 256;
  const unsigned gx = (unsigned)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));
  hipLaunchKernelGGL(reset_slots_kernel, dim3(gx, (unsigned)nseg), dim3(256), 0, st, reinterpret_cast<char *>(pool),
                     d_segs, d_slots, d_variant, nslots, d_inits);
}

}  // namespace aero
