/*
 * slot_copy.hip — moves a batch of channel slots between one group's device
 * pool and a staging buffer in one launch (aero_channel_export /
 * aero_channel_import): pack_slots_kernel gathers every byte the plan gives
 * each listed slot into the staging buffer, unpack_slots_kernel scatters a
 * staging buffer into the listed slots.  The staging buffer holds the slots'
 * packed runs (slot_copy.h: plan order, rows x elem per RS_COL entry, elem per
 * RS_ROW entry) one after the other in slot-list order, `stride` bytes each,
 * so one copy moves the whole batch between it and the host.
 *
 * The work split is the reset kernel's (slot_reset.hip): grid.y is the plan
 * entry, grid.x strides over its items.
 *   RS_COL: item = (row, slot index, 16-byte unit of the element), the unit
 *     fastest, then the slot index.  The slot list is sorted, so neighbouring
 *     lanes touch neighbouring slots of one row: a run of neighbouring slots
 *     is one contiguous pool access per wave, a lone slot one strided access
 *     per row.
 *   RS_ROW: item = (slot index, 16-byte chunk of the slot's run), the chunks
 *     16-byte aligned in the pool; the partial chunks at the ends of a run
 *     whose start or length is no multiple of 16 (uint8 rows) move byte by
 *     byte, so a neighbour's bytes are never read into the staging buffer nor
 *     written.
 * The pool side of every unit is aligned to the unit (LayoutRec::add checks
 * the arrays).  The staging side is packed, so a unit may start at any byte
 * there: it moves as one access where its staging address is aligned, and in
 * 4-, 2- or 1-byte pieces where it is not.
 */
#include <hip/hip_runtime.h>

#include "../../include/aero_engine.h"
#include "slot_copy.h"

namespace aero {

namespace {

// n bytes (2, 4, 8 or 16) between the pool (aligned to n) and the staging buffer (any alignment)
template <bool PACK>
__device__ __forceinline__ void move_unit(char *pool, char *stg, unsigned n) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(stg);
  char *dst = PACK ? stg : pool;
  const char *src = PACK ? pool : stg;
  if ((a & (n - 1)) == 0) {
    if (n == 16)
      *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(src);
    else if (n == 8)
      *reinterpret_cast<uint2 *>(dst) = *reinterpret_cast<const uint2 *>(src);
    else if (n == 4)
      *reinterpret_cast<unsigned *>(dst) = *reinterpret_cast<const unsigned *>(src);
    else
      *reinterpret_cast<unsigned short *>(dst) = *reinterpret_cast<const unsigned short *>(src);
  } else if ((a & 3) == 0) {
    for (unsigned x = 0; x < n; x += 4)
      *reinterpret_cast<unsigned *>(dst + x) = *reinterpret_cast<const unsigned *>(src + x);
  } else if ((a & 1) == 0) {
    for (unsigned x = 0; x < n; x += 2)
      *reinterpret_cast<unsigned short *>(dst + x) = *reinterpret_cast<const unsigned short *>(src + x);
  } else {
    for (unsigned x = 0; x < n; x++) dst[x] = src[x];
  }
}

// segs: the copy plan (ResetSeg::bytes = the entry's offset in a packed slot)
template <bool PACK>
__device__ __forceinline__ void copy_slots(char *pool, char *stage, unsigned long long stride, const ResetSeg *segs,
                                           const int *slots, int nslots) {
  const ResetSeg s = segs[blockIdx.y];
  const unsigned long long tid = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x;
  const unsigned long long nthr = (unsigned long long)gridDim.x * blockDim.x;
  if (s.kind == RS_COL) {
    const unsigned unit = s.elem < 16 ? s.elem : 16, nun = s.elem / unit;
    const unsigned long long per_row = (unsigned long long)nslots * nun, total = per_row * s.rows;
    for (unsigned long long k = tid; k < total; k += nthr) {
      const unsigned long long r = k / per_row, q = k - r * per_row;
      const unsigned j = (unsigned)(q / nun), u = (unsigned)(q - (unsigned long long)j * nun);
      char *p = pool + s.off + r * s.pitch + (unsigned long long)slots[j] * s.elem + (unsigned long long)u * unit;
      char *g = stage + (unsigned long long)j * stride + s.bytes + r * s.elem + (unsigned long long)u * unit;
      move_unit<PACK>(p, g, unit);
    }
  } else if (s.kind == RS_ROW) {
    const unsigned long long W = (unsigned long long)s.elem / 16 + 2;  // aligned chunks a run can overlap
    const unsigned long long total = W * nslots;
    for (unsigned long long k = tid; k < total; k += nthr) {
      const unsigned long long j = k / W, i = k - j * W;
      const unsigned long long start = s.off + (unsigned long long)slots[j] * s.elem, end = start + s.elem;
      const unsigned long long lo = (start & ~15ull) + 16 * i, hi = lo + 16;
      if (lo >= end) continue;
      char *g0 = stage + j * stride + s.bytes;  // the run's first byte in the staging buffer
      if (lo >= start && hi <= end) {
        move_unit<PACK>(pool + lo, g0 + (lo - start), 16);
      } else {
        const unsigned long long a = lo > start ? lo : start, b = hi < end ? hi : end;
        for (unsigned long long x = a; x < b; x++) {
          if (PACK)
            g0[x - start] = pool[x];
          else
            pool[x] = g0[x - start];
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void pack_slots_kernel(char *pool, char *stage, unsigned long long stride,
                                                         const ResetSeg *segs, const int *slots, int nslots) {
  copy_slots<true>(pool, stage, stride, segs, slots, nslots);
}

__global__ __launch_bounds__(256) void unpack_slots_kernel(char *pool, char *stage, unsigned long long stride,
                                                           const ResetSeg *segs, const int *slots, int nslots) {
  copy_slots<false>(pool, stage, stride, segs, slots, nslots);
}

}  // namespace

// d_segs: the copy plan (nseg entries); d_slots: nslots sorted slots; stage:
// nslots x stride bytes; pack: pool -> stage, else stage -> pool
void launch_copy_slots(hipStream_t st, bool pack, void *pool, void *stage, unsigned long long stride,
                       const ResetSeg *d_segs, int nseg, const int *d_slots, int nslots,
                       unsigned long long max_items) {
  if (nseg <= 0 || nslots <= 0) return;
  const unsigned long long blocks = (max_items + 255) / 256;
  const unsigned gx = (unsigned)(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks));
  if (pack)
    hipLaunchKernelGGL(pack_slots_kernel, dim3(gx, (unsigned)nseg), dim3(256), 0, st,
                       reinterpret_cast<char *>(pool), reinterpret_cast<char *>(stage), stride, d_segs, d_slots, nslots);
  else
    hipLaunchKernelGGL(unpack_slots_kernel, dim3(gx, (unsigned)nseg), dim3(256), 0, st,
                       reinterpret_cast<char *>(pool), reinterpret_cast<char *>(stage), stride, d_segs, d_slots, nslots);
}

int slot_copier_run(SlotCopier &sc, hipStream_t st, bool pack, void *pool, int C,
                    const std::vector<ResetSeg> &reset_plan, const int *slots, int n, uint8_t *host,
                    float *kernel_ms) {
  if (n <= 0) return AERO_OK;
  if (n > C || !host || !pool) return AERO_E_INVALID;
  for (int i = 0; i < n; i++)  // sorted slots of this pool: the kernels index the pool with them
    if (slots[i] < 0 || slots[i] >= C || (i && slots[i] < slots[i - 1])) return AERO_E_INVALID;
  if (!sc.d_plan) {
    sc.plan = copy_plan(reset_plan);
    sc.stride = slot_bytes(reset_plan);
    if (sc.plan.empty() || !sc.stride) return AERO_E_INVALID;
    if (hipMalloc(&sc.d_slots, sizeof(int) * (size_t)C) != hipSuccess) return AERO_E_NOMEM;
    ResetSeg *d = nullptr;
    if (hipMalloc(&d, sizeof(ResetSeg) * sc.plan.size()) != hipSuccess) return AERO_E_NOMEM;
    if (hipMemcpy(d, sc.plan.data(), sizeof(ResetSeg) * sc.plan.size(), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(d);
      return AERO_E_HIP;
    }
    sc.d_plan = d;  // only now: the table is on the device
  }
  const size_t need = (size_t)n * sc.stride;
  if (need > sc.stage_cap) {
    if (sc.d_stage) (void)hipFree(sc.d_stage);
    sc.d_stage = nullptr;
    sc.stage_cap = 0;
    if (hipMalloc(&sc.d_stage, need) != hipSuccess) return AERO_E_NOMEM;
    sc.stage_cap = need;
  }
  hipEvent_t a = nullptr, b = nullptr;
  auto fail = [&](int rc) {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
    return rc;
  };
  if (hipMemcpyAsync(sc.d_slots, slots, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st) != hipSuccess)
    return AERO_E_HIP;
  if (!pack && hipMemcpyAsync(sc.d_stage, host, need, hipMemcpyHostToDevice, st) != hipSuccess) return AERO_E_HIP;
  if (kernel_ms) {
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return fail(AERO_E_HIP);
    (void)hipEventRecord(a, st);
  }
  launch_copy_slots(st, pack, pool, sc.d_stage, sc.stride, sc.d_plan, (int)sc.plan.size(), sc.d_slots, n,
                    reset_items(reset_plan, n));
  if (kernel_ms) (void)hipEventRecord(b, st);
  if (hipGetLastError() != hipSuccess) return fail(AERO_E_HIP);
  sc.launches++;
  if (pack && hipMemcpyAsync(host, sc.d_stage, need, hipMemcpyDeviceToHost, st) != hipSuccess) return fail(AERO_E_HIP);
  if (hipStreamSynchronize(st) != hipSuccess) return fail(AERO_E_HIP);
  if (kernel_ms) {
    *kernel_ms = 0;
    (void)hipEventElapsedTime(kernel_ms, a, b);
  }
  // a large batch's staging is not kept
  if (sc.stage_cap > ((size_t)64 << 20)) {
    (void)hipFree(sc.d_stage);
    sc.d_stage = nullptr;
    sc.stage_cap = 0;
  }
  return fail(AERO_OK);
}

void slot_copier_free(SlotCopier &sc) {
  if (sc.d_plan) (void)hipFree(sc.d_plan);
  if (sc.d_slots) (void)hipFree(sc.d_slots);
  if (sc.d_stage) (void)hipFree(sc.d_stage);
  sc.d_plan = nullptr;
  sc.d_slots = nullptr;
  sc.d_stage = nullptr;
  sc.stage_cap = 0;
}

}  // namespace aero
