/*
 * coarse_sched.h — which workgroup of the persistent coarse kernel takes
 * which channel, and in what order (coarse.hip; modelled on the CPU by
 * tools/coarse_sched_sim.cpp, tests/test_coarse_sched.py).
 *
 * A launch has grid(nch, G) workgroups.  Workgroup b owns the channels
 * b, b + grid, b + 2 grid, ... (iters(nch, grid, b) of them, numbered k).
 * It looks at them BATCH at a time: lane l of every wave evaluates "hop due"
 * for k = k0 + l, a ballot makes the batch's mask, and the workgroup walks
 * the set bits from the lowest (first / rest).  While it works on one due
 * channel it already loads the state of the next one of the same batch
 * (mask still nonzero after rest); the first due channel of a batch has no
 * such predecessor and the last no successor.
 *
 * Plain integer arithmetic only: this header is compiled for the device and
 * for the host model.
 */
#pragma once

#if defined(__HIPCC__)
#define CSCHED_FN __host__ __device__ inline
#else
#define CSCHED_FN inline
#endif

namespace aero {
namespace csched {

constexpr int BATCH = 64;  // one lane per channel of a batch

// workgroups of a launch over nch channels with at most G resident (G >= 1)
CSCHED_FN int grid(int nch, int G) { return nch < G ? nch : G; }
// channels workgroup b owns
CSCHED_FN int iters(int nch, int grid, int b) { return b < nch ? (nch - b + grid - 1) / grid : 0; }
// its k-th channel
CSCHED_FN int channel(int grid, int b, int k) { return b + k * grid; }
// does lane l of the batch starting at k0 have a channel?
CSCHED_FN bool lane_has(int iters, int k0, int l) { return k0 + l < iters; }
// the walk over a batch's due mask (mask != 0)
CSCHED_FN int first(unsigned long long mask) { return __builtin_ctzll(mask); }
CSCHED_FN unsigned long long rest(unsigned long long mask) { return mask & (mask - 1); }

}  // namespace csched
}  // namespace aero
