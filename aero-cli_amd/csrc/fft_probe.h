// fft_probe.hip's entry points (diagnostic: aero_device_fft in engine.hip)
#pragma once
#include <hip/hip_runtime.h>

namespace aero {

constexpr int FP_MAX_REC = 256;  // records of one launch (16384 points: 64 MiB each way)

// Whether production builds the transform: fft_dit<L, INV> for L = 12, 13
// (both directions) and 14 (forward); chain::fft for L = 13, 14 at a depth of
// 1, 2 or 3 (the depth of a dit transform is not looked at)
bool fft_probe_known(int kind, int log2n, int inverse, int depth);

// One workgroup of 2^(log2n - 4) threads per record: `in` and `out` hold nrec
// records of 2^log2n complex values in natural order.  tw / twi: this size's
// host_twiddles tables, twg / twgi: their fftl::twg_build copies (chain
// only).  The caller has validated the arguments with fft_probe_known.
void launch_fft_probe(hipStream_t st, int kind, int log2n, int inverse, int depth, int start, int stop,
                      const double2 *in, int nrec, double2 *out, const double2 *tw, const double2 *twi,
                      const double2 *twg, const double2 *twgi);

}  // namespace aero
