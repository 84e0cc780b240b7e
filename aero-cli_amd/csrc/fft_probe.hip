/*
 * fft_probe.hip — diagnostic only (aero_device_fft, tests/test_gpu_fft.py)
 *
 * Runs the device transforms on values the caller hands over, so the tests
 * can compare every output value with the oracle's JFFT on input the
 * synthetic streams never produce (impulses, single bins, zeros, the ends of
 * the exponent range).  One workgroup per record, with the thread count and
 * launch bounds of the production kernel that runs the same transform:
 *
 *  dit    fft_dit<L, INV> as cchan.hip (L = 12, both directions), burst.hip's
 *         Hilbert fast-FIR (13, both) and the trident checks (14, forward)
 *         instantiate it: loaded bit-reversed into layout 0, read out of the
 *         final layout.  The inverse is JFFT's sum without its 1/N.
 *  chain  chain::fft (fft_chain.h) strung together as coarse_kernel does:
 *         depth 1  fft<L, true, false>
 *         depth 2  bins start..stop zeroed, fft<L, false, true> (no 1/N, no N:
 *                  the kernel skips both)
 *         depth 3  the values squared with the kernel's expression,
 *                  fft<L, false, false>
 *         The load (epos<L, 0>, bitrev) and the read-out (out_bin_thread |
 *         out_bin_reg) restate coarse.hip's: the kernel computes them from a
 *         thread index it reads anew per channel and interleaves them with
 *         its ring image, and it is left as it is.  The production copy of
 *         both is covered by the y comparison of tests/test_gpu_coarse_y.py.
 */
#include <hip/hip_runtime.h>

#include "../../include/aero_engine.h"
#include "fft_chain.h"
#include "fft_dit.h"
#include "fft_probe.h"

namespace aero {

namespace {

template <int L>
constexpr int dit_min_blocks() {
  return L == 12 ? 2 : 1;  // prefilter_blk_kernel; hilbert_kernel and trident_kernel give none
}

template <int L, bool INV>
__global__ __launch_bounds__(1 << (L - 4), dit_min_blocks<L>()) void fprobe_dit_kernel(const double2 *in, double2 *out,
                                                                                       const double2 *tw,
                                                                                       const double2 *twd) {
  constexpr int N = 1 << L, FT = N / 16, PADDED = N + N / 16;
  constexpr int LAST = L == 12 ? 2 : 3;  // the layout fft_dit leaves
  __shared__ double lds[PADDED];
  __shared__ double2 s_tw[TwLds<L>::LEN];
  const int t = threadIdx.x;
  const size_t rec = (size_t)blockIdx.x * N;
  load_tw_lds<L>(s_tw, tw, t, FT);
  __syncthreads();
  double2 x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = in[rec + bitrev<L>(epos<L, 0>(t, i))];
  fft_dit<L, INV>(x, t, lds, twd, s_tw);
#pragma unroll
  for (int i = 0; i < 16; ++i) out[rec + epos<L, LAST>(t, i)] = x[i];
}

template <int L>
__global__ __launch_bounds__(1 << (L - 4), L == 13 ? 4 : 1) void fprobe_chain_kernel(
    const double2 *in, double2 *out, int depth, int start, int stop, const double2 *tw, const double2 *twi,
    const double2 *twg, const double2 *twgi) {
  constexpr int N = 1 << L, FT = N / 16, PADDED = N + N / 16;
  static_assert(PADDED >= (FT / 64) * fftl::WL_REGION && PADDED >= fftl::gidx(N - 1) + 1, "the exchanges fit");
  __shared__ double lds[PADDED];
  __shared__ double2 s_tw[TwLds<L>::LEN];
  const int t = threadIdx.x;
  const size_t rec = (size_t)blockIdx.x * N;
  load_tw_lds<L>(s_tw, tw, t, FT);
  __syncthreads();
  double2 x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = in[rec + bitrev<L>(epos<L, 0>(t, i))];
  chain::fft<L, true, false>(x, t, lds, tw, s_tw, twg);
  const int bin_t = chain::out_bin_thread<L>(t);
  if (depth >= 2) {  // uniform: every thread meets the same barriers
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int p = bin_t | chain::out_bin_reg<L>(i);
      if (p >= start && p <= stop) x[i] = make_double2(0.0, 0.0);
    }
    chain::fft<L, false, true>(x, t, lds, twi, s_tw, twgi);
  }
  if (depth >= 3) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const double r = x[i].x * x[i].x - x[i].y * x[i].y;
      const double im = 2.0 * (x[i].x * x[i].y);
      x[i] = make_double2(r, im);
    }
    chain::fft<L, false, false>(x, t, lds, tw, s_tw, twg);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) out[rec + (bin_t | chain::out_bin_reg<L>(i))] = x[i];
}

}  // namespace

bool fft_probe_known(int kind, int log2n, int inverse, int depth) {
  if (inverse != 0 && inverse != 1) return false;
  if (kind == AERO_FFT_DIT) return log2n == 12 || log2n == 13 || (log2n == 14 && !inverse);
  if (kind == AERO_FFT_CHAIN) return (log2n == 13 || log2n == 14) && !inverse && depth >= 1 && depth <= 3;
  return false;
}

void launch_fft_probe(hipStream_t st, int kind, int log2n, int inverse, int depth, int start, int stop,
                      const double2 *in, int nrec, double2 *out, const double2 *tw, const double2 *twi,
                      const double2 *twg, const double2 *twgi) {
  const dim3 g(nrec), b(1 << (log2n - 4));
  if (kind == AERO_FFT_DIT) {
    if (log2n == 12 && !inverse) hipLaunchKernelGGL((fprobe_dit_kernel<12, false>), g, b, 0, st, in, out, tw, tw);
    if (log2n == 12 && inverse) hipLaunchKernelGGL((fprobe_dit_kernel<12, true>), g, b, 0, st, in, out, tw, twi);
    if (log2n == 13 && !inverse) hipLaunchKernelGGL((fprobe_dit_kernel<13, false>), g, b, 0, st, in, out, tw, tw);
    if (log2n == 13 && inverse) hipLaunchKernelGGL((fprobe_dit_kernel<13, true>), g, b, 0, st, in, out, tw, twi);
    if (log2n == 14 && !inverse) hipLaunchKernelGGL((fprobe_dit_kernel<14, false>), g, b, 0, st, in, out, tw, tw);
  } else if (kind == AERO_FFT_CHAIN) {
    if (log2n == 13)
      hipLaunchKernelGGL(fprobe_chain_kernel<13>, g, b, 0, st, in, out, depth, start, stop, tw, twi, twg, twgi);
    if (log2n == 14)
      hipLaunchKernelGGL(fprobe_chain_kernel<14>, g, b, 0, st, in, out, depth, start, stop, tw, twi, twg, twgi);
  }
}

}  // namespace aero
