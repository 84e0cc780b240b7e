// ebno.hip — per-channel Eb/N0: the reference's OQPSKEbNoMeasure over the AGC
// ring the demod kernels already keep (AERO_F_EBNO, ebno_kernel), and its
// MSKEbNoMeasure over a ring of its own (AERO_F_EBNO_MSK, ebno_msk_kernel,
// further down); both steps in ebno.h.
//
// Launched after the demod launch of an OQPSK or C group whose engine has the
// flag.  One lane per channel: the lane takes the samples the demod has
// consumed since the estimator's last launch, [done, LS_NSAMP), from the
// time-major ring S.agc[AGC_LEN][C] (a wave reads contiguous doubles per row)
// and leaves the two sums, the smoothed EbNo and the new done-count.  A demod
// launch covers at most the PCM ring (engine.hip PCM_CAP = 65536 samples), so
// the entries of its samples and the entries EBNO_LEN behind them are still
// in the ring (engine.hip asserts PCM_CAP <= AGC_LEN - EBNO_LEN; a lane that
// finds a longer span leaves its state alone).
//
// Only the sums and the 0.8 / 0.2 recurrence are serial.  The loop takes four
// samples a turn: their sums one after the other, then the four tebno values
// (two divisions by a constant, one IEEE division and a log10 each), which
// depend on nothing but their own sums and overlap in the pipeline, then the
// four recurrence steps.  The result is the serial one bit for bit: the same
// operations on the same operands.
#include <hip/hip_runtime.h>

#include "ebno.h"
#include "engine_common.h"

namespace aero {

namespace {

constexpr int EBNO_UNROLL = 4;
constexpr int EBNO_WG = 64;  // one wave a workgroup: 64 channels, spread over the CUs

__global__ __launch_bounds__(EBNO_WG) void ebno_kernel(EbnoDev E, const double *__restrict__ agc,
                                                       const int *__restrict__ agc_ptr,
                                                       const long long *__restrict__ nsamp_row, int C, int nch,
                                                       int agc_len, double fb, int hop) {
  const int c = blockIdx.x * EBNO_WG + threadIdx.x;
  if (c >= nch) return;
  const long long nsamp = nsamp_row[c], done = E.done[c];
  long long left = nsamp - done;
  // nothing new; or a span the ring no longer holds (no demod launch gives one)
  if (left <= 0 || left > (long long)(agc_len - EBNO_LEN)) return;
  double s1 = E.acc[c], s2 = E.acc[(size_t)C + c], eb = E.acc[(size_t)2 * C + c];
  int row = (int)((agc_ptr[c] - left % agc_len + agc_len) % agc_len);  // in [0, agc_len)
  auto older = [agc_len](int r) { return r >= EBNO_LEN ? r - EBNO_LEN : r - EBNO_LEN + agc_len; };
  auto next = [agc_len](int r) { return r + 1 == agc_len ? 0 : r + 1; };
  for (; left >= EBNO_UNROLL; left -= EBNO_UNROLL) {
    double a[EBNO_UNROLL], o[EBNO_UNROLL], q1[EBNO_UNROLL], q2[EBNO_UNROLL], t[EBNO_UNROLL];
#pragma unroll
    for (int k = 0; k < EBNO_UNROLL; ++k) {
      a[k] = agc[(size_t)row * C + c];
      o[k] = agc[(size_t)older(row) * C + c];
      row = next(row);
    }
#pragma unroll
    for (int k = 0; k < EBNO_UNROLL; ++k) {
      ebno_sums(s1, s2, a[k], o[k]);
      q1[k] = s1;
      q2[k] = s2;
    }
#pragma unroll
    for (int k = 0; k < EBNO_UNROLL; ++k) t[k] = ebno_tebno(q1[k], q2[k], fb);
#pragma unroll
    for (int k = 0; k < EBNO_UNROLL; ++k) eb = ebno_smooth(eb, t[k]);
  }
  for (; left > 0; --left) {
    eb = ebno_step(s1, s2, eb, agc[(size_t)row * C + c], agc[(size_t)older(row) * C + c], fb);
    row = next(row);
  }
  E.acc[c] = s1;
  E.acc[(size_t)C + c] = s2;
  E.acc[(size_t)2 * C + c] = eb;
  E.done[c] = nsamp;
  // the channel stands on a hop boundary: the value the reference emits with
  // that hop (FreqOffsetEstimateSlot runs before the hop sample's own Update,
  // decode/oqpskdemodulator.cpp:351-402, :614)
  if (E.tr && (nsamp + 1) % hop == 0) {
    const int k = E.tr_n[c];
    if (k < E.tr_cap) {
      double *r = E.tr + ((size_t)c * E.tr_cap + k) * 2;
      r[0] = (double)nsamp;
      r[1] = eb;
    }
    E.tr_n[c] = k + 1;
  }
}

// AERO_F_EBNO_MSK: MSKEbNoMeasure behind the demod launch of a continuous MSK
// group (ebno.h).  The MSK AGC ring S.agc[Fs][C] holds one second and the
// estimator's window is two, so the lane keeps the estimator's last 2 Fs inputs
// in a ring of its own, time-major [2 Fs][C] like the AGC ring: sample i of
// [done, LS_NSAMP) is read from the AGC ring's row i % Fs, the term the moving
// averages drop from the own ring's row i % (2 Fs), which the sample then
// takes.  A demod launch covers at most one hop (MSK_HOP samples, fewer than
// the smallest AGC ring: engine.hip asserts it), so the rows of one launch are
// distinct and the samples' AGC entries are all there; a lane that finds a
// span longer than the AGC ring leaves its state alone.  The loop is the OQPSK
// one: four samples a turn, their sums in order, their tebno values side by
// side, their recurrence steps in order: the serial result bit for bit.
__global__ __launch_bounds__(EBNO_WG) void ebno_msk_kernel(EbnoDev E, double *__restrict__ own,
                                                           const double *__restrict__ agc,
                                                           const long long *__restrict__ nsamp_row, int C, int nch,
                                                           int fs, int hop) {
  const int c = blockIdx.x * EBNO_WG + threadIdx.x;
  if (c >= nch) return;
  const long long nsamp = nsamp_row[c], done = E.done[c];
  long long left = nsamp - done;
  // nothing new; or a span the AGC ring no longer holds (no demod launch gives one), or a
  // count no estimator has (an imported slot's contents are not the engine's own)
  if (done < 0 || left <= 0 || left > (long long)fs) return;
  const int len = 2 * fs;
  // the reciprocal msk_ebno_div's contract asks for, and glibc's log10(2.0): once a launch
  const double dlen = (double)len, rlen = 1.0 / dlen, lg2 = aero_log10(2.0);
  double s1 = E.acc[c], s2 = E.acc[(size_t)C + c], eb = E.acc[(size_t)2 * C + c];
  int ar = (int)(done % fs), row = (int)(done % len);  // in [0, fs), [0, len)
  auto anext = [fs](int r) { return r + 1 == fs ? 0 : r + 1; };
  auto onext = [len](int r) { return r + 1 == len ? 0 : r + 1; };
  for (; left >= EBNO_UNROLL; left -= EBNO_UNROLL) {
    double a[EBNO_UNROLL], o[EBNO_UNROLL], q1[EBNO_UNROLL], q2[EBNO_UNROLL], t[EBNO_UNROLL];
#pragma unroll
    for (int k = 0; k < EBNO_UNROLL; ++k) {
      a[k] = agc[(size_t)ar * C + c];
      o[k] = own[(size_t)row * C + c];
      own[(size_t)row * C + c] = a[k];
      ar = anext(ar);
      row = onext(row);
    }
#pragma unroll
    for (int k = 0; k < EBNO_UNROLL; ++k) {
      ebno_sums(s1, s2, a[k], o[k]);
      q1[k] = s1;
      q2[k] = s2;
    }
#pragma unroll
    for (int k = 0; k < EBNO_UNROLL; ++k) t[k] = msk_ebno_tebno(q1[k], q2[k], dlen, rlen, lg2);
#pragma unroll
    for (int k = 0; k < EBNO_UNROLL; ++k) eb = ebno_smooth(eb, t[k]);
  }
  for (; left > 0; --left) {
    const double a = agc[(size_t)ar * C + c];
    eb = msk_ebno_step(s1, s2, eb, a, own[(size_t)row * C + c], dlen, rlen, lg2);
    own[(size_t)row * C + c] = a;
    ar = anext(ar);
    row = onext(row);
  }
  E.acc[c] = s1;
  E.acc[(size_t)C + c] = s2;
  E.acc[(size_t)2 * C + c] = eb;
  E.done[c] = nsamp;
  // the channel stands on a hop boundary: the value the reference emits with
  // that hop (FreqOffsetEstimateSlot, reached from the overlapped buffer before
  // the hop sample's own Update, decode/mskdemodulator.cpp:287-309, :461).
  // The index counts from the estimator's construction; the host adds the
  // samples of earlier rates as it does for the hop records
  if (E.tr && (nsamp + 1) % hop == 0) {
    const int k = E.tr_n[c];
    if (k < E.tr_cap) {
      double *r = E.tr + ((size_t)c * E.tr_cap + k) * 2;
      r[0] = (double)nsamp;
      r[1] = eb;
    }
    E.tr_n[c] = k + 1;
  }
}

}  // namespace

void launch_ebno_msk(hipStream_t st, const EbnoDev &E, double *own, const DevState &S, int nch) {
  if (nch <= 0) return;
  hipLaunchKernelGGL(ebno_msk_kernel, dim3((unsigned)((nch + EBNO_WG - 1) / EBNO_WG)), dim3(EBNO_WG), 0, st, E, own,
                     (const double *)S.agc, (const long long *)(S.ls + (size_t)LS_NSAMP * S.C), S.C, nch, S.g.fs,
                     S.g.hop);
}

void launch_ebno(hipStream_t st, const EbnoDev &E, const DevState &S, int nch, double fb) {
  if (nch <= 0) return;
  hipLaunchKernelGGL(ebno_kernel, dim3((unsigned)((nch + EBNO_WG - 1) / EBNO_WG)), dim3(EBNO_WG), 0, st, E,
                     (const double *)S.agc, (const int *)(S.is + (size_t)IS_AGC_PTR * S.C),
                     (const long long *)(S.ls + (size_t)LS_NSAMP * S.C), S.C, nch, S.g.agc_len, fb, S.g.hop);
}

}  // namespace aero
