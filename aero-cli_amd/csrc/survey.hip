/*
 * survey.hip — the channeliser's wideband carrier survey (aero_chan_survey_*,
 * include/aero_chan.h): an averaged power spectrum of the CF32 stream the
 * VFOs read, which is in HBM already.
 *
 * The stream is cut into segments of N = 4096, 8192 or 16384 samples on a
 * grid that starts with the first read after the survey was started.  No read
 * length is a multiple of N, so a segment straddles reads, batches and
 * aero_chan_run calls: the unfinished tail (< N samples) stays in a carry
 * buffer, and a run's logical stream is that buffer followed by the run's
 * input.  Per segment, all in FP64 without contraction:
 *   x[i] = (double)re[i] * w[i], (double)im[i] * w[i]   (no product without a window)
 *   X    = fft_dit<log2n, false>(x)                      JFFT's forward transform, bit for bit
 *   p[k] = X[k].re * X[k].re + X[k].im * X[k].im         natural bin order
 *   acc[k] = acc[k] + p[k]                               in stream order
 *
 *   survey_seg_kernel   one workgroup of N/16 threads per segment, as the
 *                       other users of fft_dit (16 values per thread, loaded
 *                       bit-reversed into layout 0, converted and windowed on
 *                       the way); writes p to a scratch row per segment
 *   survey_fold_kernel  one lane per bin walks the run's rows in segment
 *                       order, so the sum is the sequential one; the same
 *                       launch copies the new tail into the carry buffer
 * Two launches per run, on the channeliser's stream after dc_kernel.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../include/aero_engine.h"
#include "fft_dit.h"
#include "survey.h"
#include "tables_host.h"

namespace aero {

namespace {

#define CHK(x)                                                                         \
  do {                                                                                 \
    hipError_t err__ = (x);                                                            \
    if (err__ != hipSuccess) {                                                         \
      fprintf(stderr, "aero_chan: %s failed: %s\n", #x, hipGetErrorString(err__));     \
      return AERO_E_HIP;                                                               \
    }                                                                                  \
  } while (0)

constexpr int FOLD_TILE = 256;

// Segment blockIdx.x of the logical stream carry[0 .. ncarry) ++ in[...].
// LDS: N + N/16 doubles of exchange buffer plus TwLds<L> (43 / 78 / 152 KiB
// for L = 12 / 13 / 14: three, two and one workgroup per CU).
template <int L>
__global__ __launch_bounds__(1 << (L - 4), L == 12 ? 2 : 1) void survey_seg_kernel(
    const float2 *__restrict__ carry, long long ncarry, const float2 *__restrict__ in,
    const double *__restrict__ win, double *__restrict__ P, const double2 *__restrict__ tw) {
  constexpr int N = 1 << L, FT = N / 16, PADDED = N + N / 16;
  constexpr int LAST = L == 12 ? 2 : 3;  // the layout fft_dit leaves
  __shared__ double lds[PADDED];
  __shared__ double2 s_tw[TwLds<L>::LEN];
  const int t = threadIdx.x;
  const long long base = (long long)blockIdx.x * N;
  load_tw_lds<L>(s_tw, tw, t, FT);
  __syncthreads();
  double2 x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int p = bitrev<L>(epos<L, 0>(t, i));
    const long long j = base + p;
    const float2 v = j < ncarry ? carry[j] : in[j - ncarry];
    double re = (double)v.x, im = (double)v.y;
    if (win) {  // uniform
      const double w = win[p];
      re = re * w;
      im = im * w;
    }
    x[i] = make_double2(re, im);
  }
  fft_dit<L, false>(x, t, lds, tw, s_tw);
  double *row = P + (size_t)blockIdx.x * N;
#pragma unroll
  for (int i = 0; i < 16; ++i) row[epos<L, LAST>(t, i)] = x[i].x * x[i].x + x[i].y * x[i].y;
}

// acc[k] += P[0][k], P[1][k], ... in that order; carry[dst0 + k] = src[k] for
// the ntail (< N) samples of the new tail.  N / FOLD_TILE workgroups.
__global__ __launch_bounds__(FOLD_TILE) void survey_fold_kernel(double *__restrict__ acc, const double *__restrict__ P,
                                                               int N, int nseg, float2 *__restrict__ carry,
                                                               const float2 *__restrict__ src, int ntail, int dst0) {
  const int k = blockIdx.x * FOLD_TILE + threadIdx.x;
  if (nseg) {
    double a = acc[k];
    for (int s = 0; s < nseg; s++) a = a + P[(size_t)s * N + k];
    acc[k] = a;
  }
  if (k < ntail) carry[dst0 + k] = src[k];
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

struct Survey {
  int log2n = 0, N = 0;
  long long max_samples = 0, max_seg = 0;
  char *mem = nullptr;
  size_t bytes = 0;
  float2 *carry = nullptr;
  double *acc = nullptr, *win = nullptr, *P = nullptr;
  double2 *tw = nullptr;
  long long ncarry = 0;   // samples in the carry buffer (< N)
  uint64_t in_acc = 0;    // segments in acc
};

int survey_create(int log2n, const double *window, long long max_samples, Survey **out) {
  if (!out || max_samples < 1 || (log2n != 12 && log2n != 13 && log2n != 14)) return AERO_E_INVALID;
  *out = nullptr;
  Survey *s = new Survey();
  s->log2n = log2n;
  const size_t N = (size_t)1 << log2n;
  s->N = (int)N;
  s->max_samples = max_samples;
  s->max_seg = (long long)((N - 1 + (size_t)max_samples) / N);  // a full tail before the largest run
  const size_t o_carry = 0, o_acc = align256(o_carry + N * sizeof(float2)), o_win = align256(o_acc + N * sizeof(double)),
               o_tw = align256(o_win + (window ? N * sizeof(double) : 0)), o_P = align256(o_tw + N * sizeof(double2));
  s->bytes = o_P + (size_t)std::max<long long>(s->max_seg, 1) * N * sizeof(double);
  if (hipMalloc(reinterpret_cast<void **>(&s->mem), s->bytes) != hipSuccess) {
    delete s;
    return AERO_E_NOMEM;
  }
  s->carry = reinterpret_cast<float2 *>(s->mem + o_carry);
  s->acc = reinterpret_cast<double *>(s->mem + o_acc);
  s->win = window ? reinterpret_cast<double *>(s->mem + o_win) : nullptr;
  s->tw = reinterpret_cast<double2 *>(s->mem + o_tw);
  s->P = reinterpret_cast<double *>(s->mem + o_P);
  std::vector<double> tw(2 * N), twi(2 * N);
  host_twiddles((int)N, tw.data(), twi.data());  // JFFT::init, as every user of fft_dit sets them up
  hipError_t e = hipMemset(s->mem, 0, o_P);
  if (e == hipSuccess && window) e = hipMemcpy(s->win, window, N * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s->tw, tw.data(), N * sizeof(double2), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    fprintf(stderr, "aero_chan: survey setup failed: %s\n", hipGetErrorString(e));
    (void)hipFree(s->mem);
    delete s;
    return AERO_E_HIP;
  }
  *out = s;
  return AERO_OK;
}

void survey_destroy(Survey *s) {
  if (!s) return;
  (void)hipDeviceSynchronize();
  (void)hipFree(s->mem);
  delete s;
}

size_t survey_bytes(const Survey *s) { return s ? s->bytes : 0; }

int survey_run(Survey *s, hipStream_t st, const float2 *in, long long n, int *launches, uint64_t *segments) {
  if (!s || !in || n < 0 || n > s->max_samples) return AERO_E_INVALID;
  const long long N = s->N, total = s->ncarry + n, nseg = total / N;
  if (nseg > s->max_seg) return AERO_E_INVALID;  // sized at create
  int nl = 0;
  if (nseg) {
    const dim3 g((unsigned)nseg), b((unsigned)(N / 16));
    if (s->log2n == 12) hipLaunchKernelGGL(survey_seg_kernel<12>, g, b, 0, st, s->carry, s->ncarry, in, s->win, s->P, s->tw);
    if (s->log2n == 13) hipLaunchKernelGGL(survey_seg_kernel<13>, g, b, 0, st, s->carry, s->ncarry, in, s->win, s->P, s->tw);
    if (s->log2n == 14) hipLaunchKernelGGL(survey_seg_kernel<14>, g, b, 0, st, s->carry, s->ncarry, in, s->win, s->P, s->tw);
    nl++;
  }
  // the new tail: behind the last whole segment, which lies in `in` once a
  // segment was completed (nseg * N >= N > ncarry); else this input is appended
  const long long ntail = total - nseg * N;
  const float2 *src = nseg ? in + (nseg * N - s->ncarry) : in;
  const int dst0 = nseg ? 0 : (int)s->ncarry, ncopy = nseg ? (int)ntail : (int)n;
  if (nseg || ncopy) {
    hipLaunchKernelGGL(survey_fold_kernel, dim3((unsigned)(N / FOLD_TILE)), dim3(FOLD_TILE), 0, st, s->acc, s->P, (int)N,
                       (int)nseg, s->carry, src, ncopy, dst0);
    nl++;
  }
  CHK(hipGetLastError());
  s->ncarry = ntail;
  s->in_acc += (uint64_t)nseg;
  if (launches) *launches = nl;
  if (segments) *segments = (uint64_t)nseg;
  return AERO_OK;
}

int survey_read(Survey *s, hipStream_t st, double *power, size_t cap, uint64_t *segments, int reset) {
  if (!s || !power || !segments || cap < (size_t)s->N) return AERO_E_INVALID;
  CHK(hipMemcpyAsync(power, s->acc, (size_t)s->N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (reset) CHK(hipMemsetAsync(s->acc, 0, (size_t)s->N * sizeof(double), st));
  CHK(hipStreamSynchronize(st));
  *segments = s->in_acc;
  if (reset) s->in_acc = 0;
  return AERO_OK;
}

}  // namespace aero
