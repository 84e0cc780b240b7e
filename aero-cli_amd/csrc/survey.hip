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
 *
 * The hold (aero_chan_survey_hold_*) runs beside it on the same rows: groups
 * of `group` consecutive segments, per bin the largest and the smallest group
 * sum, the number of group sums above a level and, optionally, a ring of the
 * last `rows` group sums.  A group straddles runs as a segment straddles
 * reads: the unfinished sum stays in gsum, the fill count on the host.
 *
 *   survey_hold_kernel  fold's shape: one lane per bin walks the run's rows in
 *                       segment order; a third launch behind the fold, only
 *                       while a hold is on and the run completed a segment
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
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

// Per bin k over the run's rows, in segment order: gsum += p; when the group's
// last segment is in (fill counts the segments in gsum at the start of the
// run), the sum goes to peak / low / busy and row `row` of the ring, and gsum
// starts again at +0.  fill, group, row and rows are uniform, so every branch
// on them is.  A NaN sum fails all three comparisons.  level == nullptr: busy
// is not counted; ring == nullptr: rows == 0.  N / FOLD_TILE workgroups.
__global__ __launch_bounds__(FOLD_TILE) void survey_hold_kernel(double *__restrict__ gsum, double *__restrict__ peak,
                                                               double *__restrict__ low, uint32_t *__restrict__ busy,
                                                               const double *__restrict__ level,
                                                               double *__restrict__ ring, const double *__restrict__ P,
                                                               int N, int nseg, int fill, int group, int row, int rows) {
  const int k = blockIdx.x * FOLD_TILE + threadIdx.x;
  double g = gsum[k], pk = peak[k], lo = low[k];
  uint32_t bz = busy[k];
  const double lv = level ? level[k] : __builtin_inf();
  for (int s = 0; s < nseg; s++) {
    g = g + P[(size_t)s * N + k];
    if (++fill < group) continue;
    if (g > pk) pk = g;
    if (g < lo) lo = g;
    if (g > lv) bz++;
    if (ring) {
      ring[(size_t)row * N + k] = g;
      if (++row == rows) row = 0;
    }
    g = 0.0;
    fill = 0;
  }
  gsum[k] = g;
  peak[k] = pk;
  low[k] = lo;
  busy[k] = bz;
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

}  // namespace

// peak, low and busy lie behind one another, and `init` holds their start
// values (+0, +infinity, 0) in the same layout: a reset is one copy
struct Hold {
  int group = 0, rows = 0;
  char *mem = nullptr;
  size_t bytes = 0, state_bytes = 0;
  double *gsum = nullptr, *peak = nullptr, *low = nullptr, *level = nullptr, *ring = nullptr;
  uint32_t *busy = nullptr;
  char *init = nullptr;
  int fill = 0;           // segments in gsum (< group)
  uint64_t gidx = 0;      // groups completed since the start
  uint64_t in_hold = 0;   // groups in peak / low / busy
};

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
  Hold *hold = nullptr;   // nullptr while none is on
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
  survey_hold_stop(s);
  (void)hipFree(s->mem);
  delete s;
}

size_t survey_bytes(const Survey *s) { return s ? s->bytes : 0; }

int survey_run(Survey *s, hipStream_t st, const float2 *in, long long n, int *launches, uint64_t *segments,
               uint64_t *groups) {
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
  uint64_t ng = 0;
  if (Hold *h = s->hold; h && nseg) {  // P stays as it is until the next run's segment kernel
    hipLaunchKernelGGL(survey_hold_kernel, dim3((unsigned)(N / FOLD_TILE)), dim3(FOLD_TILE), 0, st, h->gsum, h->peak, h->low,
                       h->busy, h->level, h->ring, s->P, (int)N, (int)nseg, h->fill, h->group,
                       h->rows ? (int)(h->gidx % (uint64_t)h->rows) : 0, h->rows);
    nl++;
    ng = (uint64_t)((h->fill + nseg) / h->group);
    h->fill = (int)((h->fill + nseg) % h->group);
    h->gidx += ng;
    h->in_hold += ng;
  }
  CHK(hipGetLastError());
  s->ncarry = ntail;
  s->in_acc += (uint64_t)nseg;
  if (launches) *launches = nl;
  if (segments) *segments = (uint64_t)nseg;
  if (groups) *groups = ng;
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

int survey_hold_start(Survey *s, int group, int rows, const double *level) {
  if (!s || s->hold || group < 1 || group > 65536 || rows < 0 || rows > 4096) return AERO_E_INVALID;
  const size_t N = (size_t)s->N;
  Hold *h = new Hold();
  h->group = group;
  h->rows = rows;
  h->state_bytes = N * (2 * sizeof(double) + sizeof(uint32_t));
  const size_t o_gsum = 0, o_state = align256(o_gsum + N * sizeof(double)), o_init = align256(o_state + h->state_bytes),
               o_level = align256(o_init + h->state_bytes), o_ring = align256(o_level + (level ? N * sizeof(double) : 0));
  h->bytes = o_ring + (size_t)rows * N * sizeof(double);
  if (hipMalloc(reinterpret_cast<void **>(&h->mem), h->bytes) != hipSuccess) {
    delete h;
    return AERO_E_NOMEM;
  }
  h->gsum = reinterpret_cast<double *>(h->mem + o_gsum);
  h->peak = reinterpret_cast<double *>(h->mem + o_state);
  h->low = h->peak + N;
  h->busy = reinterpret_cast<uint32_t *>(h->low + N);
  h->init = h->mem + o_init;
  h->level = level ? reinterpret_cast<double *>(h->mem + o_level) : nullptr;
  h->ring = rows ? reinterpret_cast<double *>(h->mem + o_ring) : nullptr;
  // a level that is NaN or infinite is never exceeded: +infinity on the device
  std::vector<double> inf(N, __builtin_inf()), lv;
  if (level) {
    lv.assign(level, level + N);
    for (double &v : lv)
      if (!(v >= -DBL_MAX && v <= DBL_MAX)) v = __builtin_inf();
  }
  hipError_t e = hipMemset(h->mem, 0, o_level);
  if (e == hipSuccess) e = hipMemcpy(h->init + N * sizeof(double), inf.data(), N * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(h->peak, h->init, h->state_bytes, hipMemcpyDeviceToDevice);
  if (e == hipSuccess && level) e = hipMemcpy(h->level, lv.data(), N * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    fprintf(stderr, "aero_chan: survey hold setup failed: %s\n", hipGetErrorString(e));
    (void)hipFree(h->mem);
    delete h;
    return AERO_E_HIP;
  }
  s->hold = h;
  return AERO_OK;
}

void survey_hold_stop(Survey *s) {
  if (!s || !s->hold) return;
  (void)hipDeviceSynchronize();
  (void)hipFree(s->hold->mem);
  delete s->hold;
  s->hold = nullptr;
}

bool survey_hold_on(const Survey *s) { return s && s->hold; }

size_t survey_hold_bytes(const Survey *s) { return s && s->hold ? s->hold->bytes : 0; }

int survey_hold_read(Survey *s, hipStream_t st, double *peak, double *low, uint32_t *busy, size_t cap, uint64_t *groups,
                     int reset) {
  if (!s || !s->hold || !peak || !low || !groups || cap < (size_t)s->N) return AERO_E_INVALID;
  Hold *h = s->hold;
  const size_t N = (size_t)s->N;
  CHK(hipMemcpyAsync(peak, h->peak, N * sizeof(double), hipMemcpyDeviceToHost, st));
  CHK(hipMemcpyAsync(low, h->low, N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (busy) CHK(hipMemcpyAsync(busy, h->busy, N * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (reset) CHK(hipMemcpyAsync(h->peak, h->init, h->state_bytes, hipMemcpyDeviceToDevice, st));
  CHK(hipStreamSynchronize(st));
  *groups = h->in_hold;
  if (reset) h->in_hold = 0;
  return AERO_OK;
}

int survey_hold_rows(Survey *s, hipStream_t st, double *dst, size_t cap_rows, uint64_t *first_group, size_t *n) {
  if (!s || !s->hold || !s->hold->rows || !first_group || !n || (cap_rows && !dst)) return AERO_E_INVALID;
  Hold *h = s->hold;
  const size_t N = (size_t)s->N, rows = (size_t)h->rows;
  const size_t have = (size_t)std::min<uint64_t>(h->gidx, rows), m = std::min(have, cap_rows);
  const uint64_t first = h->gidx - m;
  // rows first .. first + m - 1 lie at first % rows onwards, around the ring's end
  const size_t r0 = (size_t)(first % rows), m0 = std::min(m, rows - r0);
  if (m0) CHK(hipMemcpyAsync(dst, h->ring + r0 * N, m0 * N * sizeof(double), hipMemcpyDeviceToHost, st));
  if (m > m0) CHK(hipMemcpyAsync(dst + m0 * N, h->ring, (m - m0) * N * sizeof(double), hipMemcpyDeviceToHost, st));
  CHK(hipStreamSynchronize(st));
  *first_group = first;
  *n = m;
  return m < have ? AERO_E_FULL : AERO_OK;
}

}  // namespace aero
