/*
 * coarse.hip — CoarseFreqEstimate::ProcessBasebandData
 * (decode/coarsefreqestimate.cpp:89-150) plus the hop-time control path
 * OqpskDemodulator::FreqOffsetEstimateSlot (decode/oqpskdemodulator.cpp:562-620),
 * SignalHunter::updatedSignalStatus (decode/hunter.cpp:21-42) and
 * CenterFreqChangedSlot (decode/oqpskdemodulator.cpp:256-280), for every
 * channel whose 4096-sample hop is due.
 *
 * One workgroup works on one channel at a time.  The 16384-point kinds
 * (OQPSK, C channel) fill a CU with one 1024-thread workgroup, so their
 * launch is persistent: at most one workgroup per CU, each walking through
 * its share of the channels (coarse_sched.h) with the next channel's state
 * and this channel's hop-control state loaded under the tail's arithmetic,
 * the next due channel's head (ring image, table gathers) run under this
 * channel's tail ("the overlapped head" below; coarse_lds.h),
 * and the other waves starting the next channel while lane 0 finishes the
 * hop control.  The 8192-point MSK kinds run several workgroups per CU and
 * keep one workgroup per channel (the same code, a walk of one).
 *
 * The 16384-point FP64 FFTs keep 16
 * complex values per thread in registers and run JFFT's radix-2 DIT
 * butterflies (decode/jfft.cpp:114-212) chained through register stages, a
 * wave-local LDS transpose, lane permutes and one workgroup exchange per
 * transform (fft_chain.h); every butterfly uses the same operands and
 * twiddle as the reference, so the output is bit-identical regardless of how
 * butterflies are scheduled.
 */
#include <hip/hip_runtime.h>

#include <type_traits>

#include "aero_math.h"
#include "coarse_lds.h"
#include "coarse_sched.h"
#include "engine_common.h"
#include "fft_chain.h"

namespace aero {

#ifdef AERO_X_OCML  // timing experiment only (see demod_oqpsk.hip)
#define CO_HYPOT ::hypot
#define CO_HYPOT_NR ::hypot
#define CO_LOG10_GE1(x) ::log10(x)
#define CO_LOG10_GE1_TAB(x, tab) ::log10(x)
#else
#define CO_HYPOT aero_hypot
#define CO_HYPOT_NR aero_hypot_nr
// log10 of max(|X|, 1): the argument is at least 1, and finite for any finite
// spectrum (one wave-uniform test; aero_math.h)
#define CO_LOG10_GE1(x) aero_log10_ge1_w(x, &aero_g_log_tab[0][0])
#define CO_LOG10_GE1_TAB(x, tab) aero_log10_ge1_w(x, tab)
#endif

// Geometry of one channel's coarse estimate (decode/coarsefreqestimate.cpp:39-76
// with the settings each demodulator applies).  OQPSK: setSettings(14, 10500,
// 10500, 48000); MSK: setSettings(13, 900, 600, Fs).
template <int M>
struct CoarseK;
template <>
struct CoarseK<MODE_OQPSK> {
  static constexpr int LOG2N = 14, HOPN = 4096, START = 3584, STOP = 12800, ILO = 4608, IHI = 11776, EPB = 1792;
  static constexpr int YLO = clds::YLO14, YHI = clds::YHI14;
  static constexpr double FS = 48000.0;
};
// the C channel: setSettings(14, 10500, 8400, 48000): the OQPSK bins, the
// expected peak at round(8400 / (2 hzperbin)) = 1434; the raised-cosine window
// in place of the boxcar (coarsefreqestimate.cpp:97-104)
template <>
struct CoarseK<MODE_C8400> {
  static constexpr int LOG2N = 14, HOPN = 4096, START = 3584, STOP = 12800, ILO = 4608, IHI = 11776, EPB = 1434;
  static constexpr int YLO = clds::YLO14, YHI = clds::YHI14;
  static constexpr double FS = 48000.0;
};
// MSK at Fs (setSettings(13, 900, 600, Fs)): hzperbin = Fs / 8192; startbin
// round(900 / hzperbin), stopbin nfft - startbin, the fold search over
// [round(-900 / hzperbin + 4096), round(900 / hzperbin + 4096)) with
// expectedpeakbin round(600 / (2 hzperbin)); y kept over MSK_YLO..MSK_YHI
template <int FS>
struct MskCoarseBins;
template <>
struct MskCoarseBins<12000> {
  static constexpr int START = 614, STOP = 7578, ILO = 3482, IHI = 4710, EPB = 205;
};
template <>
struct MskCoarseBins<24000> {
  static constexpr int START = 307, STOP = 7885, ILO = 3789, IHI = 4403, EPB = 102;
};
template <>
struct MskCoarseBins<48000> {
  static constexpr int START = 154, STOP = 8038, ILO = 3942, IHI = 4250, EPB = 51;
};
template <int M>
struct CoarseK {
  using B = MskCoarseBins<msk_fs(M)>;
  static constexpr int LOG2N = 13, HOPN = 2048, START = B::START, STOP = B::STOP, ILO = B::ILO, IHI = B::IHI,
                       EPB = B::EPB;
  static constexpr int YLO = MSK_YLO, YHI = MSK_YHI;
  static_assert(ILO - EPB - 1 >= YLO && IHI - 1 + EPB + 1 <= YHI, "fold search inside the kept y bins");
  static constexpr double FS = (double)msk_fs(M);
};

// the bins and rate one launch works with: compile-time for the fixed-rate
// groups, the group's MskGen for a generic-rate one
struct CoarseBins {
  int start, stop, ilo, ihi, epb;
  double fs;
};
template <int M>
__device__ __forceinline__ CoarseBins coarse_bins(const DevState &S) {
  using K = CoarseK<M>;
  if constexpr (msk_generic(M))
    return {S.mg.start, S.mg.stop, S.mg.ilo, S.mg.ihi, S.mg.epb, S.mg.fs};
  else
    return {K::START, K::STOP, K::ILO, K::IHI, K::EPB, K::FS};
}

__device__ __forceinline__ void set_freq1(double &freq, double &step, double f, double fs) {  // SetFreq (DSP.cpp:163-168)
  freq = f;
  if (freq < 0) freq = 0;
  step = (freq) * ((double)WTSIZE) / fs;
}

struct HopCtl {
  double m2f, m2s, mcf, mcs;
  int countdown2, countdown, ecd, yres_next;
  long long zb;
  bool stepped;  // SignalHunter emitted newFreqCenter(step_fc) this hop
  double step_fc;
};

// OqpskDemodulator::FreqOffsetEstimateSlot (decode/oqpskdemodulator.cpp:562-620),
// SignalHunter (decode/hunter.cpp:21-42; maxTries 15, params 0/25000/10500,
// decode/decode.cpp:161,169) and CenterFreqChangedSlot (:256-280).  dcd is
// never set (DCDstatSlot unconnected, decode/decode.cpp:168-241).
__device__ __forceinline__ bool hop_control_oqpsk(HopCtl &h, bool c8400, double est, double mse, unsigned &iter,
                                                  int &scans, long long nk) {
  const double thr = 0.65, lockingbw = 10500.0, Fs = 48000.0;
  if (mse < thr) {
    if (h.countdown2 > 0)
      h.countdown2--;
    else
      set_freq1(h.m2f, h.m2s, h.mcf + est, Fs);
  } else
    h.countdown2 = 5;
  if ((mse > thr) && (fabs(h.m2f - (h.mcf + est)) > 3.0)) set_freq1(h.m2f, h.m2s, h.mcf + est, Fs);
  if ((mse < thr) && (fabs(h.m2f - h.mcf) > 3.0)) {
    if (h.countdown > 0)
      h.countdown--;
    else {
      set_freq1(h.mcf, h.mcs, h.m2f, Fs);
      if (h.mcf < lockingbw / 2.0) set_freq1(h.mcf, h.mcs, lockingbw / 2.0, Fs);
      if (h.mcf > (Fs / 2.0 - lockingbw / 2.0)) set_freq1(h.mcf, h.mcs, Fs / 2.0 - lockingbw / 2.0, Fs);
      h.ecd = 4;  // bigchange (coarsefreqestimate.cpp:128-132)
      h.yres_next = 1;
      h.zb = nk + 1;  // bbcycbuff zeroed
    }
  } else
    h.countdown = 4;
  const bool gotasignal = !(mse > thr);
  if (gotasignal) {
    iter = 0;
  } else {
    iter++;
    if (iter > 0 && iter % 15u == 0) {
      double fc = 0u + (10500u >> 1) * (int)(iter / 15u);
      if (fc > 25000u - (10500u >> 1)) {
        fc = 0.0;
        iter = 0;
        scans++;
      }
      h.stepped = true;
      h.step_fc = fc;
      // CenterFreqChangedSlot, afc on; fb != 8400 clamps the centre
      // (oqpskdemodulator.cpp:256-265); fb is 10500 as aero-decode's Decoder
      // leaves it (decode/decode.cpp:152-159, oqpskdemodulator.h:24-32)
      if (!c8400) {
        if (fc < (0.5 * 10500.0)) fc = 0.5 * 10500.0;
        if (fc > (Fs / 2.0 - 0.5 * 10500.0)) fc = Fs / 2.0 - 0.5 * 10500.0;
      }
      set_freq1(h.mcf, h.mcs, fc, Fs);
      set_freq1(h.m2f, h.m2s, h.mcf, Fs);
      if ((h.m2f - h.mcf) > (lockingbw / 2.0)) set_freq1(h.m2f, h.m2s, h.mcf + (lockingbw / 2.0), Fs);
      if ((h.m2f - h.mcf) < (-lockingbw / 2.0)) set_freq1(h.m2f, h.m2s, h.mcf - (lockingbw / 2.0), Fs);
      h.zb = nk + 1;
    }
  }
  return gotasignal;
}

__device__ __forceinline__ bool hop_control(HopCtl &h, std::integral_constant<int, MODE_OQPSK>, double, double est,
                                            double mse, unsigned &iter, int &scans, long long nk) {
  return hop_control_oqpsk(h, false, est, mse, iter, scans, nk);
}
// the C channel: the same slot (its prefilter mixer's retune there is
// overridden by the message-end retune before any prefilter runs, :555-569)
__device__ __forceinline__ bool hop_control(HopCtl &h, std::integral_constant<int, MODE_C8400>, double, double est,
                                            double mse, unsigned &iter, int &scans, long long nk) {
  return hop_control_oqpsk(h, true, est, mse, iter, scans, nk);
}

// MskDemodulator::FreqOffsetEstimateSlot (decode/mskdemodulator.cpp:430-469;
// its AFC branch needs dcd, never set), SignalHunter with params 0/6000/900
// (decode/decode.cpp:193) and MskDemodulator::CenterFreqChangedSlot (:220-240).
template <int M>
__device__ __forceinline__ bool hop_control(HopCtl &h, std::integral_constant<int, M>, double Fs, double est,
                                            double mse, unsigned &iter, int &scans, long long nk) {
  const double thr = 0.5, lockingbw = 900.0, fb = 600.0;
  if ((mse > thr) && (fabs(h.m2f - (h.mcf + est)) > 0.0)) set_freq1(h.m2f, h.m2s, h.mcf + est, Fs);
  h.countdown = 4;
  const bool gotasignal = !(mse > thr);
  if (gotasignal) {
    iter = 0;
  } else {
    iter++;
    if (iter > 0 && iter % 15u == 0) {
      double fc = 0u + (900u >> 1) * (int)(iter / 15u);
      if (fc > 6000u - (900u >> 1)) {
        fc = 0.0;
        iter = 0;
        scans++;
      }
      h.stepped = true;
      h.step_fc = fc;
      if (fc < (0.75 * fb)) fc = 0.75 * fb;
      if (fc > (Fs / 2.0 - 0.75 * fb)) fc = Fs / 2.0 - 0.75 * fb;
      set_freq1(h.mcf, h.mcs, fc, Fs);
      set_freq1(h.m2f, h.m2s, h.mcf, Fs);
      if ((h.m2f - h.mcf) > (lockingbw / 2.0)) set_freq1(h.m2f, h.m2s, h.mcf + (lockingbw / 2.0), Fs);
      if ((h.m2f - h.mcf) < (-lockingbw / 2.0)) set_freq1(h.m2f, h.m2s, h.mcf - (lockingbw / 2.0), Fs);
      h.zb = nk + 1;
    }
  }
  return gotasignal;
}

// AERO_X_STAMPS (diagnostic build only): s_memtime cycle totals per section
// of wave 0 of every workgroup (batch scan + channel state, ring to LDS,
// table gathers + mix, FFT 1, boxcar+iFFT+square, FFT 3, |X|, log10
// smoothing, fold search, lane 0's hop control; slots 0-9), wave 0's whole
// time in the kernel over the workgroups that ran a hop (slot 10: less the
// sections, the turnover between channels and the launch) and the number of
// hops (slot 11).  With the overlapped head slots 0 and 1 count the plain
// heads only and slot 2 the successor's mix; its image loads, the barrier
// inside |X| and the issue of its table gathers run inside slot 6, the
// twiddle write at the head of slot 7, under which the gathers land
// (scripts/coarse_stamps.py)
constexpr int CSTAMP_N = 12;
#ifdef AERO_X_STAMPS
__device__ unsigned long long g_cstamps[CSTAMP_N];
#define CSTAMP(k)                                                  \
  do {                                                             \
    __builtin_amdgcn_sched_barrier(0);                             \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();    \
    cst_[k] += t_ - ctime_;                                        \
    ctime_ = t_;                                                   \
    __builtin_amdgcn_sched_barrier(0);                             \
  } while (0)
#else
#define CSTAMP(k) \
  do {            \
  } while (0)
#endif

// a wave-uniform value, in scalar registers from here on
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long long uni(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

// the lane's number, by an instruction the compiler does not move out of a loop
__device__ __forceinline__ int lane_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=&v"(l));
  return l;
}

// what a hop needs of its channel's state before its first barrier
struct HopPro {
  long long filled, zero_before;
  int hops_done, yreset;
};
__device__ __forceinline__ HopPro load_pro(const DevState &S, int C, int c) {
  HopPro p;
  p.filled = S.ls[LS_FILLED * C + c];
  p.zero_before = S.ls[LS_ZERO_BEFORE * C + c];
  p.hops_done = S.is[IS_HOPS_DONE * C + c];
  p.yreset = S.is[IS_YRESET * C + c];
  return p;
}
__device__ __forceinline__ HopPro uni(const HopPro &p) {
  return {uni(p.filled), uni(p.zero_before), uni(p.hops_done), uni(p.yreset)};
}

// what lane 0's hop control reads of it (nothing else writes these during a
// launch, so they are loaded while the tail's arithmetic runs)
struct HopEpi {
  double mse, m2f, m2s, mcf, mcs;
  int ecd, countdown2, countdown, iter, scans, steps, hop_n;
};
__device__ __forceinline__ HopEpi load_epi(const DevState &S, int C, int c) {
  HopEpi e;
  e.mse = S.ds[DS_MSE * C + c];
  e.m2f = S.ds[DS_M2_FREQ * C + c];
  e.m2s = S.ds[DS_M2_STEP * C + c];
  e.mcf = S.ds[DS_MC_FREQ * C + c];
  e.mcs = S.ds[DS_MC_STEP * C + c];
  e.ecd = S.is[IS_EMPTYCD * C + c];
  e.countdown2 = S.is[IS_COUNTDOWN2 * C + c];
  e.countdown = S.is[IS_COUNTDOWN * C + c];
  e.iter = S.is[IS_HUNT_ITER * C + c];
  e.scans = S.is[IS_HUNT_SCANS * C + c];
  e.steps = S.is[IS_HUNT_STEPS * C + c];
  e.hop_n = S.hop_n[c];
  return e;
}

// The workgroup's LDS (coarse_lds.h).  Without the overlapped head: the four
// arrays as they always were.  With it: one raw buffer carved at the map's
// offsets, because the next channel's ring image lies across the end of lds
// and s_tw.
template <int L, int YLEN, bool OVL>
struct CoarseLds {
  double *lds;
  double2 *s_tw;
  double *red_v;
  int *red_i;
  uint32_t *img;   // the overlapped head's ring image (OVL only)
  double *logtab;  // its copy of aero_g_log_tab (OVL only)
};
template <int L, int YLEN, bool OVL>
__device__ __forceinline__ CoarseLds<L, YLEN, OVL> coarse_lds() {
  using LM = clds::Map<L, YLEN, OVL>;
  static_assert(LM::TWLEN == TwLds<L>::LEN && clds::ypad(12345) == fftl::ypadn<6>(12345), "coarse_lds.h restates these");
  if constexpr (OVL) {
    __shared__ __attribute__((aligned(16))) unsigned char raw[LM::TOTAL];
    return {reinterpret_cast<double *>(raw + LM::LDS_OFF), reinterpret_cast<double2 *>(raw + LM::TW_OFF),
            reinterpret_cast<double *>(raw + LM::REDV_OFF), reinterpret_cast<int *>(raw + LM::REDI_OFF),
            reinterpret_cast<uint32_t *>(raw + LM::IMG_OFF), reinterpret_cast<double *>(raw + LM::LOGTAB_OFF)};
  } else {
    __shared__ double lds[LM::PADDED];
    __shared__ double2 s_tw[LM::TWLEN];
    __shared__ double red_v[LM::FT / 64];
    __shared__ int red_i[LM::FT / 64];
    static_assert(sizeof lds + sizeof s_tw + sizeof red_v + sizeof red_i == LM::TOTAL, "coarse_lds.h describes this");
    return {lds, s_tw, red_v, red_i, nullptr, nullptr};
  }
}

// OVL (persistent kinds only): a due channel that follows another in its
// batch has its head (ring image, table gathers) run under that channel's
// tail; see "the overlapped head" below
template <int M, bool OVL = false>
__global__ __launch_bounds__(1 << (CoarseK<M>::LOG2N - 4), CoarseK<M>::LOG2N == 13 ? 4 : 1) void coarse_kernel(DevState S, DevTables T, int nch) {
  using K = CoarseK<M>;
  const CoarseBins KB = coarse_bins<M>(S);
  constexpr int L = K::LOG2N, N = 1 << L, FT = N / 16;
  constexpr int YLEN = K::YHI - K::YLO + 1;
  constexpr bool PERSIST = L == 14;  // launch_coarse
  static_assert(PERSIST || !OVL, "the overlapped head belongs to the persistent walk");
  const auto sm = coarse_lds<L, YLEN, OVL>();
  double *const lds = sm.lds;
  double2 *const s_tw = sm.s_tw;
  double *const red_v = sm.red_v;
  int *const red_i = sm.red_i;
  // the wave's number is kept in a scalar register and the lane's is read
  // anew per channel (lane_now): no vector register holds the thread index
  // across the walk
  const int wave = uni((int)threadIdx.x >> 6);
  const int C = S.C;
  // this workgroup's channels (coarse_sched.h)
  const int wgs = (int)gridDim.x, wg = (int)blockIdx.x;
  const int iters = csched::iters(nch, wgs, wg);
#ifdef AERO_X_STAMPS
  unsigned long long cst_[CSTAMP_N] = {}, ctime_ = __builtin_amdgcn_s_memtime();
  const unsigned long long cstart_ = ctime_;
#endif
  bool have_tw = false;
#pragma unroll 1
  for (int k0 = 0; k0 < iters; k0 += csched::BATCH) {
    // hop due? sample n_k = HOP k - 1, demod stopped there and the ring holds
    // it.  One lane per channel of the batch, every wave for itself (the
    // waves are not in step between channels, and nothing of a channel that
    // is still to come changes during the launch)
    bool due = false;
    if (csched::lane_has(iters, k0, lane_now())) {
      const int cc = csched::channel(wgs, wg, k0 + lane_now());
      const long long nsamp = S.ls[LS_NSAMP * C + cc];
      const long long avail = S.ls[LS_AVAIL * C + cc];
      const long long nkk = (long long)K::HOPN * (S.is[IS_HOPS_DONE * C + cc] + 1) - 1;
      due = nsamp == nkk && avail > nkk;
    }
    unsigned long long mask = __ballot(due);
    // the state of the channel about to start: loaded under the previous
    // channel's tail (pn, made scalar after its fold), by itself for a
    // batch's first
    HopPro pro{};
    bool have_pro = false;
    // The overlapped head (OVL).  While the workgroup is in channel c's tail
    // and a due successor c' is left in the batch, it already runs c''s head:
    //   before the third transform   c''s HopPro
    //   under the first half of |X|  c''s ring words -> the image behind ylds,
    //                                by loads that write the LDS directly
    //   a barrier inside |X|         the image is whole
    //   under the second half        the image's words, bit-reversed, and the
    //                                table gathers into x[] as its registers
    //                                die
    //   after the barrier of |X|     s_tw, which the image lay over, again
    //   under the log10 loop         nothing of c' is issued; the gathers land
    //   after the fold's barrier     the mix, and c''s forward transform
    // pre says that x[] holds c''s snapshot already.  It follows from mask alone,
    // which every wave derives for itself from state that does not change
    // under it, so all 16 waves take the same head and execute the same
    // barriers in the same order.  The batch's first due channel, and so any
    // channel after a gap between batches, takes the plain head.
    bool pre = false;
    double2 x[16];
#pragma unroll 1
    while (mask) {
      // a thread index of this channel's own: whatever is computed from it is
      // computed again per channel, not held in registers across the walk
      // (that spilled).  It is read again where a section starts, so that no
      // register holds it through the transforms either
      auto tnow = [&]() { return wave * 64 + lane_now(); };
      int t = PERSIST ? tnow() : (int)threadIdx.x;
      const int c = csched::channel(wgs, wg, k0 + csched::first(mask));
      mask = csched::rest(mask);
      if (!have_pro) pro = uni(load_pro(S, C, c));
      const long long filled = pro.filled, zero_before = pro.zero_before;
      const int hops_done = pro.hops_done, yreset = pro.yreset;
      const long long nk = (long long)K::HOPN * (hops_done + 1) - 1;
      // ring entry of the hop sample not written yet (the demod segment ended
      // before the sample was pushed): mixer_center has not moved since.  The
      // word goes to the ring and into the LDS image (not read back from
      // memory): by the thread that copies its place in the plain head, by
      // one thread of the wave that loaded its place in the overlapped one.
      // For a successor cc (overlapped head) this runs under its predecessor's
      // tail, before that channel's hop control: everything read here
      // (DS_MC_PTR, the PCM word, LS_FILLED through HopPro) is cc's own, which
      // no other channel's hop control writes; and LS_FILLED, written early,
      // is not among what a later batch's due test reads (NSAMP, AVAIL,
      // HOPS_DONE)
      auto ring_fixup = [&](int cc, long long fil, long long nkk, int tt, int &fj, uint32_t &fw) {
        fj = -1;
        fw = 0;
        if (fil <= nkk) {
          const double mc_ptr = S.ds[DS_MC_PTR * C + cc];
          int tint = (int)mc_ptr;
          if (tint >= WTSIZE) tint = 0;
          if (tint < 0) tint = WTSIZE - 1;
          const int16_t xs = S.pcm[(nkk & (S.pcm_cap - 1)) * C + cc];
          fw = (uint32_t)tint | ((uint32_t)(uint16_t)xs << 16);
          fj = (int)(nkk & (N - 1));
          if (tt == 0) {
            S.cring[(size_t)cc * N + fj] = fw;
            S.ls[LS_FILLED * C + cc] = nkk + 1;
          }
        }
      };
      const long long s0 = nk - (N - 1);  // sample of snapshot element 0 (oqpskdemodulator.cpp:359-365)
      if (!(OVL && pre)) {
        int fixj;
        uint32_t fixw;
        ring_fixup(c, filled, nk, t, fixj, fixw);
        CSTAMP(0);

        if (!have_tw) {  // once per workgroup
          load_tw_lds<L>(s_tw, T.tw, t, FT);
          // (read in the log10 loop, many barriers on)
          if constexpr (OVL)
            if (t < 256) sm.logtab[t] = (&aero_g_log_tab[0][0])[t];
          have_tw = true;
        }
        // ring words -> LDS (uint32, one pad word per 16: the bit-reversed gather
        // below reads 16-word strides, which would hit 4 of the 64 banks unpadded).
        // Every wave is past the previous channel's fold here (its last barrier),
        // so nobody reads the LDS any more; lane 0's hop control only reads red_*
        uint32_t *ring_lds = reinterpret_cast<uint32_t *>(lds);
        const uint32_t *ring = S.cring + (size_t)c * N;
        if constexpr (PERSIST) {
          // counted: of a thread index read per channel the compiler does not
          // know that j = t, t + FT, ... makes 16 trips, and a rolled loop
          // waits for each load before the next
#pragma unroll
          for (int i = 0; i < N / FT; ++i) {
            const int j = t + i * FT;
            const uint32_t w = ring[j];
            ring_lds[j + (j >> 4)] = j == fixj ? fixw : w;
          }
        } else {
          for (int j = t; j < N; j += FT) {
            const uint32_t w = ring[j];
            ring_lds[j + (j >> 4)] = j == fixj ? fixw : w;
          }
        }
        __syncthreads();
        CSTAMP(1);
        // every element's table entry is gathered before any is waited for (the
        // compiler would otherwise sink each gather into its element's branch
        // and wait for it there: 16 round trips one after another)
        double2 cs[16];
        double dval[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int q = (int)((s0 + bitrev<L>(epos<L, 0>(t, i))) & (N - 1));
          const uint32_t w = ring_lds[q + (q >> 4)];
          dval[i] = ((double)(int16_t)(w >> 16)) / 32768.0;
#ifdef AERO_X_CISLINE
          cs[i] = T.cis[w & 0x7];  // timing build: every gather on one line
#else
          cs[i] = T.cis[w & 0xFFFF];
#endif
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(cs[i].x), "+v"(cs[i].y));
        // entries below zero_before were cleared (AFC, CenterFreqChangedSlot);
        // entries of samples before the channel's first are the ring's own
        // contents (zero for a new channel: CIS[0] x 0; a channel that changed
        // rate keeps the ring it had, mskdemodulator.cpp:94-218).  zero_before
        // lies inside the snapshot only for the four hops after a reset or a
        // centre-frequency step: on every other hop (one wave-uniform test,
        // the same in all waves: HopPro) no element's sample number is looked at
#pragma unroll
        for (int i = 0; i < 16; ++i) x[i] = make_double2(cs[i].x * dval[i], cs[i].y * dval[i]);
        if (s0 < zero_before) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const long long s = s0 + bitrev<L>(epos<L, 0>(t, i));
            if (s < zero_before) x[i] = make_double2(0.0, 0.0);
          }
        }
        __syncthreads();  // the ring image is read: the LDS is the transforms' from here on
        CSTAMP(2);
      }
      // the due successor of this batch, if any: its head runs under this
      // channel's tail (OVL)
      const bool nxt = mask != 0;
      const int cn = nxt ? csched::channel(wgs, wg, k0 + csched::first(mask)) : c;
      if constexpr (PERSIST) t = tnow();
      // forward FFT
      chain::fft<L, true, false>(x, t, lds, T.tw, s_tw, T.twg);
      CSTAMP(3);
      if constexpr (PERSIST) t = tnow();
      // boxcar: zero bins startbin..stopbin (coarsefreqestimate.cpp:97-100);
      // the C channel multiplies by the raised-cosine window instead (:101-104)
      const int bin_t = chain::out_bin_thread<L>(t);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int p = bin_t | chain::out_bin_reg<L>(i);
        if constexpr (M == MODE_C8400) {
          const double w = T.cwin[i * FT + t];  // = window[p], stored in this layout's order (engine.hip)
          x[i] = make_double2(x[i].x * w, x[i].y * w);
        } else {
          if (p >= KB.start && p <= KB.stop) x[i] = make_double2(0.0, 0.0);
        }
      }
      // inverse FFT.  JFFT scales by 1/N and FFTWrapper multiplies by N
      // (jfft.cpp:206-212, fftwrapper.cpp:22-29): x * 2^-L * 2^L == x exactly for every
      // x with |x| >= 2^-1008, and a nonzero value of this path is far above that
      // (magnitudes >= ~2^-200: sums and products of pcm/32768, CIS and twiddle
      // values), so both multiplies are the identity here and are skipped.
      if constexpr (PERSIST) t = tnow();
      chain::fft<L, false, true>(x, t, lds, T.twi, s_tw, T.twgi);
      // OVL: the successor's state, needed when its ring image is written
      // under |X|; loaded here so that the squares cover the round trip, and
      // scalar from the third transform on
      // (unconditionally, of this channel again if there is no successor: a
      // conditional load comes back out of the scalar registers as a phi)
      HopPro pn{};
      if constexpr (OVL) pn = load_pro(S, C, cn);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        // square
        // (x*y + y*x: the two products are the same IEEE product, so the sum is
        // exactly 2 (x*y))
        const double r = x[i].x * x[i].x - x[i].y * x[i].y;
        const double im = 2.0 * (x[i].x * x[i].y);
        x[i] = make_double2(r, im);
      }
      if constexpr (OVL) pn = uni(pn);
      CSTAMP(4);
      if constexpr (PERSIST) t = tnow();
      chain::fft<L, false, false>(x, t, lds, T.tw, s_tw, T.twg);
      CSTAMP(5);
      if constexpr (PERSIST) t = tnow();
      uint32_t pcmw[8];  // the 16 PCM halves of the successor's ring words, two per register
      int fixjn = -1;
      uint32_t fixwn = 0;
      const long long nkn = (long long)K::HOPN * (pn.hops_done + 1) - 1;
      if (OVL && nxt) ring_fixup(cn, pn.filled, nkn, t, fixjn, fixwn);
      if constexpr (OVL) {
        // no store in flight from here to the end of |X| (lane 0's of the
        // previous channel's hop control are long done, the fix-up's are
        // rare): with a store possibly in flight the compiler takes the
        // counter to be out of order and turns every wait below into a wait
        // for everything, the gathers included
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
      }
      // OVL: the successor's ring words go into the image (coarse_lds.h) by
      // loads that write the LDS directly, no register between: wave w's
      // i-th load brings words 64 w + lane + 1024 i to a wave-uniform place
      // plus lane x 4.  The image lies behind ylds[0 .. ypad(YLEN - 1)],
      // which the waves write during |X|, across the rest of lds and s_tw,
      // short of red_* (the map's static_asserts).  This thread has passed
      // the barrier that ends the third transform's exchange (chain::gx): by
      // then every wave has finished its reads of the exchange and made the
      // transform's last read of s_tw (stages <= 9, before the exchange).
      // Called where no ordinary load's result is used before the wait in the
      // middle of |X|: with such a load in flight the compiler makes the next
      // use of any load's result a wait for everything
      auto image_issue = [&]() {
        if constexpr (OVL) {
          using LM = clds::Map<L, YLEN, OVL>;
          if (nxt) {
            const uint32_t *ringn = S.cring + (size_t)cn * N + fresh(t);
            uint32_t *dst = sm.img + LM::img(wave * 64);
#pragma unroll
            for (int i = 0; i < N / FT; ++i) {
              static_assert(LM::img(64 + 1024) == LM::img(64) + LM::img(1024), "the map adds over wave and load");
              __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(ringn + i * FT),
                                               (__attribute__((address_space(3))) void *)(dst + LM::img(i * FT)), 4, 0,
                                               0);
            }
          }
        }
      };
      // fftshift + smoothing y = 0.9 y + 10 log10(max(|X|,1)) over the bins the
      // fold reads: |X| per bin to LDS first (keeps the log10 out of the
      // register-heavy FFT scope), then a dense log10 loop; the y history (HBM)
      // is read three iterations ahead of its update, the first loads
      // overlapping the |X| work.  (Round 5 measured the alternatives on one box:
      // the whole history brought into LDS by direct-to-LDS loads as the third
      // transform ends, |X| and log10 in registers meanwhile, 21.49 ms; plain
      // register loads of the whole history, 21.58 ms; this, 20.97 ms.  The
      // history's 86 KB take ~46k cycles from issue to arrival whichever way,
      // more than the |X| and log10 work that can overlap them.)
      double *yg = S.y + (size_t)c * YLEN;
#ifdef AERO_X_NOYREAD
      auto yload = [&](int k) { return 20.0 + 0.0 * k; };  // timing build: no y history reads
#else
      auto yload = [&](int k) { return (k < YLEN && !yreset) ? yg[k] : 20.0; };
#endif
      double yp0 = yload(t), yp1 = yload(t + FT);
      // OVL: everything the tail loads before the gathers goes out ahead of
      // the image loads and is back at the wait in the middle of |X|: the
      // third look-ahead y value, and s_tw's entry for when the image is read
      double yp2 = 0.0;
      double2 twv = make_double2(0.0, 0.0);
      if constexpr (OVL) {
        yp2 = yload(t + 2 * FT);
        twv = T.tw[min(t, TwLds<L>::LEN - 1)];
        image_issue();
      }
      // no barrier here: the third transform's workgroup exchange ended with
      // one (chain::gx), after which every wave only works in registers, so the
      // LDS is free for |X| as soon as this wave gets here
      double *ylds = lds;  // bin k - YLO at ypad(k - YLO)
      auto ypad = [](int q) { return fftl::ypadn<6>(q); };
      // |X| by aero_hypot_nr when every value of the wave is in its range (the
      // usual case: |X| of a live channel is ~1e9), else by aero_hypot
      // (of the 16384-point kinds only the registers some lane stores are
      // looked at: a register holds the FT bins from out_bin_reg(i) on, the
      // lanes their low bits.  The 8192-point kinds spilled with that)
      static_assert(fftl::thread_mask(fftl::lay_g<L>(), L) == FT - 1, "a register's bins are one run of FT");
      auto stored = [](int i) {
        const int y0 = chain::out_bin_reg<L>(i) ^ (N / 2);
        return y0 + FT - 1 >= K::YLO && y0 <= K::YHI;
      };
      bool nr = true;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (PERSIST && !stored(i)) continue;
        const double a = fabs(x[i].x), b = fabs(x[i].y);
        nr = nr && a <= 0x1p200 && b <= 0x1p200 && (a >= 0x1p-200 || b >= 0x1p-200);
      }
      // OVL: element i of the successor's snapshot: its word from the image,
      // bit-reversed as the plain head reads it, the PCM half packed and the
      // table gather issued into x[i] (dead once its |X| is stored)
      const long long s0n = nkn - (N - 1);
      auto gather_word = [&](int i) {
        using LM = clds::Map<L, YLEN, OVL>;
        const int q = (int)((s0n + bitrev<L>(epos<L, 0>(t, i))) & (N - 1));
        const uint32_t w = sm.img[LM::img(q)];
        pcmw[i >> 1] |= (i & 1) ? (w & 0xFFFF0000u) : (w >> 16);
#ifdef AERO_X_CISLINE
        x[i] = T.cis[w & 0x7];  // timing build: every gather on one line
#else
        x[i] = T.cis[w & 0xFFFF];
#endif
      };
      auto gather1 = [&](int i) {
        if constexpr (OVL) {
          if (nxt) {
            gather_word(i);
          } else {
            // No successor: the same number of loads, of the table's entry 0,
            // of which nothing comes.  x[] has to be defined on this path too
            // (otherwise the previous values stay live around the whole
            // walk), and with loads here as there the two paths join with the
            // same loads in flight: joined with none in flight on this one,
            // the compiler counts its waits for this path, and on the other
            // they then wait for gathers just issued.  (One set of
            // unconditional gathers with the index forced to 0 tipped the
            // register allocation into spilling.)
            x[i] = T.cis[0];
          }
        }
      };
      if constexpr (!OVL) {
        if (__all(nr)) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int yi = (bin_t | chain::out_bin_reg<L>(i)) ^ (N / 2);
            if (yi >= K::YLO && yi <= K::YHI) ylds[ypad(yi - K::YLO)] = CO_HYPOT_NR(x[i].x, x[i].y);
          }
        } else {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int yi = (bin_t | chain::out_bin_reg<L>(i)) ^ (N / 2);
            if (yi >= K::YLO && yi <= K::YHI) ylds[ypad(yi - K::YLO)] = CO_HYPOT(x[i].x, x[i].y);
          }
        }
        yp2 = yload(t + 2 * FT);
      } else {
        // |X| in two halves with one barrier between them, outside the
        // branch on the hypot path, so that every wave passes the same
        // barriers whichever path it takes.
        //   first half    registers 0 .. XH - 1, the image loads in flight
        //   the barrier   every wave has waited for its own image loads
        //                 (which orders them for its own LDS accesses) and,
        //                 past the barrier, everybody's: the image is whole
        //   second half   the successor's elements are gathered into x[] as
        //                 the registers die: at once those of the first half
        //                 and those no lane stores, then one after each |X|
        // All image reads come before the barrier that closes |X|: past it
        // s_tw, under the image, is written again.
        constexpr int XH = 8;
        using LM = clds::Map<L, YLEN, OVL>;
        if (__all(nr)) {
#pragma unroll
          for (int i = 0; i < XH; ++i) {
            if (!stored(i)) continue;
            const int yi = (bin_t | chain::out_bin_reg<L>(i)) ^ (N / 2);
            if (yi >= K::YLO && yi <= K::YHI) ylds[ypad(yi - K::YLO)] = CO_HYPOT_NR(x[i].x, x[i].y);
          }
        } else {
#pragma unroll
          for (int i = 0; i < XH; ++i) {
            if (!stored(i)) continue;
            const int yi = (bin_t | chain::out_bin_reg<L>(i)) ^ (N / 2);
            if (yi >= K::YLO && yi <= K::YHI) ylds[ypad(yi - K::YLO)] = CO_HYPOT(x[i].x, x[i].y);
          }
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's image loads have landed
        // the fix-up's word is not in memory yet when the image loads read its
        // place (or may not be): the thread whose wave loaded the place
        // patches the image, after that wave's loads
        if (nxt && fixjn >= 0 && (fixjn & (FT - 1)) == t) sm.img[LM::img(fixjn)] = fixwn;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) pcmw[k] = 0;
        // (one branch around the whole group: its words are read together)
        if (nxt) {
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (i < XH || !stored(i)) gather_word(i);
        } else {
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (i < XH || !stored(i)) gather1(i);
        }
        // (the hypot path is chosen per register here, the gathers outside
        // the choice: around one branch over the whole half the compiler
        // waited in the branch-free path's first hypot for every gather of
        // the group above)
        const bool allnr = __all(nr);
#pragma unroll
        for (int i = XH; i < 16; ++i) {
          if (!stored(i)) continue;
          const int yi = (bin_t | chain::out_bin_reg<L>(i)) ^ (N / 2);
          if (allnr) {
            if (yi >= K::YLO && yi <= K::YHI) ylds[ypad(yi - K::YLO)] = CO_HYPOT_NR(x[i].x, x[i].y);
          } else {
            if (yi >= K::YLO && yi <= K::YHI) ylds[ypad(yi - K::YLO)] = CO_HYPOT(x[i].x, x[i].y);
          }
          gather1(i);
        }
      }
      __syncthreads();
      CSTAMP(6);
      // the loads that would otherwise sit between two channels, issued here
      // where the log10 loop and the fold hide them: the next due channel's
      // state (same batch; the first of a batch loads its own; the overlapped
      // head has it already) and, on wave 0, what lane 0's hop control reads
      have_pro = nxt;
      if constexpr (!OVL)
        if (have_pro) pn = load_pro(S, C, cn);
      // (OVL: after the log10 loop, under the fold; its 17 registers and the
      // gathered table entries do not fit beside the loop together)
      HopEpi ep{};
      if (PERSIST && !OVL && t < 64) ep = load_epi(S, C, c);
      // OVL: the log10 loop as eleven written-out iterations with the y store
      // inside (AERO_X_YWRITTEN 2, what is built).  Timing builds: 0, the
      // plain head's form (rolled, the y store inside), whose first iteration
      // waits for every gather; 1, written out with the y stores in a pass of
      // their own under the fold.  Stamps and bench of the three: DESIGN.md §4
#ifndef AERO_X_YWRITTEN
#define AERO_X_YWRITTEN 2
#endif
      constexpr bool YWRITTEN = OVL && AERO_X_YWRITTEN != 0;
      constexpr bool YSTORE_PASS = YWRITTEN && AERO_X_YWRITTEN == 1;  // 2: the y store inside the iterations
      if constexpr (OVL) {
        // every wave has read the image (the barrier above): s_tw, which it
        // covered, is written again from the table load_tw_lds read it from
        // (entry j by thread j, as there), so bit for bit what it was; the
        // fold's closing barrier publishes it before any wave starts the
        // successor's forward transform.  (From the table and not saved in
        // registers: a saved entry would have to be read before the third
        // transform's exchange and live through it, where the kernel's
        // register peak is, or cost a barrier of its own before the image.)
        if (nxt && t < TwLds<L>::LEN) s_tw[t] = twv;
      }
      auto ycalc = [&](double yold, int k) {
        // OVL: log's table from LDS.  From memory, each lookup is a vector-
        // memory load the iteration waits for, and with it (loads count down
        // in issue order) for every table gather still in flight before it
        double lg;
        if constexpr (OVL)
          lg = CO_LOG10_GE1_TAB(fmax(ylds[ypad(k)], 1.0), sm.logtab);
        else
          lg = CO_LOG10_GE1(fmax(ylds[ypad(k)], 1.0));
        const double ynew = yold * 0.9 + 0.1 * 10 * lg;
        yg[k] = ynew;
        ylds[ypad(k)] = ynew;
      };
      auto ybody = [&](int k) {
        const double yold = yp0;
        yp0 = yp1;
        yp1 = yp2;
        yp2 = yload(k + 3 * FT);
        ycalc(yold, k);
      };
      if constexpr (YWRITTEN) {
        // The written-out form: no copy of a look-ahead value from register
        // to register, which waits for the youngest load and with it for
        // every gather still in flight.  The first three iterations use the
        // history values that came back inside |X| and wait for nothing; the
        // fourth uses the first look-ahead load issued here, behind the
        // gathers, which have three iterations more to land.  The y store
        // inside the iterations keeps the waits counted (vmcnt(2), what the
        // compiler emits), so the store pass under the fold is gone.
        // One iteration, yp holding y[k] on entry and y[k + 3 FT] after.  The
        // old value is used up (0.9 y) before the new one is asked for, so
        // that the load can land in the same register: a loaded value handed
        // on to another register is again a copy that waits for the load.
        // For the same reason the load is unconditional (a clamped index) and
        // "no history" (past the bins, yreset) is applied where the value is
        // used.  Only the last iteration, which not every thread has, can be
        // skipped, and by whole waves only: a branch around an earlier one
        // joins paths with different loads in flight, after which the
        // compiler again waits for everything.
        constexpr int NIT = (YLEN + FT - 1) / FT;
        auto ystep = [&](double &yp, auto jc) {
          constexpr int j = decltype(jc)::value;
          constexpr bool full = (j + 1) * FT <= YLEN;  // every thread has this iteration
          static_assert(full || j >= NIT - 1, "one partial iteration, the last");
          if constexpr (j < NIT) {
            const int k = t + j * FT;
            if (full || uni(k) < YLEN) {
              const bool in = full || k < YLEN;
#ifdef AERO_X_NOYREAD
              double a = 20.0 * 0.9;
#else
              double a = ((in && !yreset) ? yp : 20.0) * 0.9;
              asm volatile("" : "+v"(a));
              if constexpr (j + 3 < NIT) yp = yg[min(k + 3 * FT, YLEN - 1)];
#endif
              const double lg = CO_LOG10_GE1_TAB(fmax(ylds[ypad(in ? k : YLEN - 1)], 1.0), sm.logtab);
              const double ynew = a + 0.1 * 10 * lg;
              if (in) {
                ylds[ypad(k)] = ynew;
                if constexpr (!YSTORE_PASS) yg[k] = ynew;
              }
            }
          }
        };
        static_assert(NIT <= 12, "four groups of three iterations cover the bins");
        auto ygroup = [&](auto i0c) {
          constexpr int g = decltype(i0c)::value / 4;
          ystep(yp0, std::integral_constant<int, 3 * g>());
          ystep(yp1, std::integral_constant<int, 3 * g + 1>());
          ystep(yp2, std::integral_constant<int, 3 * g + 2>());
        };
        ygroup(std::integral_constant<int, 0>());
        ygroup(std::integral_constant<int, 4>());
        ygroup(std::integral_constant<int, 8>());
        ygroup(std::integral_constant<int, 12>());
      } else {
#pragma unroll 1
        for (int k = t; k < YLEN; k += FT) ybody(k);
      }
      __syncthreads();
      CSTAMP(7);
      if constexpr (OVL) {
        if constexpr (YSTORE_PASS) {
          // ystore: this thread's new y values, from ylds to memory
#pragma unroll 1
          for (int k = t; k < YLEN; k += FT) yg[k] = ylds[ypad(k)];
        }
        if (t < 64) ep = load_epi(S, C, c);
      }
      // fold search (coarsefreqestimate.cpp:119-140): first strict maximum above 0
      double bv = 0.0;
      int bi = 0x7fffffff;
      for (int r = 0;; ++r) {
        const int i = KB.ilo + t + FT * r;
        if (i >= KB.ihi) break;
        double val = 0;
        for (int j = -1; j <= 1; j++)
          val += (ylds[ypad(i - KB.epb - j - K::YLO)] + ylds[ypad(i + KB.epb + j - K::YLO)]);
        if (val > bv) {
          bv = val;
          bi = i;
        }
      }
      // wave reduce: larger value, then smaller index
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(bv, off, 64);
        const int oi = __shfl_down(bi, off, 64);
        if (ov > bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      if ((t & 63) == 0) {
        red_v[t >> 6] = bv;
        red_i[t >> 6] = bi;
      }
      if (have_pro) pro = uni(pn);
      // the channel's last barrier: past it a wave starts the next channel; the
      // next write of red_* is a whole channel of barriers away
      __syncthreads();
      CSTAMP(8);
      pre = OVL && nxt;
      if constexpr (OVL) {
        // the overlapped head's serial rest: the successor's mix, by the plain
        // head's expression.  x[] holds the table entries gathered under the log10
        // loop and the fold, pcmw[] the PCM halves.  Past the barrier above
        // the waves go straight into the successor's forward transform, with
        // neither of the plain head's barriers: s_tw is whole again since
        // before that barrier, and what the transform writes in the LDS
        // (each wave its own region first) nobody reads any more
        if (nxt) {
#pragma unroll
          for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(x[i].x), "+v"(x[i].y));
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const uint32_t pw = pcmw[i >> 1];
            const double dv = ((double)(int16_t)((i & 1) ? (pw >> 16) : (pw & 0xFFFFu))) / 32768.0;
            x[i] = make_double2(x[i].x * dv, x[i].y * dv);
          }
          // zero_before inside the snapshot (rare, wave-uniform; see the plain head)
          if (s0n < pn.zero_before) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              const long long s = s0n + bitrev<L>(epos<L, 0>(t, i));
              if (s < pn.zero_before) x[i] = make_double2(0.0, 0.0);
            }
          }
        }
        CSTAMP(2);
      }
      if (t == 0) {
        if constexpr (!PERSIST) ep = load_epi(S, C, c);
        for (int w = 1; w < FT / 64; ++w) {
          if (red_v[w] > bv || (red_v[w] == bv && red_i[w] < bi)) {
            bv = red_v[w];
            bi = red_i[w];
          }
        }
        const int zmaxloc = (bv > 0.0) ? bi : N / 2;
        const double nfft = (double)N;
        const double freq_offset_est = -((double)(zmaxloc - nfft / 2)) * (KB.fs / nfft) * 0.5;
        double est;
        int ecd = ep.ecd;
        if (ecd <= 0) {
          est = freq_offset_est;
        } else {
          ecd--;
          est = 0;
        }

        double *ds = S.ds;
        int *is = S.is;
        const double mse = ep.mse;
        HopCtl h;
        h.m2f = ep.m2f;
        h.m2s = ep.m2s;
        h.mcf = ep.mcf;
        h.mcs = ep.mcs;
        h.countdown2 = ep.countdown2;
        h.countdown = ep.countdown;
        h.ecd = ecd;
        h.yres_next = 0;
        h.zb = zero_before;
        h.stepped = false;
        h.step_fc = 0.0;
        unsigned iter = (unsigned)ep.iter;
        int scans = ep.scans;
        const bool gotasignal = hop_control(h, std::integral_constant<int, M>(), KB.fs, est, mse, iter, scans, nk);
        is[IS_HUNT_ITER * C + c] = (int)iter;
        is[IS_HUNT_SCANS * C + c] = scans;
        if (h.stepped) {
          const int k = ep.steps;
          ds[(DS_HUNT_FC0 + (k & 7)) * C + c] = h.step_fc;
          is[IS_HUNT_STEPS * C + c] = k + 1;
        }
        ds[DS_M2_FREQ * C + c] = h.m2f;
        ds[DS_M2_STEP * C + c] = h.m2s;
        ds[DS_MC_FREQ * C + c] = h.mcf;
        ds[DS_MC_STEP * C + c] = h.mcs;
        is[IS_COUNTDOWN2 * C + c] = h.countdown2;
        is[IS_COUNTDOWN * C + c] = h.countdown;
        is[IS_EMPTYCD * C + c] = h.ecd;
        is[IS_YRESET * C + c] = h.yres_next;
        is[IS_HOPS_DONE * C + c] = hops_done + 1;
        S.ls[LS_ZERO_BEFORE * C + c] = h.zb;
        const int hn = ep.hop_n;
        if (hn < S.hop_cap) {
          double *hr = S.hops + ((size_t)c * S.hop_cap + hn) * 6;
          hr[0] = (double)nk;
          hr[1] = est;
          hr[2] = h.m2f;
          hr[3] = h.mcf;
          hr[4] = mse;
          hr[5] = gotasignal ? 1.0 : 0.0;
        }
        S.hop_n[c] = hn + 1;
      }
      CSTAMP(9);
#ifdef AERO_X_STAMPS
      cst_[CSTAMP_N - 1]++;
#endif
      if constexpr (!PERSIST) break;  // one channel per workgroup: no walk
    }
    if constexpr (!PERSIST) break;
  }
#ifdef AERO_X_STAMPS
  if (wave * 64 + lane_now() == 0 && cst_[CSTAMP_N - 1]) {
    cst_[10] = __builtin_amdgcn_s_memtime() - cstart_;
    for (int k = 0; k < CSTAMP_N; ++k) atomicAdd(&g_cstamps[k], cst_[k]);
  }
#endif
}

void coarse_read_stamps(unsigned long long *out) {
#ifdef AERO_X_STAMPS
  (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cstamps), sizeof(unsigned long long) * CSTAMP_N);
  unsigned long long z[CSTAMP_N] = {0};
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_cstamps), z, sizeof z);
#else
  for (int k = 0; k < CSTAMP_N; ++k) out[k] = 0;
#endif
}

// grid: the persistent kinds' workgroup limit (the device's CU count or
// AERO_COARSE_GRID, engine.hip)
// overlap: the persistent kinds' overlapped head (AERO_COARSE_OVERLAP,
// engine.hip); without it every channel takes the plain head
void launch_coarse(hipStream_t st, int mode, const DevState &S, const DevTables &T, int nch, int grid, bool overlap) {
  const dim3 pg(csched::grid(nch, grid < 1 ? 1 : grid));
  switch (mode) {
    case MODE_OQPSK:
      if (overlap)
        hipLaunchKernelGGL((coarse_kernel<MODE_OQPSK, true>), pg, dim3(1024), 0, st, S, T, nch);
      else
        hipLaunchKernelGGL((coarse_kernel<MODE_OQPSK, false>), pg, dim3(1024), 0, st, S, T, nch);
      break;
    case MODE_C8400:
      if (overlap)
        hipLaunchKernelGGL((coarse_kernel<MODE_C8400, true>), pg, dim3(1024), 0, st, S, T, nch);
      else
        hipLaunchKernelGGL((coarse_kernel<MODE_C8400, false>), pg, dim3(1024), 0, st, S, T, nch);
      break;
    case MODE_MSK600: hipLaunchKernelGGL(coarse_kernel<MODE_MSK600>, dim3(nch), dim3(512), 0, st, S, T, nch); break;
    case MODE_MSK1200: hipLaunchKernelGGL(coarse_kernel<MODE_MSK1200>, dim3(nch), dim3(512), 0, st, S, T, nch); break;
    case MODE_MSK600_24K:
      hipLaunchKernelGGL(coarse_kernel<MODE_MSK600_24K>, dim3(nch), dim3(512), 0, st, S, T, nch);
      break;
    case MODE_MSK600_48K:
      hipLaunchKernelGGL(coarse_kernel<MODE_MSK600_48K>, dim3(nch), dim3(512), 0, st, S, T, nch);
      break;
    case MODE_MSK1200_12K:
      hipLaunchKernelGGL(coarse_kernel<MODE_MSK1200_12K>, dim3(nch), dim3(512), 0, st, S, T, nch);
      break;
    case MODE_MSK1200_48K:
      hipLaunchKernelGGL(coarse_kernel<MODE_MSK1200_48K>, dim3(nch), dim3(512), 0, st, S, T, nch);
      break;
    default:  // generic-rate MSK (the kernel does not depend on the bit rate)
      hipLaunchKernelGGL(coarse_kernel<MODE_MSKG600>, dim3(nch), dim3(512), 0, st, S, T, nch);
      break;
  }
}

}  // namespace aero
