/*
 * ebno.h — the reference's Eb/N0 estimator for OQPSK demodulators
 * (OQPSKEbNoMeasure::Update, decode/DSP.cpp:703-722, on two
 * MovingAverage(2 Fs = 96000), decode/DSP.cpp:409-417), as one per-sample step
 * compiled for host and device.
 *
 * The estimator's input is dabval (decode/oqpskdemodulator.cpp:399-402), the
 * value AGC::Update stores as fabs(sig) (decode/DSP.cpp:371-374), so the
 * group's AGC ring S.agc[AGC_LEN][C] already holds the last 192000 inputs.
 * E is a moving average of fabs(sig) over 96000 samples and E2 one of
 * fabs(sig * sig): what E subtracts for sample n is the ring's entry of
 * sample n - 96000, and what E2 subtracts is that entry times itself
 * (a * a with a = fabs(dab) has the bits of fabs(dab * dab)).  Both are 0.0
 * while n < 96000, as the zeroed ring gives them.  So the estimator needs no
 * ring of its own: the two running sums and the smoothed EbNo are its state.
 *
 * The reference never initialises OQPSKEbNoMeasure::EbNo (the constructor,
 * decode/DSP.cpp:691-696, sets Fs, fb, E and E2 only), so its first values
 * depend on what the heap held.  The model here starts EbNo at 0.0; the 0.8 /
 * 0.2 recurrence forgets the start at 0.8^n.
 *
 * Every file that includes this is built with -ffp-contract=off: the
 * operations below are the reference's, in its order, none fused.
 */
#pragma once
#include "aero_math.h"

namespace aero {

constexpr int EBNO_LEN = 96000;  // OQPSKEbNoMeasure(2 * Fs, Fs, fb) (decode/oqpskdemodulator.cpp:39)
constexpr double EBNO_FS = 48000.0;

// MovingAverage::Update of E2 and of E for one sample: a = the sample's
// fabs(dab), old = that of the sample EBNO_LEN before it.  The serial part.
AERO_HD void ebno_sums(double &s1, double &s2, double a, double old) {
  s2 = s2 - old * old;  // E2->Update(sig * sig): MASum - MABuffer[MAPtr]
  s2 = s2 + a * a;      //                        MASum + fabs(sig * sig)
  s1 = s1 - old;        // E->Update(sig)
  s1 = s1 + a;
}

// The sample's tebno from the two sums (decode/DSP.cpp:705-719); depends on
// nothing else, so neighbouring samples' evaluations are independent.
//
// The divisions.  MASum / 96000.0 by div_cw: div_c's quotient behind a
// wave-uniform test of its contract (the sum zero, or at least 2^-900 in
// magnitude, which keeps the quotient by 96000 normal); a wave that holds a
// smaller sum (cancellation can leave any residue) takes the IEEE division.
// The quotient by 2 fb Var is the IEEE division itself: silence gives 0 / 0,
// a carrier that goes away a negative or zero Var, a constant input a Var of
// a few ulps, so neither div_c's nor div_n's contract (a normal quotient, a
// normal divisor and reciprocal) holds there.
AERO_HD double ebno_tebno(double s1, double s2, double fb) {
  const double v2 = div_cw(s2, 96000.0);    // E2->Val
  const double mean = div_cw(s1, 96000.0);  // E->Val
  const double ms = mean * mean;
  double var = v2 - mean * mean;
  var -= 0.024709 * ms;
  double mvr = ((EBNO_FS * ms) / ((2.0 * fb) * var)) * 0.13743;
  if (mvr < 0.000000001) mvr = 0.000000001;
  double t = 10.0 * aero_log10(mvr);
  if (t != t) t = 50;  // std::isnan
  if (t > 50.0) t = 50;
  if (t < 0.0) t = 0;
  return t;
}

AERO_HD double ebno_smooth(double ebno, double t) { return ebno * 0.8 + 0.2 * t; }

// OQPSKEbNoMeasure::Update
AERO_HD double ebno_step(double &s1, double &s2, double ebno, double a, double old, double fb) {
  ebno_sums(s1, s2, a, old);
  return ebno_smooth(ebno, ebno_tebno(s1, s2, fb));
}

// The walk of one channel over the samples [done, nsamp) of its AGC ring
// (time-major, `stride` doubles between rows): sample i lies at row
// (agc_ptr - (nsamp - i)) mod agc_len, agc_ptr the ring pointer after sample
// nsamp - 1, and the entry EBNO_LEN rows before it is the one E / E2 drop.
// Needs nsamp - done <= agc_len - EBNO_LEN (the old entries not yet
// overwritten).  state: {s1, s2, EbNo}.  ebno.hip's kernel does the same with
// the tebno evaluations of four samples side by side; tools/hostcheck.cpp runs
// this one.
AERO_HD void ebno_walk(const double *ring, long long stride, int agc_len, int agc_ptr, long long done,
                       long long nsamp, double fb, double *state) {
  double s1 = state[0], s2 = state[1], eb = state[2];
  long long back = nsamp - done;
  int row = (int)((agc_ptr - back % agc_len + agc_len) % agc_len);
  for (; back > 0; --back) {
    const int orow = row >= EBNO_LEN ? row - EBNO_LEN : row - EBNO_LEN + agc_len;
    eb = ebno_step(s1, s2, eb, ring[(long long)row * stride], ring[(long long)orow * stride], fb);
    row = row + 1 == agc_len ? 0 : row + 1;
  }
  state[0] = s1;
  state[1] = s2;
  state[2] = eb;
}

// ---------------------------------------------------------------- MSK
// The estimator of a continuous MSK demodulator (AERO_F_EBNO_MSK):
// MSKEbNoMeasure::Update (decode/DSP.cpp:487-503) on two MovingAverage(2 Fs)
// (decode/DSP.cpp:409-417), constructed as MSKEbNoMeasure(2.0 * Fs)
// (decode/mskdemodulator.cpp:36) and again by every setSettings (:138-140), fed
// dabval once per sample (:305-309) and emitted once per coarse hop, before
// the hop sample's own Update (:461 through :72-76, :287-296).
//
// Its input is again what AGC::Update stores as fabs(sig), but the MSK AGC is
// AGC(1, Fs): the ring S.agc[Fs][C] holds one second and the window is two.
// So the estimator keeps a ring of its own, time-major [2 Fs][C], of its last
// 2 Fs inputs: sample i (counted from the estimator's construction) is read
// from the AGC ring's row i % Fs, the term E drops is the own ring's row
// i % (2 Fs) (0.0 while i < 2 Fs, as the zeroed ring gives it) and the term E2
// drops is that entry times itself (the argument above), and the sample then
// takes that row.  EbNo is never initialised by the reference
// (decode/DSP.cpp:482-485); it starts at 0.0 here, at open and after every
// rate change (a reset slot of the new rate's group).
//
// There is no lower clamp: EbNo is negative while the window fills, and a
// tebno of -inf (a log argument of +inf) leaves EbNo at -inf for good.

// MASum / (double)MASz for MASz = 2 Fs = len, a group constant and no literal,
// so div_c (whose reciprocal the compiler folds) does not serve.  Its sequence
// does, with rlen = RN(1 / len) taken once per launch by the IEEE division:
// Markstein's theorem asks of the divisor only that rlen is its correctly
// rounded reciprocal, and len is an integer in [24000, 192000], normal with a
// normal reciprocal (a power of two, 32768 .. 131072, makes q0 exact and the
// correction zero).  The numerator is div_cw's: behind a wave-uniform test
// that it is zero or at least 2^-900 in magnitude, which keeps the quotient by
// at most 192000 normal and the residual exact; the sums of a carrier that went
// away are cancellation residues of any size, and a wave that holds a smaller
// one takes the IEEE division.  The sums cannot overflow (at most 192000 terms
// below 2^4 and their squares).
AERO_HD double msk_ebno_div(double a, double len, double rlen) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (__builtin_expect(__all(in_div_cw(a)), 1)) {
    const double q0 = a * rlen;
    const double q = fma(fma(-len, q0, a), rlen, q0);
    return a == 0.0 ? q0 : q;
  }
#else
  (void)rlen;
#endif
  return a / len;
}

// The sample's tebno from the two sums (decode/DSP.cpp:490-500); lg2 is
// aero_log10(2.0), glibc's log10(2.0) bit for bit, taken once per launch.
// sqrt(2) / Mean is the IEEE division: silence gives a zero mean (alpha = inf,
// Var alpha = 0 inf = NaN -> 50), a carrier that went away a residue mean of
// any size and sign, so no contract on the divisor holds.  aero_log10 sees
// whatever Var alpha^2 - 0.0085 is: negative (NaN -> 50), zero (-inf -> +inf
// -> 50), +inf (-> tebno -inf, which stays), and subnormals never (the
// subtraction of 0.0085 leaves none), though the function handles them.
AERO_HD double msk_ebno_tebno(double s1, double s2, double len, double rlen, double lg2) {
  const double v2 = msk_ebno_div(s2, len, rlen);    // E2->Val
  const double mean = msk_ebno_div(s1, len, rlen);  // E->Val = Mean
  const double var = v2 - mean * mean;
  const double alpha = 1.4142135623730951 / mean;  // sqrt(2) / Mean
  double t = 10.0 * (lg2 - aero_log10(((var * alpha) * alpha) - 0.0085)) - 5.0;
  if (t != t) t = 50;  // std::isnan
  if (t > 50.0) t = 50;
  return t;
}

// MSKEbNoMeasure::Update (the sums and the recurrence are the OQPSK ones)
AERO_HD double msk_ebno_step(double &s1, double &s2, double ebno, double a, double old, double len, double rlen,
                             double lg2) {
  ebno_sums(s1, s2, a, old);
  return ebno_smooth(ebno, msk_ebno_tebno(s1, s2, len, rlen, lg2));
}

// The walk of one channel over the samples [done, nsamp) counted from the
// estimator's construction: `agc` the AGC ring (fs rows, `astride` doubles
// between rows, sample i at row i % fs), `own` the estimator's ring (2 fs
// rows, `ostride` between rows), updated.  Needs nsamp - done <= fs (the
// samples' AGC entries not yet overwritten).  state: {s1, s2, EbNo}.
// ebno.hip's kernel does the same with the tebno evaluations of four samples
// side by side; tools/hostcheck.cpp runs this one.
AERO_HD void msk_ebno_walk(const double *agc, long long astride, double *own, long long ostride, int fs,
                           long long done, long long nsamp, double *state) {
  double s1 = state[0], s2 = state[1], eb = state[2];
  const int len = 2 * fs;
  const double dlen = (double)len, rlen = 1.0 / dlen, lg2 = aero_log10(2.0);
  int ar = (int)(done % fs), row = (int)(done % len);
  for (long long i = done; i < nsamp; ++i) {
    const double a = agc[(long long)ar * astride];
    eb = msk_ebno_step(s1, s2, eb, a, own[(long long)row * ostride], dlen, rlen, lg2);
    own[(long long)row * ostride] = a;
    ar = ar + 1 == fs ? 0 : ar + 1;
    row = row + 1 == len ? 0 : row + 1;
  }
  state[0] = s1;
  state[1] = s2;
  state[2] = eb;
}

// device arrays of a flagged OQPSK or C group, or (AERO_F_EBNO_MSK, with a ring
// of its own beside them) of a continuous MSK group (engine.hip layout())
struct EbnoDev {
  double *acc;      // [3][C] s1, s2, EbNo
  long long *done;  // [C] samples the estimator has taken
  double *tr;       // [C][tr_cap][2] (sample index, EbNo) at hop boundaries (AERO_F_TRACE_HOPS), else null
  int *tr_n;        // [C]
  int tr_cap;
};

}  // namespace aero
