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

// device arrays of a flagged OQPSK or C group (engine.hip layout())
struct EbnoDev {
  double *acc;      // [3][C] s1, s2, EbNo
  long long *done;  // [C] samples the estimator has taken
  double *tr;       // [C][tr_cap][2] (sample index, EbNo) at hop boundaries (AERO_F_TRACE_HOPS), else null
  int *tr_n;        // [C]
  int tr_cap;
};

}  // namespace aero
