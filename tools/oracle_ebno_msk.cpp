// oracle_ebno_msk.cpp — TEST INFRASTRUCTURE ONLY (tools/liboracle_ebno_msk.so).
//
// The oracle (oracle/aero_oracle.cpp, compiled as it stands) plus the one
// stage of the continuous MSK demodulator it leaves out: the reference's
// MSKEbNoMeasure, restated plainly below with its own two 2 Fs-entry buffers.
// The engine's kernel (aero-cli_amd/csrc/ebno.hip ebno_msk_kernel) keeps one
// ring of inputs and two sums; this checker shares only the estimator's input:
// after each oracle_push / oracle_push_rate of at most Fs samples,
// oracle_x_ebno_msk_update takes the new fabs(dab) values, in order, out of the
// oracle's MSK AGC buffer (AGC::Update stores the estimator's argument,
// decode/DSP.cpp:371-374, decode/mskdemodulator.cpp:305-309).  A push at a new
// rate finds the oracle's Fs changed and constructs the estimator again first,
// as setSettings does (decode/mskdemodulator.cpp:138-140).
#include "../oracle/aero_oracle.cpp"

#include <map>

namespace {

// MovingAverage (decode/DSP.cpp:389-417)
struct XMovingAverage {
  int MASz, MAPtr = 0;
  double MASum = 0, Val = 0;
  std::vector<double> MABuffer;
  explicit XMovingAverage(int number) : MASz(number), MABuffer((size_t)number, 0.0) {}
  double Update(double sig) {
    MASum = MASum - MABuffer[MAPtr];  // DSP.cpp:410
    MASum = MASum + fabs(sig);        // :411
    MABuffer[MAPtr] = fabs(sig);      // :412
    MAPtr++;
    MAPtr %= MASz;
    Val = MASum / ((double)MASz);  // :415
    return Val;
  }
};

enum { XB_NAN = 0, XB_HIGH = 1, XB_NEGARG = 2, XB_INTERIOR = 3, XB_COUNT = 4 };

// MSKEbNoMeasure (decode/DSP.cpp:482-503), EbNo started at 0.0 (the reference
// leaves it uninitialised; aero-cli_amd/csrc/ebno.h)
struct XMskEbNo {
  double Mean = 0, Var = 0, EbNo = 0.0;
  XMovingAverage E, E2;
  long long br[XB_COUNT] = {0, 0, 0, 0};
  explicit XMskEbNo(int number) : E(number), E2(number) {}  // DSP.cpp:482-485
  double Update(double sig) {
    E2.Update(sig * sig);              // :488
    Mean = E.Update(sig);              // :489
    Var = (E2.Val) - (E.Val * E.Val);  // :490
    double alpha = sqrt(2) / Mean;     // :491
    const double arg = ((Var * alpha * alpha) - 0.0085);
    double tebno = 10.0 * (log10(2.0) - log10(arg)) - 5.0;  // :495-496
    bool edge = false;
    if (arg < 0.0) br[XB_NEGARG]++;  // log10 of a negative number: one way into the NaN branch
    if (std::isnan(tebno)) {         // :497
      tebno = 50;
      br[XB_NAN]++;
      edge = true;
    }
    if (tebno > 50.0) {  // :499
      tebno = 50;
      br[XB_HIGH]++;
      edge = true;
    }
    if (!edge) br[XB_INTERIOR]++;
    EbNo = EbNo * 0.8 + 0.2 * tebno;  // :501
    return EbNo;
  }
};

struct XChan {
  double Fs;
  XMskEbNo m;
  long long taken = 0;
  long long br[XB_COUNT] = {0, 0, 0, 0};  // of the estimators constructed before m
  std::vector<double> series;             // EbNo after every sample
  explicit XChan(double fs) : Fs(fs), m((int)(2.0 * fs)) {}  // MSKEbNoMeasure(2.0 * Fs), mskdemodulator.cpp:36
};
std::map<const oracle_chan *, XChan> g_x;

}  // namespace

extern "C" {

// after an oracle_push / oracle_push_rate of at most Fs samples (what the AGC
// buffer holds): feeds the new samples to the estimator, constructed again
// first where the push came at a new rate; returns how many, or -1 for a
// channel that is not continuous MSK or a push that outran the AGC buffer
long long oracle_x_ebno_msk_update(oracle_chan *c) {
  if (!c || !c->msk) return -1;
  Msk &q = *c->msk;
  auto it = g_x.find(c);
  if (it == g_x.end()) it = g_x.emplace(c, XChan(q.Fs)).first;
  XChan &x = it->second;
  if (x.Fs != q.Fs) {  // setSettings: ebnomeasure = new MSKEbNoMeasure(2.0 * Fs)
    for (int k = 0; k < XB_COUNT; k++) x.br[k] += x.m.br[k];
    x.m = XMskEbNo((int)(2.0 * q.Fs));
    x.Fs = q.Fs;
  }
  const long long n = q.nsamples - x.taken;
  const AGC &a = q.agc;
  if (n < 0 || n > a.AGCMASz) return -1;
  for (long long k = 0; k < n; k++) {
    const long long at = (((long long)a.AGCMAPtr - n + k) % a.AGCMASz + a.AGCMASz) % a.AGCMASz;
    x.series.push_back(x.m.Update(a.AGCMABuffer[(size_t)at]));
  }
  x.taken = q.nsamples;
  return n;
}
// EbNo after every sample fed so far; returns their number
size_t oracle_x_ebno_msk_series(const oracle_chan *c, double *dst, size_t cap) {
  auto it = g_x.find(c);
  if (it == g_x.end()) return 0;
  return copy_out(it->second.series, dst, cap);
}
// how often each branch was taken: NaN -> 50, > 50, a negative log argument, neither clamp
void oracle_x_ebno_msk_branches(const oracle_chan *c, long long *dst4) {
  auto it = g_x.find(c);
  for (int k = 0; k < XB_COUNT; k++) dst4[k] = it == g_x.end() ? 0 : it->second.br[k] + it->second.m.br[k];
}
// the oracle's MSK AGC buffer and pointer (the ring the engine's walk is checked over): returns its length
size_t oracle_x_msk_agc_ring(const oracle_chan *c, double *dst, size_t cap, int *ptr) {
  if (!c || !c->msk) return 0;
  if (ptr) *ptr = c->msk->agc.AGCMAPtr;
  return copy_out(c->msk->agc.AGCMABuffer, dst, cap);
}
// before oracle_destroy
void oracle_x_ebno_msk_free(const oracle_chan *c) { g_x.erase(c); }

// The estimator alone, for hand-made inputs: MSKEbNoMeasure(number) with EbNo
// started at ebno0, fed in[0 .. n); out[k] = EbNo after in[k], br4 the branch
// counts as above.
void oracle_x_ebno_msk_feed(int number, double ebno0, const double *in, size_t n, double *out, long long *br4) {
  XMskEbNo m(number);
  m.EbNo = ebno0;
  for (size_t k = 0; k < n; k++) out[k] = m.Update(in[k]);
  for (int k = 0; k < XB_COUNT; k++) br4[k] = m.br[k];
}
}
