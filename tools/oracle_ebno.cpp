// oracle_ebno.cpp — TEST INFRASTRUCTURE ONLY (tools/liboracle_ebno.so).
//
// The oracle (oracle/aero_oracle.cpp, compiled as it stands) plus the one
// demodulator stage it leaves out: the reference's Eb/N0 estimator of an OQPSK
// or C channel, restated plainly below with its own two 96000-entry buffers.
// The engine's kernel (aero-cli_amd/csrc/ebno.hip) keeps no such buffers: it
// reads the values the moving averages drop back out of the AGC ring.  This
// checker does not share that trick, only the estimator's input: after each
// oracle_push of at most 96000 samples, oracle_x_ebno_update takes the new
// fabs(dab) values, in order, out of the oracle's AGC buffer (AGC::Update
// stores the estimator's argument, decode/DSP.cpp:371-374,
// decode/oqpskdemodulator.cpp:399-405).
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

enum { XB_NAN = 0, XB_HIGH = 1, XB_LOW = 2, XB_FLOOR = 3, XB_INTERIOR = 4 };

// OQPSKEbNoMeasure (decode/DSP.cpp:691-722), EbNo started at 0.0 (the
// reference leaves it uninitialised; aero-cli_amd/csrc/ebno.h)
struct XEbNo {
  double Fs, fb, Mean = 0, Var = 0, EbNo = 0.0;
  XMovingAverage E, E2;
  long long br[5] = {0, 0, 0, 0, 0};
  XEbNo(int number, double _Fs, double _fb) : Fs(_Fs), fb(_fb), E(number), E2(number) {}  // DSP.cpp:691-696
  double Update(double sig) {
    E2.Update(sig * sig);                // :704
    Mean = E.Update(sig);                // :705
    double MeanSquared = Mean * Mean;    // :706
    Var = (E2.Val) - (E.Val * E.Val);    // :707
    Var -= (0.024709 * MeanSquared);     // :708
    double mvr = (((Fs * MeanSquared / (2.0 * fb * Var))) * 0.13743);  // :709-710
    if (mvr < 0.000000001) {             // :711
      mvr = 0.000000001;
      br[XB_FLOOR]++;
    }
    double tebno = 10.0 * log10(mvr);    // :713
    bool edge = false;
    if (std::isnan(tebno)) {             // :714
      tebno = 50;
      br[XB_NAN]++;
      edge = true;
    }
    if (tebno > 50.0) {                  // :716
      tebno = 50;
      br[XB_HIGH]++;
      edge = true;
    }
    if (tebno < 0.0) {                   // :718
      tebno = 0;
      br[XB_LOW]++;
      edge = true;
    }
    if (!edge) br[XB_INTERIOR]++;
    EbNo = EbNo * 0.8 + 0.2 * tebno;     // :720
    return EbNo;
  }
};

struct XChan {
  XEbNo m;
  long long taken = 0;
  std::vector<double> series;  // EbNo after every sample
  explicit XChan(double fb) : m(2 * 48000, 48000.0, fb) {}  // OQPSKEbNoMeasure(2 * Fs, Fs, fb), oqpskdemodulator.cpp:39, :235
};
std::map<const oracle_chan *, XChan> g_x;

}  // namespace

extern "C" {

// after an oracle_push of at most 96000 samples (fewer than the AGC buffer
// holds): feeds the new samples to the estimator; returns how many, or -1 for
// a channel that is not OQPSK / C or a push that outran the AGC buffer
long long oracle_x_ebno_update(oracle_chan *c) {
  if (!c || !c->oq) return -1;
  Oqpsk &q = *c->oq;
  auto it = g_x.find(c);
  if (it == g_x.end()) it = g_x.emplace(c, XChan(q.fb)).first;
  XChan &x = it->second;
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
size_t oracle_x_ebno_series(const oracle_chan *c, double *dst, size_t cap) {
  auto it = g_x.find(c);
  if (it == g_x.end()) return 0;
  return copy_out(it->second.series, dst, cap);
}
// how often each branch was taken: NaN -> 50, > 50, < 0 -> 0, the 1e-9 floor, none of the first three
void oracle_x_ebno_branches(const oracle_chan *c, long long *dst5) {
  auto it = g_x.find(c);
  for (int k = 0; k < 5; k++) dst5[k] = it == g_x.end() ? 0 : it->second.m.br[k];
}
// the oracle's AGC buffer and pointer (the ring the engine's walk is checked over): returns its length
size_t oracle_x_agc_ring(const oracle_chan *c, double *dst, size_t cap, int *ptr) {
  if (!c || !c->oq) return 0;
  if (ptr) *ptr = c->oq->agc.AGCMAPtr;
  return copy_out(c->oq->agc.AGCMABuffer, dst, cap);
}
// before oracle_destroy
void oracle_x_ebno_free(const oracle_chan *c) { g_x.erase(c); }
}
