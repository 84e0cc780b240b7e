// hostcheck.cpp — CPU harness over the engine's host-side C++ (no GPU):
// aero-cli_amd/csrc/acars_host.cpp (SU dispatch, ISU reassembly, ACARS
// parsing and defragmenting, PChannelHost) and tables_host.cpp (the tables
// the kernels read: CIS, JFFT twiddles, RRC, MSK taps, scrambler, the
// aero-publish channeliser designs).  tests/test_hostcheck.py feeds it the
// oracle's CRC-checked frames and R/T packets and compares the items and
// tables with the oracle's; built plain and, by `build.py --asan`, with
// AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cstring>
#include <string>
#include <vector>

#include "../aero-cli_amd/csrc/acars_host.h"
#include "../aero-cli_amd/csrc/dcd_host.h"
#include "../aero-cli_amd/csrc/ebno.h"
#include "../aero-cli_amd/csrc/tables_host.h"

extern "C" {

void *hc_create(int disable_reassembly) { return new aero::PChannelHost(disable_reassembly != 0); }
void hc_destroy(void *h) { delete static_cast<aero::PChannelHost *>(h); }
void hc_frame(void *h, const uint8_t *info, int len, uint32_t okmask, int formatid) {
  static_cast<aero::PChannelHost *>(h)->frame(info, len, okmask, formatid);
}
void hc_rt_packet(void *h, int r_packet, const uint8_t *info, int len, int nsus) {
  static_cast<aero::PChannelHost *>(h)->rt_packet(r_packet != 0, info, len, nsus);
}
void hc_isu_reset(void *h) { static_cast<aero::PChannelHost *>(h)->isu_reset(); }
// pops up to cap items (emission order); returns the number copied
size_t hc_items(void *h, aero_acars_item *dst, size_t cap) {
  auto &v = static_cast<aero::PChannelHost *>(h)->items;
  const size_t n = v.size() < cap ? v.size() : cap;
  for (size_t i = 0; i < n; i++) dst[i] = v[i];
  v.erase(v.begin(), v.begin() + (long)n);
  return n;
}
// PChannelHost::save into dst (at most cap bytes are written); returns the state's size
size_t hc_save(void *h, uint8_t *dst, size_t cap) {
  std::string s;
  static_cast<aero::PChannelHost *>(h)->save(s);
  if (dst && cap) memcpy(dst, s.data(), s.size() < cap ? s.size() : cap);
  return s.size();
}
// PChannelHost::load: 1 when the state was taken, 0 when it was refused (h is then as a new host)
int hc_load(void *h, const uint8_t *src, size_t n) { return static_cast<aero::PChannelHost *>(h)->load(src, n) ? 1 : 0; }

// The host DCD countdown (dcd_host.h) over one pass of one channel, as
// engine.hip process_slot walks it.  state: {countdown, datacd, edges}, updated.
// syncs: the framing kernel's sync word; jobs: per listed job -1 (a block that
// ends no frame) or the frame's SU count, its CRC-ok mask in masks; down: 3 / 5.
void hc_dcd_pass(int *state, unsigned long long syncs, const int *jobs, const unsigned *masks, int njobs, int down,
                 int tick) {
  aero::DcdHost d;
  d.cd = state[0];
  d.dcd = state[1];
  d.edges = state[2];
  aero::DcdPass p;
  p.syncs = syncs;
  for (int j = 0; j < njobs; j++) {
    p.job(d);
    for (int k = 0; k < jobs[j]; k++) d.su((masks[j] >> k) & 1, down);
  }
  p.finish(d, tick != 0);
  state[0] = d.cd;
  state[1] = d.dcd;
  state[2] = d.edges;
}

// The Eb/N0 kernel's walk (ebno.hip) in plain C++ over ebno.h's step, for one
// channel whose AGC ring is `ring` (agc_len doubles, agc_ptr the pointer after
// sample nsamp - 1): takes the samples [done, nsamp).  state: {s1, s2, EbNo},
// updated.  Returns 0, or -1 for a span the ring no longer holds.
int aero_x_ebno_run(const double *ring, int agc_len, int agc_ptr, long long done, long long nsamp, double fb,
                    double *state) {
  if (!ring || !state || agc_len < aero::EBNO_LEN || agc_ptr < 0 || agc_ptr >= agc_len || nsamp < done ||
      nsamp - done > (long long)(agc_len - aero::EBNO_LEN))
    return -1;
  aero::ebno_walk(ring, 1, agc_len, agc_ptr, done, nsamp, fb, state);
  return 0;
}

// The MSK Eb/N0 kernel's walk (ebno.hip ebno_msk_kernel) over ebno.h's step,
// for one channel at rate fs: `agc` its AGC ring (fs doubles, sample i at
// i % fs), `own` the estimator's ring (2 fs doubles, updated); takes the samples
// [done, nsamp) counted from the estimator's construction.  state: {s1, s2,
// EbNo}, updated.  Returns 0, or -1 for a span the AGC ring no longer holds.
int aero_x_ebno_msk_run(const double *agc, double *own, int fs, long long done, long long nsamp, double *state) {
  if (!agc || !own || !state || fs < 1 || done < 0 || nsamp < done || nsamp - done > (long long)fs) return -1;
  aero::msk_ebno_walk(agc, 1, own, 1, fs, done, nsamp, state);
  return 0;
}
// aero_log10(2.0), the constant of the MSK step (glibc's log10(2.0) bit for bit)
double aero_x_ebno_msk_lg2(void) { return aero::aero_log10(2.0); }

void hc_cis(double *cis) { aero::host_cis(cis); }
void hc_twiddles(int nfft, double *tw, double *twi) { aero::host_twiddles(nfft, tw, twi); }
int hc_rrc(double alpha, int firsize, double fs, double symfreq, double *pts) {
  return aero::host_rrc(alpha, firsize, fs, symfreq, pts);
}
void hc_msk_taps(int sps, double *taps) { aero::host_msk_taps(sps, taps); }
void hc_scrambler(uint8_t *pre) { aero::host_scrambler(pre); }
int hc_pub_low_pass(double gain, double fs, double cutoff, double tw, float *taps, int cap) {
  return aero::host_pub_low_pass(gain, fs, cutoff, tw, taps, cap);
}
void hc_pub_hilbert(int len, int fs, float *pts) { aero::host_pub_hilbert(len, fs, pts); }
int hc_pub_osc_len(double fs) { return aero::host_pub_osc_len(fs); }
void hc_pub_osc(double fs, double freq, float *q) { aero::host_pub_osc(fs, freq, q); }
}
