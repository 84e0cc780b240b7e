// oracle_ranges.cpp — TEST INFRASTRUCTURE ONLY (tools/liboracle_ranges.so).
//
// The range probe of tests/cont_inputs.py: the oracle (oracle/aero_oracle.cpp)
// compiled as it stands with its observation hook ORACLE_OBS defined, so that
// every libm call of the three continuous per-sample loops and every numerator
// of a division that the kernels shorten is seen before it is made.  One entry
// point runs a stream through one continuous channel and returns, per site,
// the calls, the calls outside the device's branch-free range or division
// contract, the calls with a nonzero subnormal argument and the largest
// |argument|.  Nothing of the oracle is restated, and the ranges are the
// kernels' own: the in_* tests that aero-cli_amd/csrc/aero_math.h puts inside
// its __all(...), called here on the host.  Only the contract of div_c, div_n
// and div_r is restated, with the lines it follows: it is a comment there,
// tested nowhere on the device.
#include <cmath>
#include <cstdint>
#include <cstring>

static void oracle_obs(int site, double a, double b);
#define ORACLE_OBS(site, a, b) oracle_obs(site, a, b)
#include "../oracle/aero_oracle.cpp"
#include "../aero-cli_amd/csrc/aero_math.h"

namespace {

struct Site {
  double calls, outside, subnormal, maxabs;
};
thread_local Site g_sites[OBS_SITES];

inline bool subn(double x) { return x != 0.0 && std::fabs(x) < 0x1p-1022; }

// div_c, div_r, div_n (aero_math.h:86-87): the numerator is zero or at least 2^-969
inline bool in_div(double a) { return a == 0.0 || std::fabs(a) >= 0x1p-969; }
// div_r's further conditions (aero_math.h:81-83): b and 1/b normal, the quotient normal
inline bool in_div_r(double a, double b) {
  const double m = std::fabs(b), q = std::fabs(a / b);
  return in_div(a) && m >= 0x1p-1022 && m <= 0x1p1022 && (a == 0.0 || (q >= 0x1p-1022 && q <= 0x1p1023));
}
}  // namespace

static void oracle_obs(int site, double a, double b) {
  Site &s = g_sites[site];
  bool in = true;
  switch (site) {
    case OBS_HYPOT:
    case OBS_MSE_HYPOT:
      in = aero::in_hypot_w(a, b);
      break;
    case OBS_ATAN2:
      in = aero::in_atan2_bf(a, b);
      break;
    case OBS_TANH:
    case OBS_TANH_ST:
      in = aero::in_tanh_bf(a);
      break;
    case OBS_SINCOS:
      in = aero::in_sincos_bf(a);
      break;
    case OBS_DIV_TW:
      in = in_div_r(a, b);
      b = 0.0;  // the divisor is no argument of the statistics
      break;
    case OBS_DIV_M2PTR:
      in = aero::in_div_cw(a);
      break;
    default:  // OBS_DIV_AGC, OBS_DIV_NUDGE, OBS_DIV_MSSUM
      in = in_div(a);
      break;
  }
  s.calls += 1;
  if (!in) s.outside += 1;
  if (subn(a) || subn(b)) s.subnormal += 1;
  const double m = std::fmax(std::fabs(a), std::fabs(b));
  if (m > s.maxabs) s.maxabs = m;  // a NaN never enters: the traces are checked for those
}

// One continuous channel of `bitrate` (10500, 8400: fs is 48000; 600, 1200: an
// MSK channel at `fs`) over pcm[0, n) in messages of `msg` samples.  out:
// OBS_SITES records of (calls, outside, subnormal, largest |argument|).
// Returns OBS_SITES, or -1 for a bit rate without a continuous channel.
extern "C" int oracle_ranges(int bitrate, int fs, const int16_t *pcm, size_t n, size_t msg, double *out) {
  oracle_chan *c = oracle_create(bitrate, 0);
  if (!c) return -1;
  for (int i = 0; i < OBS_SITES; i++) g_sites[i] = Site{0, 0, 0, 0};
  if (!msg) msg = n;
  for (size_t p = 0; p < n; p += msg) oracle_push_rate(c, pcm + p, n - p < msg ? n - p : msg, fs);
  oracle_destroy(c);
  for (int i = 0; i < OBS_SITES; i++) {
    out[4 * i + 0] = g_sites[i].calls;
    out[4 * i + 1] = g_sites[i].outside;
    out[4 * i + 2] = g_sites[i].subnormal;
    out[4 * i + 3] = g_sites[i].maxabs;
  }
  return OBS_SITES;
}
