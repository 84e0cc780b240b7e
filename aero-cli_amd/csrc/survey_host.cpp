/*
 * survey_host.cpp — aero_survey_peaks (include/aero_chan.h): the carriers in
 * a survey's power spectrum, and aero_survey_activity: which of them a hold
 * saw all the time and which in bursts.  Host only, plain FP64 loops in a
 * fixed order (built without contraction), so tests/survey_model.py and
 * tests/survey_hold_model.py restate them bit for bit.
 */
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <utility>
#include <vector>

#include "../../include/aero_chan.h"

extern "C" int aero_survey_peaks(const double *power, int log2n, int sample_rate, long long center_frequency,
                                 int mix_offset, const aero_survey_peak_cfg *cfg, aero_survey_peak *out, size_t cap,
                                 size_t *n) {
  if (!power || !cfg || !n || (cap && !out) || log2n < 2 || log2n > 24 || sample_rate <= 0 || !(cfg->threshold > 0) ||
      cfg->min_bins < 1 || cfg->merge_gap < 0)
    return AERO_E_INVALID;
  *n = 0;
  const int N = 1 << log2n, H = N / 2;
  std::vector<double> q((size_t)N);
  for (int i = 0; i < N; i++) {
    const double p = power[(i + H) & (N - 1)];
    if (!(p >= 0) || p > DBL_MAX) return AERO_E_INVALID;  // NaN, negative or infinite
    q[i] = p;
  }
  std::vector<double> sorted(q);
  std::sort(sorted.begin(), sorted.end());
  const double floor = sorted[(size_t)(N - 1) / 2];
  const double limit = cfg->threshold * floor;
  // maximal runs of hot bins, merged over gaps of at most merge_gap cold bins
  std::vector<std::pair<int, int>> runs;
  for (int i = 0; i < N;) {
    if (!(q[i] > limit)) {
      i++;
      continue;
    }
    int b = i;
    while (b + 1 < N && q[b + 1] > limit) b++;
    if (!runs.empty() && i - runs.back().second - 1 <= cfg->merge_gap)
      runs.back().second = b;
    else
      runs.push_back({i, b});
    i = b + 1;
  }
  const double fs = (double)sample_rate, dn = (double)N;
  size_t count = 0;
  for (auto &r : runs) {
    const int a = r.first, b = r.second, w = b - a + 1;
    if (w < cfg->min_bins) continue;
    if (count < cap) {
      double sum = 0.0, num = 0.0, den = 0.0;
      for (int i = a; i <= b; i++) {
        const double f = (double)(i - H) * fs / dn, e = q[i] - floor;
        sum = sum + q[i];
        num = num + e * f;
        den = den + e;
      }
      aero_survey_peak &p = out[count];
      p.first_bin = a;
      p.last_bin = b;
      p.bandwidth_hz = (double)w * fs / dn;
      p.ratio = sum / (double)w / floor;
      // cold bins of a merged gap can outweigh the hot ones only with a
      // threshold below 2: then the middle of the run
      p.offset_hz = den > 0 ? num / den : ((double)(a - H) * fs / dn + (double)(b - H) * fs / dn) / 2.0;
      p.frequency = center_frequency + llround(p.offset_hz) - (long long)mix_offset;
    }
    count++;
  }
  *n = count;
  return count > cap ? AERO_E_FULL : AERO_OK;
}

extern "C" int aero_survey_activity(const double *power, uint64_t segments, const double *peak, const double *low,
                                    const uint32_t *busy, uint64_t groups, int group, int log2n, double threshold,
                                    const aero_survey_peak *runs, size_t nruns, aero_survey_act *out) {
  if (!power || !peak || !low || (nruns && (!runs || !out)) || segments == 0 || groups == 0 || group < 1 || log2n < 2 ||
      log2n > 24 || !(threshold > 0))
    return AERO_E_INVALID;
  const int N = 1 << log2n, H = N / 2;
  for (int k = 0; k < N; k++)  // NaN, negative or infinite
    if (!(power[k] >= 0) || power[k] > DBL_MAX || !(peak[k] >= 0) || peak[k] > DBL_MAX) return AERO_E_INVALID;
  for (size_t r = 0; r < nruns; r++)
    if (runs[r].first_bin < 0 || runs[r].last_bin >= N || runs[r].first_bin > runs[r].last_bin) return AERO_E_INVALID;
  std::vector<double> sorted(power, power + N);
  std::sort(sorted.begin(), sorted.end());
  const double floor = sorted[(size_t)(N - 1) / 2];
  const double fgrp = floor / (double)segments * (double)group;
  for (size_t r = 0; r < nruns; r++) {
    const int a = runs[r].first_bin, b = runs[r].last_bin, w = b - a + 1;
    double on = 0.0, off = 0.0;
    uint64_t nb = 0;
    for (int i = a; i <= b; i++) {
      const int k = (i + H) & (N - 1);
      on = on + peak[k];
      off = off + low[k];
      if (busy) nb += busy[k];
    }
    aero_survey_act &o = out[r];
    o.on_ratio = on / (double)w / fgrp;
    o.off_ratio = off / (double)w / fgrp;
    o.duty = busy ? (double)nb / ((double)w * (double)groups) : -1.0;
    o.kind = !(o.on_ratio > threshold) ? AERO_SURVEY_IDLE
                                       : o.off_ratio > threshold ? AERO_SURVEY_CONTINUOUS : AERO_SURVEY_BURST;
  }
  return AERO_OK;
}
