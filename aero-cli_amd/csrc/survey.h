// survey.hip's entry points: the channeliser's wideband carrier survey
// (aero_chan_survey_* in include/aero_chan.h; chan.hip owns the handle)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace aero {

struct Survey;

// A survey on segments of 1 << log2n samples (12, 13 or 14) with the caller's
// window (1 << log2n doubles, copied; nullptr: none), sized for runs of up to
// max_samples input samples.  Allocates on the current device and waits for
// it.  AERO_E_INVALID: another log2n.
int survey_create(int log2n, const double *window, long long max_samples, Survey **out);
// Waits for the device.
void survey_destroy(Survey *s);
// device memory held
size_t survey_bytes(const Survey *s);
// The next n samples of the stream (device memory, read on st): completes the
// segments they fill, adds their power to the sums in stream order and keeps
// the unfinished tail.  *launches: kernel launches made, *segments: segments added.
int survey_run(Survey *s, hipStream_t st, const float2 *in, long long n, int *launches, uint64_t *segments);
// Waits for st; the sums (1 << log2n doubles, cap at least that) and the number
// of segments in them; reset != 0 zeroes both afterwards (not the tail).
int survey_read(Survey *s, hipStream_t st, double *power, size_t cap, uint64_t *segments, int reset);

}  // namespace aero
