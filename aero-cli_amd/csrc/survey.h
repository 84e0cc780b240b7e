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
// the unfinished tail.  *launches: kernel launches made, *segments: segments
// added, *groups: groups a hold completed (0 without one).
int survey_run(Survey *s, hipStream_t st, const float2 *in, long long n, int *launches, uint64_t *segments,
               uint64_t *groups);
// Waits for st; the sums (1 << log2n doubles, cap at least that) and the number
// of segments in them; reset != 0 zeroes both afterwards (not the tail).
int survey_read(Survey *s, hipStream_t st, double *power, size_t cap, uint64_t *segments, int reset);

// The hold beside a survey (aero_chan_survey_hold_* in include/aero_chan.h):
// groups of `group` segments (1 .. 65536) from the next segment completed, a
// ring of `rows` group sums (0 .. 4096), level: 1 << log2n doubles, copied, or
// nullptr.  Allocates and waits for the device.  AERO_E_INVALID: one is on, or
// a value out of range.
int survey_hold_start(Survey *s, int group, int rows, const double *level);
// Waits for the device; nothing to do when none is on.
void survey_hold_stop(Survey *s);
bool survey_hold_on(const Survey *s);
// device memory the hold holds (0 when none is on)
size_t survey_hold_bytes(const Survey *s);
// Waits for st; peak, low and busy (busy may be nullptr; cap at least
// 1 << log2n) and the number of groups in them; reset != 0 then sets them back
// to +0, +infinity, 0 and 0 (not the unfinished group, the ring or the index).
int survey_hold_read(Survey *s, hipStream_t st, double *peak, double *low, uint32_t *busy, size_t cap, uint64_t *groups,
                     int reset);
// Waits for st; the last min(rows, groups completed) group sums, oldest first,
// *first_group the index of the first from the hold's start, *n their number;
// fewer than that fit: the newest cap_rows and AERO_E_FULL.
int survey_hold_rows(Survey *s, hipStream_t st, double *dst, size_t cap_rows, uint64_t *first_group, size_t *n);

}  // namespace aero
