/*
 * aero_chan.h — C ABI of the MI355X channeliser (aero-publish's VFO tree).
 *
 * Replaces the CPU channeliser of airframesio/aero-cli's aero-publish:
 * Publisher::loadSettings (publish/publisher.cpp:55-227) builds main VFOs and
 * their sub-VFOs from the SDRReceiver INI, Publisher::demodData
 * (publish/publisher.cpp:285-306) hands every CF32 read to the main VFOs, and
 * vfo::process (publish/vfo.cpp:154-186) mixes, half-band decimates and
 * USB-demodulates each sub-VFO into int16 audio that ZmqPublisher::publish
 * (publish/zmqpublisher.cpp:61-73) sends to aero-decode.  Here the audio stays
 * in HBM: aero_chan_feed pushes it into aero_engine channels directly.
 *
 * Numerics: FP32, bit-exact with the reference's sample-by-sample code,
 * including the half-band queue copy-back that keeps the wrong slots
 * (publish/dsp.cpp:163-172) and the oscillator's first-sample quirk
 * (publish/oscillator.cpp:12-27).  Errors are the AERO_E_* codes of
 * aero_engine.h.
 */
#ifndef AERO_CHAN_H
#define AERO_CHAN_H

#include <stddef.h>
#include <stdint.h>

#include "aero_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aero_chan aero_chan;

/* [General] keys of the INI (publish/publisher.cpp:65-113) plus the GPU side */
typedef struct {
  int device;            /* HIP device */
  int sample_rate;       /* 288000, 1536000 or 1920000 (publish/publisher.h:32) */
  int center_frequency;  /* Hz */
  int mix_offset;        /* added to every [vfos] frequency (publisher.cpp:160) */
  int correct_dc_bias;   /* demodData's DC removal (publisher.cpp:292-296) */
  int max_blocks;        /* reads (blocks) batched per aero_chan_run */
  int flags;             /* AERO_CHAN_F_* */
} aero_chan_cfg;

/* one [main_vfos] entry (publisher.cpp:115-148) */
typedef struct {
  int frequency;
  int out_rate;
  int compress_scale;    /* 0: 1 */
  int publish;           /* zmq_address and zmq_topic set: 4-bit IQ output when it has no sub-VFOs */
} aero_chan_main;

/* one [vfos] entry (publisher.cpp:151-222) */
typedef struct {
  int frequency;
  int data_rate;         /* out_rate 0: 600 -> 12000, 1200 -> 24000, other -> 48000 */
  int out_rate;
  int filter_bandwidth;  /* 0: no audio low-pass */
  float gain;            /* INI "gain" (percent) */
  int skip;              /* not computed by this process (multi-GPU sharding) */
} aero_chan_vfo;

#define AERO_CHAN_F_HOST_OUT 0x1 /* keep every output for aero_chan_pop_* */

/* Publisher::loadSettings.  At most 3 main VFOs (VFOsub[3], publisher.h:50);
 * a [vfos] entry that no main VFO covers is refused when main VFOs exist
 * (the reference would feed it another main VFO's stream) and never runs when
 * there are none (as in the reference). */
int aero_chan_create(const aero_chan_cfg *cfg, const aero_chan_main *mains, int nmain, const aero_chan_vfo *vfos,
                     int nvfo, aero_chan **out);
void aero_chan_destroy(aero_chan *c);

/* complex samples per read: buflen / 2 (publisher.cpp:92-100) */
int aero_chan_block_len(aero_chan *c, int *block_len);
/* [vfos] entry v: info5 = {main index (-1: none), output rate, output samples
 * per block, half-band stages, late decimation 0/5/6} */
int aero_chan_vfo_info(aero_chan *c, int v, int *info5);
/* [main_vfos] entry m: info3 = {output rate, output samples per block, half-band stages} */
int aero_chan_main_info(aero_chan *c, int m, int *info3);

/* nblocks whole reads of interleaved CF32 (SOAPY_SDR_CF32, publisher.cpp:254);
 * dev != 0: a HIP device pointer.  Copied before returning.  At most
 * max_blocks reads may be pending between two aero_chan_run calls: a push
 * beyond that returns AERO_E_FULL (nothing of the excess is taken), except
 * with AERO_CHAN_F_HOST_OUT, where the full batch runs first and its
 * outputs are kept for aero_chan_pop_*. */
int aero_chan_push(aero_chan *c, const float *iq, size_t nblocks, int dev);
/* processes the pending reads (asynchronous; aero_chan_sync waits) */
int aero_chan_run(aero_chan *c);
int aero_chan_sync(aero_chan *c);
/* device view of the last batch's int16 audio of [vfos] entry v (valid until
 * the next push/run; call aero_chan_sync before reading it on another stream) */
int aero_chan_vfo_output(aero_chan *c, int v, const int16_t **dptr, size_t *n);
/* AERO_CHAN_F_HOST_OUT: pop the audio of [vfos] entry v / the 4-bit IQ of main VFO m */
int aero_chan_pop_audio(aero_chan *c, int v, int16_t *dst, size_t cap, size_t *n);
int aero_chan_pop_iq(aero_chan *c, int m, int8_t *dst, size_t cap, size_t *n);
/* vfo::transmitData -> ZMQ -> Decoder::audioReceived (vfo.cpp:289-313,
 * decode/decode.cpp:283-366) without the hop: the last batch's audio of every
 * [vfos] entry v with ch[v] >= 0 goes to engine channel ch[v]
 * (aero_push_pcm_dev).  Each read of the batch is one message, as
 * vfo::process publishes one per read (vfo.cpp:184): an 8400-bps C channel
 * prefilters and a burst channel takes (writeDataSlot) every read on its own,
 * however many reads the batch held; the continuous kinds do not depend on
 * the message boundaries.  Call once per aero_chan_run. */
int aero_chan_feed(aero_chan *c, aero_engine *e, const int *ch);

/*
 * [vfos] entries while the receiver runs.
 *
 * Every stage of a VFO has finite memory and its NCO is indexed by the reads
 * the channeliser has taken, so a VFO that starts at read k with zero filter
 * histories produces, after aero_chan_vfo_settle output samples, bit for bit
 * the audio of a VFO that was there from read 0, and from its first sample
 * the audio of such a VFO whose input was silent until read k.  A VFO's
 * output does not depend on when it was opened, and no other VFO's audio and
 * no main VFO's IQ changes by one bit when one comes or goes.
 *
 * The ids of aero_chan_create's entries are 0 .. nvfo-1.  A VFO that is
 * closed or skipped gives its device slot to a free list of its shape (main
 * VFO, half-band stages, late decimation, samples per read, output rate and
 * audio filter, which fix the tap counts); a VFO that starts takes the free
 * slot of its shape with the smallest index.  Where there is none it
 * allocates one, which waits for the device; aero_chan_reserve avoids that.
 * The starts since the last read share one kernel launch at the next
 * aero_chan_push / aero_chan_run, which clears their histories and fills
 * their NCO tables on the device.
 *
 * aero_chan_vfo_open, _close and _skip first run the reads that are pushed
 * and not yet run, as aero_chan_run does (without the opened VFO, with the
 * closed one): call them after aero_chan_feed / aero_chan_vfo_output have
 * used the previous batch.
 */
/* Adds one [vfos] entry, resolved as aero_chan_create resolves them (the
 * same AERO_E_INVALID cases; also when no main VFO covers the frequency, or
 * the one that does publishes 4-bit IQ, which a sub-VFO would silence).
 * *v_out: the smallest free id.  The VFO takes part from the first read
 * pushed after the call; before the first read at all it is exactly an entry
 * given to aero_chan_create.  cfg->skip: the id is taken, nothing runs. */
int aero_chan_vfo_open(aero_chan *c, const aero_chan_vfo *cfg, int *v_out);
/* Audio of v that has not been popped is dropped.  Afterwards every call
 * that takes v returns AERO_E_INVALID and aero_chan_feed ignores ch[v], until
 * the id is given out again. */
int aero_chan_vfo_close(aero_chan *c, int v);
/* The skip flag of entry v (from create or open) at run time: the id and the
 * configuration stay; skip = 1 releases the slot as close does (audio that is
 * not popped stays), skip = 0 starts the VFO as open does.  To hand a VFO to
 * another process, the receiver clears its skip one read before the owner
 * sets its own: the receiver's audio from its second read on continues the
 * owner's when the settle time is below one read. */
int aero_chan_vfo_skip(aero_chan *c, int v, int skip);
/* n free slots of the shape `like` resolves to (and room in the job blobs),
 * so that opens of that shape allocate nothing */
int aero_chan_reserve(aero_chan *c, const aero_chan_vfo *like, int n);
/* one past the largest id in use: the length of aero_chan_feed's ch array */
int aero_chan_vfo_count(aero_chan *c, int *n);
/* output samples after a start within which v may differ from a VFO that was
 * always there: 124 (Hilbert) + audio taps + ceil(late taps / late) + 12 per
 * half-band stage of the VFO and of its main VFO */
int aero_chan_vfo_settle(aero_chan *c, int v, size_t *samples);
/* "device_bytes": device memory held (a survey's and its hold's buffers while
 * they are on); "vfo_inits": start-kernel launches; "slots_free": free slots
 * held; "survey_launches": kernel launches made for surveys and their holds
 * since creation (0 while none was ever started); "survey_segments": segments
 * accumulated since creation; "survey_groups": groups a hold completed since
 * creation.  Other names: AERO_E_INVALID. */
int aero_chan_stat(aero_chan *c, const char *name, uint64_t *value);

/*
 * Wideband carrier survey: an averaged power spectrum of the input, to find
 * where [vfos] entries belong (the reference has no counterpart).
 *
 * Off by default; while off the channeliser launches and allocates nothing
 * for it.  While a survey is on:
 *
 *  - It reads the sample stream the VFOs read: the pushed CF32 reads in
 *    order, after the DC removal when correct_dc_bias is set and raw
 *    otherwise.  Samples are counted from the first read that runs after
 *    aero_chan_survey_start.
 *  - Segment s is samples [s*N, (s+1)*N) of that stream, N = 2^log2n, log2n
 *    12, 13 or 14.  No read length is a multiple of N, so a segment straddles
 *    reads, batches and aero_chan_run calls; the unfinished tail (< N
 *    samples) is carried on the device.
 *  - Per segment, in FP64 without contraction, in this order:
 *      x[i] = (double)re[i] * w[i], (double)im[i] * w[i]  with the caller's
 *             window w (N doubles; NULL: no multiplication at all);
 *      X    = the forward radix-2 transform of the decoder (JFFT,
 *             decode/jfft.cpp:114-212, with JFFT::init's tables), bit for bit;
 *      p[k] = X[k].re * X[k].re + X[k].im * X[k].im, natural bin order
 *             k = 0 .. N-1 (bin k: k * sample_rate / N above the centre for
 *             k < N/2, (k - N) * sample_rate / N for the upper half);
 *      acc[k] = acc[k] + p[k], the sum over segments taken in stream order.
 *    The result equals that sequential computation in every bit.
 *  - The survey does not depend on the VFOs: entries may be opened, closed and
 *    skipped while it runs, and no VFO's audio and no main VFO's IQ changes by
 *    one bit when a survey starts, runs or stops.
 *
 * aero_chan_survey_start and _stop first run the reads that are pushed and
 * not yet run, as aero_chan_run does (without the survey / with it): call
 * them after aero_chan_feed / aero_chan_vfo_output have used the previous
 * batch.  Both wait for the device (they allocate / free the buffers).
 */
typedef struct {
  int log2n;             /* 12, 13 or 14 */
  const double *window;  /* 2^log2n doubles, copied; NULL: none */
} aero_chan_survey_cfg;
/* AERO_E_INVALID: another log2n, or a survey is already on.  The grid starts
 * at the next read pushed. */
int aero_chan_survey_start(aero_chan *c, const aero_chan_survey_cfg *cfg);
/* Drops sums, count and tail (AERO_E_INVALID: none is on).  A later start
 * begins a fresh grid at the next read. */
int aero_chan_survey_stop(aero_chan *c);
/* Waits for the runs launched so far (reads pushed and not yet run are not
 * run), then power[0 .. N) = acc and *segments = the number of segments in
 * it; cap < N: AERO_E_INVALID.  reset != 0 then zeroes both; the carried tail
 * and the segment grid are not reset. */
int aero_chan_survey_read(aero_chan *c, double *power, size_t cap, uint64_t *segments, int reset);

/*
 * The carriers in a survey spectrum.  A host function: no aero_chan and no GPU
 * is needed.  Plain FP64 loops in the order given, without contraction:
 *
 *  1. q[i] = power[(i + N/2) mod N], i = 0 .. N-1: ascending frequency,
 *     f_i = (double)(i - N/2) * (double)sample_rate / (double)N.
 *  2. floor = the lower median of q: element (N-1)/2 of the sorted copy.
 *  3. Bin i is hot when q[i] > threshold * floor (all-zero input: none).
 *  4. Maximal runs of hot bins; runs separated by at most merge_gap cold bins
 *     are merged (the cold bins belong to the merged run); then runs shorter
 *     than min_bins are dropped.  A run does not wrap around the band edge.
 *  5. Per run [a, b], sums in ascending i: first_bin = a, last_bin = b
 *     (indices into q); bandwidth_hz = (b - a + 1) * sample_rate / N;
 *     ratio = (sum q[i]) / (b - a + 1) / floor (infinite over a zero floor);
 *     offset_hz = sum((q[i] - floor) * f_i) / sum(q[i] - floor), or
 *     (f_a + f_b) / 2 where that divisor is not positive.
 *  6. frequency = center_frequency + llround(offset_hz) - mix_offset: the
 *     value a [vfos] entry's `frequency` takes to be centred on the carrier.
 *     The channeliser's mixers move the input by center_frequency -
 *     (frequency + mix_offset) (publisher.cpp:115-222), so a carrier offset_hz
 *     above the centre lands on 0 Hz of that entry, and an entry 1000 Hz below
 *     `frequency` puts it at 1000 Hz of its upper-sideband audio.
 *
 * Peaks are written in ascending frequency.  *n is the number found; when it
 * exceeds cap the first cap are written and AERO_E_FULL is returned.
 * AERO_E_INVALID: log2n outside 2 .. 24, sample_rate <= 0, threshold <= 0,
 * min_bins < 1, merge_gap < 0, or a power value that is negative or not
 * finite.
 */
typedef struct {
  double threshold;  /* hot: above threshold x the median bin */
  int min_bins;      /* shortest run reported */
  int merge_gap;     /* cold bins two runs may be apart and still be one */
} aero_survey_peak_cfg;
typedef struct {
  double offset_hz, bandwidth_hz, ratio;
  long long frequency;
  int first_bin, last_bin;
} aero_survey_peak;
int aero_survey_peaks(const double *power, int log2n, int sample_rate, long long center_frequency, int mix_offset,
                      const aero_survey_peak_cfg *cfg, aero_survey_peak *out, size_t cap, size_t *n);

/*
 * Peak / min hold, duty and a waterfall beside a survey that is on.  The
 * survey's sum averages a carrier that is on the air a few percent of the time
 * (the burst R/T and C-band channels) away; the hold keeps, per bin, what
 * groups of `group` consecutive segments reached.
 *
 * Group g is segments [g*group, (g+1)*group) of the survey, counted from the
 * first segment the survey completes after aero_chan_survey_hold_start (that
 * segment may hold tail samples from before the call).  Per completed
 * segment, in stream order, per bin k, in FP64 without contraction, with p
 * the survey's p[k] of that segment:
 *     gsum[k] = gsum[k] + p[k]                       gsum starts at +0.0
 *   and after the group's last segment, with s = gsum[k]:
 *     if (s > peak[k]) peak[k] = s;                  peak starts at +0.0
 *     if (s < low[k]) low[k] = s;                    low starts at +infinity
 *     if (s > level[k]) busy[k] += 1;                with a level; busy starts at 0
 *     row g mod rows of the ring [k] = s;            with rows > 0
 *     gsum[k] = +0.0.
 * A NaN sum changes none of peak, low and busy; a level that is NaN or
 * infinite is never exceeded.  A group straddles reads, batches and
 * aero_chan_run calls as a segment does: gsum and the number of segments in it
 * are carried.  The results equal that sequential computation in every bit.
 *
 * The hold reads what the survey computed and writes buffers of its own: the
 * survey's sums, every VFO's audio and every main VFO's IQ are bit for bit
 * what they are without it.  One more kernel launch per run that completes a
 * segment; nothing is launched or allocated for it while none is on.
 */
typedef struct {
  int group;            /* segments per group, 1 .. 65536 */
  int rows;             /* group sums kept for aero_chan_survey_hold_rows, 0 .. 4096 */
  const double *level;  /* 2^log2n doubles, natural bin order, copied; NULL: busy is not counted */
} aero_chan_survey_hold_cfg;
/* AERO_E_INVALID: no survey is on, a hold is already on, or group / rows out
 * of range.  As aero_chan_survey_start it first runs the reads that are
 * pushed and not yet run (without the hold), and it waits for the device (it
 * allocates). */
int aero_chan_survey_hold_start(aero_chan *c, const aero_chan_survey_hold_cfg *cfg);
/* Drops the hold's state and memory (AERO_E_INVALID: none is on); waits for
 * the device.  The survey goes on.  aero_chan_survey_stop ends a hold that is
 * on. */
int aero_chan_survey_hold_stop(aero_chan *c);
/* Waits for the runs launched so far, then peak[0 .. N), low[0 .. N) and, when
 * busy is not NULL, busy[0 .. N) in natural bin order, and *groups = the
 * number of groups in them; cap < N: AERO_E_INVALID.  reset != 0 then sets
 * them back to +0.0, +infinity, 0 and 0 groups.  The unfinished group, the
 * group grid, the ring and the group index are not reset (as the survey's
 * read leaves its tail), and the survey's read, with or without reset, does
 * not touch the hold.  busy has 32 bits: reset before 2^32 groups. */
int aero_chan_survey_hold_read(aero_chan *c, double *peak, double *low, uint32_t *busy, size_t cap, uint64_t *groups,
                               int reset);
/* The waterfall: waits for the runs launched so far, then the last
 * min(rows, groups completed since the start) group sums, oldest first, N
 * doubles each; *first_group = the index of the first row written, counted
 * from the hold's start (resets do not change it), *n = the rows written.
 * When cap_rows is smaller than that count: the newest cap_rows and
 * AERO_E_FULL.  rows == 0: AERO_E_INVALID. */
int aero_chan_survey_hold_rows(aero_chan *c, double *dst, size_t cap_rows, uint64_t *first_group, size_t *n);

/*
 * Continuous or burst: what a hold says about the carriers of a spectrum.  A
 * host function: no aero_chan and no GPU is needed.  The intended use is
 * aero_survey_peaks on the hold's peak array (a valid spectrum for it), then
 * this function on the runs it returns, with the survey's sums of the same
 * period as `power`.  Plain FP64 in this order, without contraction, N =
 * 2^log2n:
 *
 *  1. floor = the lower median of power: element (N-1)/2 of the sorted copy,
 *     as step 2 of aero_survey_peaks.
 *  2. fgrp = floor / (double)segments * (double)group: the floor of a group sum.
 *  3. Per run, with its first_bin .. last_bin (indices i into the ascending
 *     order), k = (i + N/2) mod N and w = last_bin - first_bin + 1, sums in
 *     ascending i and IEEE divisions (infinite or NaN over a zero floor):
 *       on_ratio  = (sum peak[k]) / w / fgrp
 *       off_ratio = (sum low[k]) / w / fgrp
 *       duty      = (double)(sum busy[k]) / ((double)w * (double)groups), or
 *                   -1.0 when busy is NULL.
 *  4. kind = AERO_SURVEY_IDLE unless on_ratio > threshold; else
 *     AERO_SURVEY_CONTINUOUS when off_ratio > threshold; else AERO_SURVEY_BURST.
 *
 * AERO_E_INVALID: segments == 0, groups == 0, group < 1, log2n outside
 * 2 .. 24, threshold <= 0, a run whose bins are outside [0, N) or reversed, or
 * a power / peak value that is negative or not finite (low may be +infinity).
 */
#define AERO_SURVEY_IDLE 0
#define AERO_SURVEY_CONTINUOUS 1
#define AERO_SURVEY_BURST 2
typedef struct {
  double on_ratio, off_ratio, duty;
  int kind;
} aero_survey_act;
int aero_survey_activity(const double *power, uint64_t segments, const double *peak, const double *low,
                         const uint32_t *busy, uint64_t groups, int group, int log2n, double threshold,
                         const aero_survey_peak *runs, size_t nruns, aero_survey_act *out);

#ifdef __cplusplus
}
#endif
#endif
