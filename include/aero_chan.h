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
/* "device_bytes": device memory held; "vfo_inits": start-kernel launches;
 * "slots_free": free slots held.  Other names: AERO_E_INVALID. */
int aero_chan_stat(aero_chan *c, const char *name, uint64_t *value);

#ifdef __cplusplus
}
#endif
#endif
