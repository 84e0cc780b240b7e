/*
 * aero_engine.h — C ABI of the MI355X-native Aero demodulation engine.
 *
 * Drop-in boundary for aero-decode's per-VFO DSP chain.  In the reference
 * (airframesio/aero-cli, decode/) the boundary is a set of Qt signal/slot
 * edges wired in decode/decode.cpp:168-241; each entry point below names the
 * edge it replaces.  Plain pointers and sizes only; no torch/HIP types.
 *
 * Threading: one host thread per engine (the reference runs all DSP on the
 * Qt main thread); push/run/pop on one engine must be serialised by the
 * caller.  Ownership: the caller owns every buffer it passes; the engine
 * copies input before returning and copies output into caller arrays.
 * Errors: 0 = OK, negative = AERO_E_* (aero_strerror).
 */
#ifndef AERO_ENGINE_H
#define AERO_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AERO_OK 0
#define AERO_E_INVALID (-1)    /* bad argument / unsupported bit rate      */
#define AERO_E_NOMEM (-2)      /* device or host allocation failed         */
#define AERO_E_HIP (-3)        /* HIP runtime error                        */
#define AERO_E_NOGPU (-4)      /* no gfx950 device / kernels not loadable  */
#define AERO_E_FULL (-5)       /* channel table or PCM ring full           */
#define AERO_E_RATE (-6)       /* sample rate the channel kind does not serve (MSK: outside [12000, 96000] Hz) */
#define AERO_E_DEVICE (-7)     /* a kernel gave up (wave hand-off timeout, a DCD tick ring overrun): the run's outputs are invalid */

/* engine flags */
#define AERO_F_TRACE_PT 0x1    /* keep the rotated pt_qpsk trace (parity tests)      */
#define AERO_F_TRACE_BLOCKS 0x2 /* keep decoded Viterbi blocks (parity tests)         */
#define AERO_F_TIMING 0x4      /* HIP-event timing of every kernel launch            */
#define AERO_F_TRACE_SOFT 0x8  /* keep delivered soft bits for aero_pop_softbits      */
#define AERO_F_TRACE_HOPS 0x10 /* keep per-hop coarse-estimator records              */
#define AERO_F_TRACE_FRAMES 0x20 /* keep per-frame infofield records (aero_pop_frames) */
#define AERO_F_DCD_TICK 0x40   /* continuous OQPSK: run AeroL's 1 s data-carrier-detect
                                  timer (decode/aerol.cpp:900-902, 1043-1058) on the
                                  sample clock, one tick per 48000 input samples, as
                                  the shipped binary's event loop fires it once per
                                  second of real-time audio (decode/main.cpp:106).
                                  Without it the timer never fires: after a lost
                                  message a channel that has synced once searches
                                  for the UW only at the expected frame boundary.
                                  Continuous OQPSK only: burst channels ignore it
                                  (AERO_F_DCD_TICK_BURST is theirs), and so do
                                  continuous MSK and C channels, whose
                                  DataCarrierDetect then only ever rises
                                  (AERO_F_DCD_TICK_CONT is theirs) */
#define AERO_F_DCD_TICK_BURST 0x80 /* burst channels (10500 OQPSK, 600/1200 MSK): run
                                  the same timer.  A sync sets datacd and a countdown
                                  of 12 that only the timer takes down (the burst
                                  window ends after 10500 soft bits, several bursts
                                  later, decode/aerol.cpp:2008-2028); the fourth
                                  tick after a sync clears datacd and reopens the UW
                                  search for the next burst.  The reference's timer
                                  slot runs from the event loop, between two
                                  writeData calls, and a burst channel's output
                                  depends on message boundaries anyway, so the tick
                                  of sample 48000 k - 1 (counted from the channel's
                                  open) fires at the end of the message (one
                                  aero_push_pcm* call) that holds that sample: after
                                  every soft-bit group that message delivered to
                                  AeroL::Decode, before the first of the next
                                  message.  A message that completes several
                                  seconds carries as many ticks.  Where in real time
                                  the shipped binary's timer fires is not pinned;
                                  this placement is, bit for bit, against the oracle
                                  with the timer slot called there
                                  (tests/oracle_tick.py).  Burst MSK does not gate
                                  its sync on datacd: there only the DataCarrierDetect
                                  changes differ */
#define AERO_F_DCD_TICK_CONT 0x100 /* continuous 600/1200-bps MSK (any rate in
                                  [12000, 96000] Hz) and the 8400-bps C channel: run
                                  the same timer on the sample clock.  A channel
                                  counts the samples until its next tick, starting
                                  at the rate Fs it was opened at; the tick fires
                                  after the sample that takes the count to 0 (after
                                  everything that sample delivered to AeroL, before
                                  anything the next one delivers) and the count
                                  restarts at the current Fs.  An MSK rate change
                                  Fs_old -> Fs_new rescales the elapsed part of the
                                  second: left = Fs_new - ((Fs_old - left) * Fs_new)
                                  / Fs_old in integers; AeroL's countdown, datacd and
                                  the edge count carry over.  Neither framing reads
                                  datacd, so every decoded output is the same with
                                  and without the flag; only dcd_edges of
                                  aero_channel_get_events differs: it can fall, which
                                  is how a host sees a C call end or an MSK carrier
                                  go (without the flag it rises once and stays).  As
                                  in the reference, a steady MSK carrier's DCD flaps
                                  under the timer.  OQPSK and burst channels ignore
                                  the flag */
#define AERO_F_EBNO 0x200      /* continuous OQPSK and the C channel: compute the
                                  reference's Eb/N0 estimate (OQPSKEbNoMeasure,
                                  decode/DSP.cpp:691-722, fed once per sample from
                                  OqpskDemodulator::writeData and emitted once per
                                  coarse hop, decode/oqpskdemodulator.cpp:397-402,
                                  :614) for aero_channel_get_quality, and with
                                  AERO_F_TRACE_HOPS aero_pop_ebno.  One more kernel
                                  after every demod launch of those groups reads
                                  the estimator's 2 s of input back out of the AGC
                                  ring the demodulator keeps anyway; its state is
                                  three doubles and a counter per channel.  No
                                  decoded output changes by one bit.  Without the
                                  flag nothing is allocated or launched.  The state
                                  is part of a channel's blob: the layout
                                  fingerprint of an OQPSK or C channel differs with
                                  the flag (and, with it, with AERO_F_TRACE_HOPS,
                                  which adds the record ring), so such a blob moves
                                  only between engines that agree on it
                                  (aero_channel_import: AERO_E_INVALID otherwise).
                                  Continuous MSK and burst channels ignore the
                                  flag (aero_channel_quality says why) */
#define AERO_F_EBNO_MSK 0x400  /* continuous 600/1200-bps MSK at any rate in
                                  [12000, 96000] Hz (the compiled 12 / 24 / 48 kHz
                                  groups, the generic-rate groups, both kernel
                                  shapes): compute the reference's Eb/N0 estimate
                                  (MSKEbNoMeasure, decode/DSP.cpp:482-503, fed
                                  dabval once per sample and emitted once per
                                  coarse hop, decode/mskdemodulator.cpp:305-309,
                                  :461) for aero_channel_get_quality, and with
                                  AERO_F_TRACE_HOPS aero_pop_ebno.  The estimator
                                  averages 2 s and the MSK AGC ring holds 1 s, so
                                  each channel keeps a ring of its own of 2 Fs
                                  doubles: 16 Fs bytes per channel slot of the
                                  group (192 KB at 12 kHz, 1.5 MB at 96 kHz; a
                                  full 65536-channel 12 kHz group 12.6 GB), in
                                  aero_stat("device_bytes").  One more kernel runs
                                  after every demod launch of those groups.  No
                                  MSK demod kernel and no decoded output changes.
                                  A rate change starts a fresh estimator, as the
                                  reference's setSettings constructs one
                                  (:138-140).  Without the flag nothing is
                                  allocated or launched, and layouts and blobs
                                  are what they were.  The flag is one of a
                                  blob's decode-shaping flags: a blob moves only
                                  between engines that agree on it
                                  (aero_channel_import: AERO_E_INVALID otherwise).
                                  OQPSK, C and burst channels ignore it;
                                  AERO_F_EBNO alone still leaves MSK without an
                                  estimate */

typedef struct aero_engine aero_engine;

typedef struct {
  int device;       /* HIP device ordinal                                   */
  int max_channels; /* channel table size (memory is sized for this)        */
  int flags;        /* AERO_F_*                                              */
} aero_engine_cfg;

typedef struct {
  int bitrate;            /* 10500 (OQPSK), 600 or 1200 (MSK); decode/decode.h:42;
                             8400: the C channel (OqpskDemodulator at fb = 8400 +
                             AeroL::DecodeC, decode/aerol.cpp:2145-2415), outside
                             aero-decode's validBitRates; continuous only, fs 48000 */
  int burst;              /* 1: aero-decode --burst: 10500 bps OQPSK, or
                             600 / 1200 bps MSK (one fb = 1200 demodulator at
                             48 kHz, decode/decode.cpp:123-132)               */
  uint32_t fs;            /* 48000 / 12000 / 24000 for 10500 / 600 / 1200 bps
                             (decode/decode.cpp:145, 152-159); burst MSK takes
                             any rate, the audio is demodulated as 48 kHz
                             (burstmskdemodulator.cpp:708-714 only logs it)   */
  int disable_reassembly; /* 1: items are ACARSfragmentsignal (decode.cpp:233) */
} aero_channel_cfg;

/* ACARSItem (decode/aerol.h:163-197) as a fixed-size POD.  `parsed`
 * (libacars, absent) and the wall-clock time are not produced. */
typedef struct {
  uint32_t aesid;
  uint8_t gesid, qno, refno, seqno;
  uint8_t mode, tak, bi, nonacars;
  uint8_t downlink, valid, hastext, moretocome;
  uint8_t fragment; /* 1 = ACARSfragmentsignal, 0 = ACARSsignal */
  uint8_t label_len, reg_len, pad0;
  char label[4];
  char reg[16];
  uint32_t msg_len;  /* bytes used in msg */
  char msg[3584];    /* Latin-1 text, not NUL-terminated */
} aero_acars_item;

/* Engine lifetime (replaces Decoder::Decoder / ~Decoder, decode/decode.cpp:72-260). */
int aero_engine_create(const aero_engine_cfg *cfg, aero_engine **out);
void aero_engine_destroy(aero_engine *e);

/* Opens one VFO channel: the Decoder ctor's demod + AeroL + hunter wiring
 * (decode/decode.cpp:117-241) for one -t topic.  bitrate 10500 at fs 48000,
 * or 600 / 1200 (MSK) at any fs in [12000, 96000] Hz: 12000, 24000 and
 * 48000 run kernels compiled for the rate, other rates the generic-rate MSK
 * kernels.  AERO_E_INVALID for another bit rate or OQPSK rate, AERO_E_RATE
 * for an MSK rate outside that range. */
int aero_channel_open(aero_engine *e, const aero_channel_cfg *cfg, int *ch_out);

/* Closes one channel: ~Decoder for one topic (decode/decode.cpp:243-260).
 * The channel's group finishes its queued GPU passes and host frame work
 * first.  Samples pushed to ch and not yet consumed by a run are dropped, and
 * so is every output not yet popped (items, also those waiting in
 * aero_pop_items_all, soft bits, hops, pt, blocks, frames, R/T tests and
 * packets, C units, voice): a host that wants the channel's tail calls
 * aero_flush and pops before it closes.  Other channels' outputs do not
 * change by one bit, wherever the close falls between their runs.
 *
 * Until the id is given out again, every call that takes ch returns
 * AERO_E_INVALID (a second close too, and aero_trace_select or
 * aero_chan_feed with ch in their lists, which then do nothing).
 * aero_channel_open returns the smallest free id, and takes the smallest
 * free slot of the kind's group; the reopened channel starts as the first
 * channel of a new engine does (hop indices, DCD edges and event counters
 * count from its first sample).  The slot's device state is reset by one
 * kernel launch for every slot closed since the group last ran, at the
 * group's next push or run (or per-channel query: aero_channel_stat and
 * aero_channel_get_events read device state).  A generic-rate MSK group is
 * released when its last channel leaves. */
int aero_channel_close(aero_engine *e, int ch);

/* Snapshot of n channels' decoder state as n self-delimiting blobs written
 * back to back (ch[i]'s blob is the i-th).  dst == NULL: *bytes = the size
 * needed, nothing else happens to dst.  cap too small: AERO_E_FULL, nothing
 * written (*bytes is still the size needed).  A closed or out-of-range id:
 * AERO_E_INVALID.
 *
 * An export is a snapshot, not a close: the channel stays open and carries on
 * exactly as if nothing had happened, and no channel's output changes by one
 * bit.  A move is export, the caller's pops, aero_channel_close, and
 * aero_channel_import on the other engine (another GPU, another process, a
 * later run of the program: a blob may be kept in a file).
 *
 * What travels is everything that decides the channel's future output: every
 * byte its slot owns in the group's device pool (AGC ring, loops, coarse
 * history, AFC / hunter, AeroL framing and DCD, the PCM ring with the samples
 * pushed and not yet demodulated: a partial hop, a C-channel message not yet
 * prefiltered, a burst message pushed since the last run), the host counters
 * (so hop sample indices, soft-bit positions, dcd_edges and hunter_steps
 * continue their numbering), the half-assembled ISUs and ACARS messages, and
 * the channel's aero_channel_cfg.  What does not: outputs produced and not yet
 * popped (items, soft bits, hops, pt, blocks, frames, R/T tests and packets, C
 * units, voice) stay with the source channel.
 *
 * The channels' groups first finish what is queued, as aero_channel_close
 * does: the pending init / reset of slots, their GPU passes and host frame
 * work; host messages queued by aero_push_pcm are moved to the PCM ring.
 * Nothing is demodulated.  One launch of the pack kernel per group and call,
 * however many channels (aero_stat "slot_copies").
 *
 * The blob (little-endian): 8-byte magic "AEROCHB1", u32 version, the
 * channel's cfg as i32 bitrate, i32 burst, u32 fs, i32 disable_reassembly,
 * u32 decode-shaping engine flags, u64 layout fingerprint, u64 total length,
 * u64 length + device section, u64 length + host section.  Only the version
 * that wrote a blob reads it. */
int aero_channel_export(aero_engine *e, const int *ch, int n, void *dst, size_t cap, size_t *bytes);

/* Opens one channel per blob of src (ids and slots as aero_channel_open gives
 * them: the smallest free first) and installs the exported state; ch_out[i] =
 * the id of blob i, *n = the number of blobs.  The channels continue where the
 * exported ones were: pushing the rest of the stream gives, bit for bit, what
 * the uninterrupted channel would have given.  One blob may be imported more
 * than once (each import is its own channel).
 *
 * Admission is aero_channel_open's: AERO_E_FULL when the kind's group or
 * reserved pool has too few free slots for the batch (or cap_ch < blobs); a
 * generic-rate MSK group or the C group is created on first use.
 * AERO_E_INVALID, before anything is opened or written, for a blob whose
 * magic, version or total length is wrong, whose section lengths run past
 * `bytes`, whose kind aero_channel_open refuses, whose layout fingerprint
 * differs from this engine's for the kind (a hash over the kinds, element
 * sizes, rows and fills of the per-channel arrays; not their offsets or the
 * group's size, which may differ), or whose decode-shaping flags differ from
 * the engine's (AERO_F_TRACE_PT, AERO_F_TRACE_BLOCKS, AERO_F_DCD_TICK,
 * AERO_F_DCD_TICK_BURST, AERO_F_DCD_TICK_CONT; the parity traces AERO_F_TRACE_SOFT and AERO_F_TRACE_HOPS are not checked, but
 * continue their numbering only between engines that both keep them).  The
 * fingerprint follows the library's state layout, not only its flags: the
 * build that introduced AERO_F_DCD_TICK_CONT added one per-channel counter to
 * every continuous kind (OQPSK, MSK and C, flag on or off), so blobs that an
 * earlier build exported are refused by it and by later ones, a deliberate
 * format break; burst blobs are not affected.  Every
 * length is checked before it is used.  A batch is all or nothing: on any
 * error no channel of it stays open.
 *
 * The states are written by one launch of the unpack kernel per group and
 * call, ordered on the group's stream after the init or pending reset of the
 * slots they land in; the call returns when it has finished. */
int aero_channel_import(aero_engine *e, const void *src, size_t bytes, int *ch_out, int cap_ch, int *n);

/* Declares that the engine will hold at most n channels of `kind`
 * (bitrate / burst / fs as for aero_channel_open) at once: the kind's group
 * is then created with n slots (rounded up to 64, as max_channels is)
 * instead of max_channels, and the n + 1st open returns AERO_E_FULL until a
 * channel of the kind is closed.  For kinds a large engine holds few of:
 * one C channel costs 2.4 MB of rings per slot of its group.
 * AERO_E_INVALID when the kind's group already exists, n < 1,
 * n > max_channels, or the kind is one aero_channel_open refuses.  A
 * generic-rate MSK group holds at most 256 channels whatever is reserved.
 * Without this call a group has max_channels slots. */
int aero_engine_reserve(aero_engine *e, const aero_channel_cfg *kind, int n);

/* One ZMQ message == one call: Decoder::audioReceived ->
 * OqpskDemodulator::dataReceived / MskDemodulator::dataReceived
 * (decode/decode.cpp:352, decode/oqpskdemodulator.cpp:624-630,
 * decode/mskdemodulator.cpp:472-481).  pcm: int16 LE real samples, copied
 * before returning (a continuous channel's message is staged in pinned host
 * memory and reaches the GPU at the next aero_run).  fs: an OQPSK or burst
 * channel only logs a mismatch; a continuous MSK channel re-applies its
 * settings at any rate in [12000, 96000] Hz, keeping the state
 * MskDemodulator::setSettings keeps (decode/mskdemodulator.cpp:94-218), and
 * refuses a rate outside it (AERO_E_RATE, the message is dropped). */
int aero_push_pcm(aero_engine *e, int ch, const int16_t *pcm, size_t n, uint32_t fs);

/* Lockstep batch push for channels [0, nch): pcm is time-major, n samples
 * per channel, sample t of channel c at pcm[t*ld + c].  dev != 0: pcm is a
 * HIP device pointer (inputs already resident in HBM).  Channels [0, nch)
 * must be of one kind (continuous bit rate, burst OQPSK or burst MSK).  For
 * burst channels the batch is one message per channel (at most 16384
 * samples; burst OQPSK output depends on message boundaries,
 * decode/burstoqpskdemodulator.cpp:264).  The channels must have been opened
 * in order into one group (engine channel j is the group's slot j): once an
 * MSK rate change has moved a channel into a slot another channel left, that
 * group no longer qualifies (AERO_E_INVALID; push per channel instead).
 * Closing and reopening channels of an engine of one kind keeps the
 * condition: the smallest free id gets the smallest free slot (the reopened
 * channels restart at sample 0, so a continuous batch is lockstep again only
 * once every channel of it has been reopened). */
int aero_push_pcm_batch(aero_engine *e, const int16_t *pcm, size_t n, size_t ld, int nch, int dev);

/* aero_push_pcm with pcm a HIP device pointer (e.g. channeliser audio already
 * in HBM, aero_chan.h); the samples are copied before returning. */
int aero_push_pcm_dev(aero_engine *e, int ch, const int16_t *pcm, size_t n, uint32_t fs);

/* Runs the batched kernels for every channel over all pushed samples that
 * complete a coarse-estimate hop; aero_flush also processes the tail. */
int aero_run(aero_engine *e);
int aero_flush(aero_engine *e);

/* Soft bits delivered to AeroL (groups of 32 for OQPSK, 12 for MSK, 0..255;
 * decode/oqpskdemodulator.cpp:534-540, decode/mskdemodulator.cpp:404-407).
 * Needs AERO_F_TRACE_SOFT. */
int aero_pop_softbits(aero_engine *e, int ch, int16_t *dst, size_t cap, size_t *n);

/* ACARSItems emitted on ACARSsignal (or ACARSfragmentsignal with
 * disable_reassembly), in emission order (decode/aerol.cpp:457,522,2127,2142). */
int aero_pop_items(aero_engine *e, int ch, aero_acars_item *dst, size_t cap, size_t *n);

/* Items of every channel in one call (channel order, then emission order);
 * ch[i] receives item i's channel.  For hosts that serve many VFOs from one
 * engine: one call per aero_run instead of one per channel.  Only the first
 * msg_len bytes of each msg are written.
 *
 * aero_run is asynchronous: it enqueues the GPU work and returns.  The pop
 * calls return what has completed so far (in order); aero_flush and
 * aero_sync return only when every pushed sample's outputs are available. */
int aero_pop_items_all(aero_engine *e, aero_acars_item *dst, int *ch, size_t cap, size_t *n);

/* Diagnostics used by the parity tests and the bench.
 * hops: 6 doubles per coarse hop (sample index, estimate, mixer2 Hz,
 * mixer_center Hz, mse, signal). pt: 2 doubles per carrier event.
 * blocks: uint32 count + decoded bits (bytes 0/1) per Viterbi block.
 * frames: 320 bytes per completed frame (312 infofield, u32 len, u32 crc mask);
 * needs AERO_F_TRACE_FRAMES. */
int aero_pop_hops(aero_engine *e, int ch, double *dst, size_t cap_records, size_t *n);
/* Limits the trace collection of continuous channels (soft bits, hops, pt,
 * blocks, frames) to the n channels in ch (n = 0: every channel again), so
 * a parity test can sample a few channels of a full-size batch.  Test
 * support; no reference counterpart. */
int aero_trace_select(aero_engine *e, const int *ch, int n);
int aero_pop_pt(aero_engine *e, int ch, double *dst, size_t cap_records, size_t *n);
int aero_pop_blocks(aero_engine *e, int ch, uint8_t *dst, size_t cap, size_t *n);
int aero_pop_frames(aero_engine *e, int ch, uint8_t *dst, size_t cap, size_t *n);
/* Burst channels (AERO_F_TRACE_FRAMES): every R/T test (uint32 blockptr,
 * uint32 RTChannelDeleaveFECScram result) and every decoded R/T packet
 * (uint32 'R'/'T', uint32 length, the infofield bytes), in order
 * (decode/aerol.h:755-836). */
int aero_pop_rt_tests(aero_engine *e, int ch, uint8_t *dst, size_t cap, size_t *n);

/* C channel (bitrate 8400).  A C-channel message is one prefilter block
 * (decode/oqpskdemodulator.cpp:292-324, output depends on message boundaries):
 * at most 32768 samples per aero_push_pcm (AERO_E_INVALID above).
 * c_units: the 12-byte SUs AeroL::DecodeC emits on Call_progress_Signal
 * (CRC-valid, message 0x30, decode/aerol.cpp:2329-2346), cap / *n in SUs.
 * voice: per decoded frame (Voicesignal, :2394-2402) a 304-byte record: uint32
 * LE AES of the frame's last Call_progress SU (0 = "000000"), then the 300
 * voice bytes (25 frames of 12); cap / *n in records.  Frames (36 SU bytes,
 * CRC mask of the 3 SUs) through aero_pop_frames with AERO_F_TRACE_FRAMES. */
int aero_pop_c_units(aero_engine *e, int ch, uint8_t *dst, size_t cap, size_t *n);
int aero_pop_voice(aero_engine *e, int ch, uint8_t *dst, size_t cap, size_t *n);
int aero_pop_rt_packets(aero_engine *e, int ch, uint8_t *dst, size_t cap, size_t *n);

/* Timing (AERO_F_TIMING): kernel names {"demod","coarse","frame","viterbi"},
 * and with AERO_F_EBNO / AERO_F_EBNO_MSK "ebno" (prefixed "c8400_" for the C
 * group and "msk600_", "msk600_18750_", ... for an MSK group, as the others),
 * give summed device milliseconds (HIP events) and launch counts; host
 * sections {"host_push","host_run","host_wait_njobs","host_wait_jobs",
 * "host_frames"} give summed wall milliseconds and entry counts.  Both since
 * the last reset. */
int aero_timing(aero_engine *e, const char *name, double *ms, long *launches);
void aero_timing_reset(aero_engine *e);

/* Counters since creation.  "device_bytes" / "groups": the device pools of
 * the continuous channel groups that exist now and their number (a
 * generic-rate MSK group holds at most 256 channels and is released when its
 * last channel moves to another rate).  Continuous channels: "viterbi_jobs" (blocks
 * the GPU Viterbi decoded and handed back), "frames" (frames delivered to
 * the SU/ACARS host), "su_crc_ok" (SUs whose CRC-16 checked); burst
 * channels: "rt_tests" (RTChannelDeleaveFECScram decodes run),
 * "rt_packets" (R/T packets that passed their CRCs), "rt_pass_max" (the most
 * R/T tests one pass handed to the host; from 256 on they are split over the
 * host threads); "slot_copies": launches of the kernels that pack and unpack
 * exported / imported slots; "slot_resets": launches of the kernel that resets closed
 * channels' slots (one per group for all the slots closed since the group
 * last pushed or ran); "ebno_launches": launches of the Eb/N0 kernel (0
 * without AERO_F_EBNO and AERO_F_EBNO_MSK).  Joins the
 * asynchronous host frame work first.  AERO_E_INVALID for another name. */
int aero_stat(aero_engine *e, const char *name, uint64_t *value);

/* Per-channel state: "hunter_scans" (full SignalHunter scans without a
 * signal, decode/hunter.cpp:31-37 -- aero-decode's --no-signal-exit),
 * "freq_center" (the mixer centre in Hz after the last coarse hop).  Waits
 * for the channel's queued GPU work. */
int aero_channel_stat(aero_engine *e, int ch, const char *name, int64_t *value);

/* Decoder status events of one channel since it opened, for aero-decode's
 * verbose log (Decoder::handleDcdChange / handleNewFreqCenter,
 * decode/decode.cpp:429-439).  dcd_edges: changes of AeroL's data carrier
 * detect as SignalHunter::handleDcd passes them on (decode/hunter.cpp:14-19);
 * they alternate and the first is "no signal => signal".  hunter_steps:
 * SignalHunter::newFreqCenter emissions (decode/hunter.cpp:31-40), with the
 * centre of step k (1-based) in hunter_fc[(k - 1) & 7] for the last eight
 * steps (0 for burst channels: their hunter is disabled, decode/decode.cpp:175).
 * Waits for the channel's queued GPU work. */
typedef struct {
  int64_t dcd_edges;
  int64_t hunter_steps;
  double hunter_fc[8];
} aero_channel_events;
int aero_channel_get_events(aero_engine *e, int ch, aero_channel_events *out);

/* Signal quality of one continuous channel, for a host that ranks many VFOs
 * of one engine (which of the opened channels hold a usable carrier, how good
 * it is, when it degrades).  Waits for the channel's queued GPU work, as
 * aero_channel_stat does.
 *   samples    input samples demodulated since the channel opened
 *   mse        the demodulator's mean squared error after `samples` samples
 *              (what FreqOffsetEstimateSlot tests, oqpskdemodulator.cpp:562-620,
 *              mskdemodulator.cpp:430-469)
 *   mixer_hz   mixer2's frequency; center_hz the mixer centre
 *   signal     1 when mse is not above the kind's threshold (0.65 for OQPSK
 *              and C, 0.5 for MSK): what the hunter takes for "got a signal"
 *   ebno_db    with AERO_F_EBNO on a continuous OQPSK or C channel
 *              (ebno_valid = 1): OQPSKEbNoMeasure::EbNo after `samples`
 *              samples, 0 .. 50 dB in the reference's own calibration.  The
 *              reference never initialises EbNo; here it starts at 0.0 and
 *              the 0.8 / 0.2 smoothing forgets the start within a few samples.
 *              With AERO_F_EBNO_MSK on a continuous MSK channel
 *              (ebno_valid = 1): MSKEbNoMeasure::EbNo after `samples`
 *              samples, of the estimator constructed at the channel's last
 *              rate change (`samples` itself counts from the channel's first
 *              sample).  Range (-inf, 50] dB: the reference has no lower
 *              clamp, so the value is negative during the first 2 s while
 *              the window fills, and a sample whose log argument is +inf
 *              leaves it at -inf until the next rate change.  It starts at
 *              0.0 at open and after every rate change.
 *              Otherwise ebno_valid = 0 and ebno_db = 0
 * After a plain aero_run a channel stands on its last hop's boundary:
 * samples, mse, mixer_hz, center_hz and signal then equal fields 0, 4, 2, 3
 * and 5 of the last aero_pop_hops record bit for bit, and ebno_db is the value
 * the reference emits with that hop (EbNoMeasurmentSignal).
 *
 * Continuous MSK has its estimate under a flag of its own because of what it
 * costs: MSKEbNoMeasure averages 2 s while the MSK AGC ring holds 1 s, so each
 * channel keeps a ring of 2 Fs doubles (up to 192000) for it; AERO_F_EBNO alone
 * leaves ebno_valid = 0 there.  Burst channels compute their EbNo inside the
 * burst demodulators, only while a burst is demodulated and from a value no
 * ring keeps (per burst, another schedule): AERO_E_INVALID, as for a closed or
 * out-of-range id. */
typedef struct {
  int64_t samples;
  double ebno_db, mse, mixer_hz, center_hz;
  int32_t signal, ebno_valid;
} aero_channel_quality;
int aero_channel_get_quality(aero_engine *e, int ch, aero_channel_quality *out);

/* AERO_F_EBNO (OQPSK, C) or AERO_F_EBNO_MSK (continuous MSK) with
 * AERO_F_TRACE_HOPS (parity tests): 2 doubles per record,
 * (sample index, EbNo), in order; one record whenever a demod launch leaves
 * the channel on a coarse-hop boundary, so every hop record popped so far has
 * a record with its sample index (field 0, which counts across an MSK rate
 * change as the hop records do), and a flush that ends exactly on a
 * boundary may leave one more.  Records not yet popped follow an MSK channel
 * to its new rate's group.  AERO_E_INVALID without both flags of the
 * channel's kind, and for burst channels. */
int aero_pop_ebno(aero_engine *e, int ch, double *dst, size_t cap_records, size_t *n);

/* Total input samples demodulated across channels since creation. */
uint64_t aero_samples_processed(aero_engine *e);

/* Synchronise the engine's stream. */
int aero_sync(aero_engine *e);

/* Evaluates the device libm on n inputs (parity test of aero_math.h):
 * fn 0 hypot, 1 atan2, 2 tanh, 3 sin, 4 cos, 5 log10, 6 sqrt, 7 fmod(x,360),
 * 8 division x/y, ..., 21 log10 of x >= 1 (aero_engine.py MATH_FN has the
 * whole list).  x, y, out are host arrays. */
int aero_device_math(aero_engine *e, int fn, const double *x, const double *y, double *out, size_t n);

/* Diagnostic, like aero_device_math: runs one of the device's K=7 soft
 * Viterbi decoders on ncw codewords of nsoft soft values each (parity test
 * against the oracle on input no stream produces).  bits takes nsoft / 2
 * bytes (0 / 1) per codeword: the nsoft / 2 - 6 decoded bits, then zeros.
 * in, bits and overlap are host arrays; ncw <= 65536.
 *
 * Flat variants: `in` is ncw x nsoft soft values in decoding order, nsoft
 * even, 24 <= nsoft <= 6080; overlap is not used.
 *   AERO_VIT_WAVE        history in LDS
 *   AERO_VIT_REGS        history in registers (the R/T tests' decoder)
 *   AERO_VIT_REGS2_SELF  the two-codeword decoder given one codeword twice
 *                        (a continuous job without a partner)
 *   AERO_VIT_REGS2_PAIR  codewords 2k and 2k + 1 in one wave
 * Production-source variants: the two-codeword decoder reads its stream as
 * the continuous channels' kernels do.  `in` is ncw records of BLK + 64
 * bytes: the raw block as the framing kernel stores it (BLK bytes: a 64-row
 * interleaver block row by row, or the C channel's depunctured frame), the 62
 * soft values the previous block's decode left as overlap, one byte `first`
 * (1: the stream's first block, the overlap is not read), one pad byte.  The
 * decoded stream is the overlap (unless first), the deinterleaved block
 * (position 64 j + l from row (27 l) mod 64, column j; for C the frame with
 * erasures at 4 k + 3) and 24 erasures, so nsoft = BLK + 24 (first) or
 * BLK + 86 and every record's `first` agrees with it.  overlap takes the 62
 * values per record the source hands to the next block.  Blocks 2k and
 * 2k + 1 share a wave, as two channels' jobs do; C frames decode alone.
 *   AERO_VIT_BLOCK4992 (OQPSK), AERO_VIT_BLOCK384 (MSK 600),
 *   AERO_VIT_BLOCK576 (MSK 1200), AERO_VIT_CSOFT (BLK = 5460) */
#define AERO_VIT_WAVE 0
#define AERO_VIT_REGS 1
#define AERO_VIT_REGS2_SELF 2
#define AERO_VIT_REGS2_PAIR 3
#define AERO_VIT_BLOCK4992 4
#define AERO_VIT_BLOCK384 5
#define AERO_VIT_BLOCK576 6
#define AERO_VIT_CSOFT 7
int aero_device_viterbi(aero_engine *e, int variant, const uint8_t *in, size_t ncw, size_t nsoft, uint8_t *bits,
                        uint8_t *overlap);

/* Diagnostic, like aero_device_viterbi: runs a device FFT on nrec records of
 * 2^log2n complex doubles (re, im pairs, natural order; host arrays) and
 * returns each record's transform in natural order, one workgroup per record
 * as in production, with tables built by the functions the channel groups
 * use.  nrec <= 256.
 *   AERO_FFT_DIT    fft_dit: log2n 12 or 13 (inverse 0 or 1) or 14 (inverse
 *                   0).  The inverse is the plain sum, without JFFT's 1/N.
 *                   depth, start and stop are not looked at.
 *   AERO_FFT_CHAIN  the coarse estimator's chained transforms, log2n 13 or
 *                   14, inverse 0: depth 1 the forward transform; depth 2
 *                   then bins start..stop zeroed (none if start > stop) and
 *                   the inverse (without 1/N); depth 3 then every value
 *                   squared and the forward transform again.
 * AERO_E_INVALID for anything else, before anything is launched. */
#define AERO_FFT_DIT 0
#define AERO_FFT_CHAIN 1
int aero_device_fft(aero_engine *e, int kind, int log2n, int inverse, int depth, int start, int stop,
                    const double *in, size_t nrec, double *out);

/* Diagnostic: the coarse estimator's smoothed spectrum y of a continuous
 * channel (CoarseFreqEstimate::y, decode/coarsefreqestimate.cpp) as its next
 * hop will read it: the bins the engine keeps, *first_bin .. *first_bin + *n
 * - 1 of the nfft, into dst (cap doubles; AERO_E_INVALID if too few).  After
 * a bigchange() the kernel has not applied yet, 20.0 for every bin.  Waits
 * for the channel's queued GPU work.  AERO_E_INVALID for a burst channel. */
int aero_channel_coarse_y(aero_engine *e, int ch, double *dst, size_t cap, size_t *n, int *first_bin);

const char *aero_strerror(int rc);

#ifdef __cplusplus
}
#endif
#endif
