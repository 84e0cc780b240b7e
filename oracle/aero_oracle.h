/*
 * aero_oracle.h — TEST INFRASTRUCTURE ONLY.
 *
 * C API of the CPU restatement of airframesio/aero-cli's continuous
 * 10500-bps OQPSK decode path (decode/oqpskdemodulator.cpp, decode/DSP.cpp,
 * decode/coarsefreqestimate.cpp, decode/jfft.cpp, decode/hunter.cpp,
 * decode/aerol.cpp, decode/jconvolutionalcodec.cpp + libcorrect).
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library, and only as the checker.  Nothing in the product path
 * links or calls it.
 *
 * Parity status: see oracle/aero_oracle.cpp header.
 */
#ifndef AERO_ORACLE_H
#define AERO_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct oracle_chan oracle_chan;

/* flags */
#define ORACLE_TRACE_PT 1 /* record every rotated pt_qpsk (re,im) */
#define ORACLE_BURST 2    /* burst mode (aero-decode --burst): 10500 OQPSK, 600/1200 MSK */
#define ORACLE_DCD_TICK 4 /* continuous OQPSK: AeroL's 1 s DCD timer (aerol.cpp:900-902,
                             1043-1058) fires after every Fs input samples */

/* bitrate 10500 / 8400 (continuous OQPSK P / C channel), 600 / 1200 (MSK) */
oracle_chan *oracle_create(int bitrate, int flags);
void oracle_destroy(oracle_chan *c);

/* One call == one ZMQ message == OqpskDemodulator::dataReceived
 * (decode/oqpskdemodulator.cpp:624-630). */
int oracle_push(oracle_chan *c, const int16_t *pcm, size_t n);
/* the same with the message's sample rate (Decoder::audioReceived): an MSK
 * channel re-applies its settings at a new rate (mskdemodulator.cpp:473-481) */
int oracle_push_rate(oracle_chan *c, const int16_t *pcm, size_t n, int fs);

/* Soft bits delivered to AeroL (groups of 32, decode/oqpskdemodulator.cpp:534-540). */
size_t oracle_softbits(const oracle_chan *c, uint8_t *dst, size_t cap);
/* burst: delivered soft bits including the -1 start-of-packet markers */
size_t oracle_softbits16(const oracle_chan *c, int16_t *dst, size_t cap);
/* burst: every R/T test (uint32 blockptr, uint32 result code) in order */
size_t oracle_rt_tests(const oracle_chan *c, uint8_t *dst, size_t cap);
/* burst: per decoded R/T packet: uint32 kind ('R'/'T'), uint32 length, infofield bytes */
size_t oracle_rt_packets(const oracle_chan *c, uint8_t *dst, size_t cap);

/* C channel (bitrate 8400, AeroL::DecodeC, decode/aerol.cpp:2145-2415): every
 * CRC-valid Call_progress SU (Call_progress_Signal, 12 bytes each), and per
 * decoded frame a uint32 AES (of the frame's last Call_progress, 0 for
 * "000000") followed by the 300 voice bytes (Voicesignal). */
size_t oracle_c_units(const oracle_chan *c, uint8_t *dst, size_t cap);
size_t oracle_voice(const oracle_chan *c, uint8_t *dst, size_t cap);

/* Per coarse-estimate hop, 6 doubles: sample index, freq_offset_est emitted,
 * mixer2 freq, mixer_center freq (after the slot ran), mse, signal flag. */
size_t oracle_hops(const oracle_chan *c, double *dst, size_t cap_records);

/* Continuous channels: CoarseFreqEstimate's smoothed spectrum y (all nfft
 * values, fftshifted bin order), and |out[i]| of the last process() after its
 * fftshift (the argument of its log10; before the first hop all zero).  Both
 * return nfft and copy at most cap values. */
size_t oracle_coarse_y(const oracle_chan *c, double *dst, size_t cap);
size_t oracle_coarse_absx(const oracle_chan *c, double *dst, size_t cap);

/* Decoder status events (decode/decode.cpp:429-439): *dcd_edges = the data
 * carrier detect changes SignalHunter::handleDcd passes on; returns the
 * number of newFreqCenter emissions and copies their centres (at most cap). */
size_t oracle_events(oracle_chan *c, long long *dcd_edges, double *fc, size_t cap);

/* rotated pt_qpsk trace (2 doubles per carrier event), only with ORACLE_TRACE_PT */
size_t oracle_pt(const oracle_chan *c, double *dst, size_t cap_records);

/* Per decoded P-channel block: 2496 (or 2483 first) decoded bits as bytes 0/1,
 * prefixed by a uint32 count. */
size_t oracle_blocks(const oracle_chan *c, uint8_t *dst, size_t cap);

/* Per completed frame: 320 bytes = up to 312 infofield bytes (zero padded),
 * then uint32 infofield length, then uint32 crc-ok bitmask (26 bits). */
size_t oracle_frames(const oracle_chan *c, uint8_t *dst, size_t cap);

/* Link-layer trace of AeroL::Decode (continuous P channels): per event four
 * long long: kind (1 UW sync, 2 frame-length wrap without a UW, 3 block handed
 * to the decoder, 4 frame done, 5 DCD tick, 6 isudata.reset()), soft bits taken
 * so far, cntr before the event, datacdcountdown after it.  For the CPU tests
 * to prove what a stream reaches; nothing of it is compared with the GPU. */
size_t oracle_link_trace(oracle_chan *c, long long *dst, size_t cap_records);

/* Past the modem: the end-of-frame SU loop on caller bytes (a frame record
 * and items come out as from a decoded frame), the R/T branch on a caller's
 * packet (kind 'R' / 'T'; -1: shorter than the reference can produce), and
 * isudata.reset(). */
int oracle_feed_frame(oracle_chan *c, const uint8_t *info, int len, int formatid);
int oracle_feed_rt_packet(oracle_chan *c, int kind, const uint8_t *info, int len, int nsus);
void oracle_feed_isu_reset(oracle_chan *c);

/* How often each return of ISUData::update, ParserISU::parse,
 * ACARSDefragmenter::defragment and RISUData::update and each branch of the
 * end-of-frame SU dispatch was taken (the order of tests/aero_testlib.py
 * BRANCHES); returns their number.  For a test to show that its inputs reach
 * them all. */
size_t oracle_branch_hits(const oracle_chan *c, long long *dst, size_t cap);

/* ACARSItems as canonical text lines (see tests/aero_items.py). */
size_t oracle_items(const oracle_chan *c, char *dst, size_t cap);

/* libcorrect-ABI restatement (r=1/2, K=7, polys {109,79}). */
size_t oracle_conv_encode(const uint8_t *msg, size_t msg_len, uint8_t *encoded);
size_t oracle_viterbi_decode_soft(const uint8_t *soft, size_t num_encoded_bits,
                                  uint8_t *msg);
/* The same decoder with one rule broken (test infrastructure: shows that a
 * test's inputs reach the rule).  mut 0: none; 1: ACS ties keep the
 * predecessor whose dropped bit is 1; 2: least-metric ties go to the highest
 * index; 3: no renormalisation subtract; 4: the windowed traceback starts
 * from state 0; 5: the least-metric search is not restricted in the tail. */
size_t oracle_viterbi_decode_soft_mut(const uint8_t *soft, size_t num_encoded_bits,
                                      uint8_t *msg, int mut);

/* Known-answer helpers */
uint16_t oracle_crc16_bytes(const uint8_t *bytes, int n);
void oracle_scrambler_bits(int *dst, int n);
void oracle_deinterleave_perm(int N, int *src_index_of_dst);
void oracle_rrc_design(double alpha, int firsize, double fs, double symfreq, double *dst);
void oracle_cis_table(double *dst); /* 19999 x (cos, sin) */
void oracle_twiddles(int nfft, int inverse, double *dst);
void oracle_msk_taps(int sps, double *dst); /* MskDemodulator matched filter, 2*sps taps */

/* raw JFFT-order transform for the FFT parity test (in place, nfft complex) */
void oracle_fft(double *x, int nfft, int inverse);

/* aero-publish channeliser (pub_oracle.cpp).  mains: nmain x {frequency,
 * out_rate, compress_scale, publish}; vfos: nvfo x {frequency, data_rate,
 * out_rate, filter_bandwidth}; gains: the INI "gain" values.  NULL when the
 * configuration is invalid. */
typedef struct oracle_pub oracle_pub;
oracle_pub *oracle_pub_create(int fs, int center, int mix_offset, int dcc, const int *mains, int nmain,
                              const int *vfos, const float *gains, int nvfo);
void oracle_pub_destroy(oracle_pub *o);
int oracle_pub_block_len(const oracle_pub *o);
void oracle_pub_process(oracle_pub *o, const float *iq, int nblocks); /* interleaved CF32 blocks */
size_t oracle_pub_usb(const oracle_pub *o, int v, int16_t *dst, size_t cap);
size_t oracle_pub_iq(const oracle_pub *o, int m, int8_t *dst, size_t cap);
int oracle_pub_info(const oracle_pub *o, int v, int *info7);
int oracle_pub_low_pass(double gain, double fs, double cutoff, double tw, float *dst, int cap);
void oracle_pub_hilbert(int len, int fs, float *dst);
void oracle_pub_osc(double fs, double freq, float *dst); /* (int)fs complex */

#ifdef __cplusplus
}
#endif
#endif
