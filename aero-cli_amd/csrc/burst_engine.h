// burst_engine.h — the burst-mode group's entry points for engine.hip
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/aero_engine.h"

namespace aero {

struct BurstGroup;
class HostPool;
enum BurstKind { BURST_OQPSK = 0, BURST_MSK = 1 };  // 10500 OQPSK / 600-1200 MSK (both bit rates in one group)
int burst_group_create(int device, int flags, int max_channels, int kind, BurstGroup **out);
void burst_group_destroy(BurstGroup *g);
int burst_open(BurstGroup *g, int bitrate, bool disable_reassembly, int *local);
// closes local channel c: its pending samples and undelivered outputs are
// dropped, its slot is reset (one kernel launch for every slot closed or
// reopened since, at the group's next push or run) and reused by burst_open,
// the smallest free slot first
int burst_close(BurstGroup *g, int c);
struct LayoutRec;
size_t burst_layout_plan(int kind, int C, LayoutRec *rec);  // slot_reset.h: the pool's arrays; returns the pool size
int burst_push(BurstGroup *g, int c, const int16_t *pcm, size_t n, bool dev, bool msg_start, bool msg_end);
int burst_push_batch(BurstGroup *g, const int16_t *src, size_t n, size_t ld, int nch, bool dev);
int burst_run(BurstGroup *g, int flush);
int burst_sync(BurstGroup *g);
int burst_pop_soft(BurstGroup *g, int c, int16_t *dst, size_t cap, size_t *n);
int burst_pop_hops(BurstGroup *g, int c, double *dst, size_t cap_records, size_t *n);
int burst_pop_tests(BurstGroup *g, int c, uint8_t *dst, size_t cap, size_t *n);
int burst_pop_packets(BurstGroup *g, int c, uint8_t *dst, size_t cap, size_t *n);
std::vector<aero_acars_item> &burst_items(BurstGroup *g, int c);
uint64_t burst_processed(const BurstGroup *g);
uint64_t burst_stat(const BurstGroup *g, int which);  // 0: R/T tests run, 1: R/T packets decoded, 2: most tests of one pass, 3: reset-kernel launches, 4: pack / unpack launches
// aero_channel_export / aero_channel_import (chan_blob.h, slot_copy.h)
struct BurstHost;
void burst_blob_plan(int kind, uint64_t *fingerprint, size_t *dev_bytes);  // of a kind's packed slot (no GPU)
bool burst_is_open(const BurstGroup *g, int c);
int burst_slots_left(const BurstGroup *g);  // opens until AERO_E_FULL
int burst_export_begin(BurstGroup *g);      // pending init and resets done, the stream idle
void burst_export_host(const BurstGroup *g, int c, std::string &out);  // the host section of channel c
bool burst_host_fits(const BurstHost &h);   // its counters are ones a push or run can continue from
int burst_pack(BurstGroup *g, const int *slots, int n, uint8_t *dst);  // sorted slots -> n packed slots (one launch)
int burst_unpack(BurstGroup *g, const int *slots, int n, const uint8_t *src);  // and back, after the slots' init / reset
void burst_import_host(BurstGroup *g, int c, BurstHost &h);  // installs (and takes) the parsed host section
int burst_dcd_edges(BurstGroup *g, int c, int64_t *edges);  // AeroL datacd changes (waits for the group's work)
void burst_timing(BurstGroup *g, const char *name, double *ms, long *launches);  // adds to *ms / *launches
void burst_timing_reset(BurstGroup *g);
void burst_group_set_pool(BurstGroup *g, HostPool *pool);  // host threads for the R/T tests (the engine's)

}  // namespace aero
