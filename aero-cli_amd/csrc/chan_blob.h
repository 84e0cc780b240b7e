// chan_blob.h — the channel blob of aero_channel_export / aero_channel_import
// (host only, no HIP): one channel's decoder state as a self-delimiting run of
// bytes.  Little-endian:
//
//   0   8  magic "AEROCHB1"
//   8   4  u32 version (BLOB_VERSION; another version is refused)
//   12  4  i32 bitrate          the channel's aero_channel_cfg
//   16  4  i32 burst
//   20  4  u32 fs
//   24  4  i32 disable_reassembly
//   28  4  u32 flags            the engine's decode-shaping flags (BLOB_FLAGS)
//   32  8  u64 layout fingerprint (slot_copy.h plan_fingerprint)
//   40  8  u64 total length of the blob
//   48  8  u64 D, then D bytes: the device section (slot_copy.h: the packed slot)
//   ..  8  u64 H, then H bytes: the host section (ContHost / BurstHost below)
//
// Blobs may come from a file: BlobReader checks every length against the
// bytes left before it is used, and every count before a loop or allocation.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <vector>

#include "acars_host.h"

namespace aero {

constexpr char BLOB_MAGIC[8] = {'A', 'E', 'R', 'O', 'C', 'H', 'B', '1'};
constexpr uint32_t BLOB_VERSION = 1;
constexpr size_t BLOB_HEADER = 48;
// flags that shape what a channel decodes or what its slot holds
constexpr uint32_t BLOB_FLAGS = AERO_F_TRACE_PT | AERO_F_TRACE_BLOCKS | AERO_F_DCD_TICK | AERO_F_DCD_TICK_BURST |
                                AERO_F_DCD_TICK_CONT | AERO_F_EBNO_MSK;

// appends little-endian fields to a string
struct BlobWriter {
  std::string &s;
  explicit BlobWriter(std::string &out) : s(out) {}
  void u8(uint8_t v) { s.push_back((char)v); }
  void u32(uint32_t v) {
    for (int k = 0; k < 4; k++) s.push_back((char)((v >> (8 * k)) & 0xFF));
  }
  void i32(int32_t v) { u32((uint32_t)v); }
  void u64(uint64_t v) {
    for (int k = 0; k < 8; k++) s.push_back((char)((v >> (8 * k)) & 0xFF));
  }
  void i64(int64_t v) { u64((uint64_t)v); }
  void bytes(const void *p, size_t n) { s.append(static_cast<const char *>(p), n); }
  void str(const std::string &v) {  // u32 length + bytes
    u32((uint32_t)v.size());
    s.append(v);
  }
};

// bounds-checked cursor: a read past the end returns zero and clears ok
struct BlobReader {
  const uint8_t *p;
  size_t n, pos = 0;
  bool ok = true;
  BlobReader(const uint8_t *src, size_t len) : p(src), n(len) {}
  size_t left() const { return n - pos; }
  // the next k bytes (nullptr and !ok when fewer are left)
  const uint8_t *take(size_t k) {
    if (!ok || k > left()) {
      ok = false;
      return nullptr;
    }
    const uint8_t *r = p + pos;
    pos += k;
    return r;
  }
  uint8_t u8() {
    const uint8_t *q = take(1);
    return q ? q[0] : 0;
  }
  uint32_t u32() {
    const uint8_t *q = take(4);
    uint32_t v = 0;
    if (q)
      for (int k = 0; k < 4; k++) v |= (uint32_t)q[k] << (8 * k);
    return v;
  }
  int32_t i32() { return (int32_t)u32(); }
  uint64_t u64() {
    const uint8_t *q = take(8);
    uint64_t v = 0;
    if (q)
      for (int k = 0; k < 8; k++) v |= (uint64_t)q[k] << (8 * k);
    return v;
  }
  int64_t i64() { return (int64_t)u64(); }
  bool str(std::string &out) {  // u32 length + bytes; the length checked before the copy
    const uint32_t len = u32();
    const uint8_t *q = take(len);
    if (!q && len) return false;
    if (!ok) return false;
    out.assign(reinterpret_cast<const char *>(q), len);
    return true;
  }
  // a count of records of at least `min_each` bytes: refused when the bytes left cannot hold them
  bool count(uint32_t &c, size_t min_each) {
    c = u32();
    if (!ok || (size_t)c > left() / (min_each ? min_each : 1)) ok = false;
    return ok;
  }
};

struct BlobHeader {
  aero_channel_cfg cfg{};
  uint32_t flags = 0;
  uint64_t fingerprint = 0, total = 0;
  const uint8_t *dev = nullptr, *host = nullptr;  // into the parsed buffer
  uint64_t dev_len = 0, host_len = 0;
};

inline size_t blob_size(size_t dev_len, size_t host_len) { return BLOB_HEADER + 8 + dev_len + 8 + host_len; }
// writes the header and the two length prefixes and the host section into dst
// (blob_size bytes); returns where the dev_len bytes of the device section go
uint8_t *blob_write(uint8_t *dst, const aero_channel_cfg &cfg, uint32_t flags, uint64_t fingerprint, size_t dev_len,
                    const std::string &host);
// the blob at src (at most `bytes` long): false for a wrong magic, version or
// total length, or a section that runs past the end
bool blob_parse(const uint8_t *src, size_t bytes, BlobHeader &h);

// host mirrors and counters of a continuous channel (engine.hip Group)
struct ContHost {
  int64_t avail = 0, nsamp = 0, hops = 0, hop_base = 0, soft_seen = 0, pre_end = 0;
  int32_t c_cd = 0, c_dcd = 0, c_edges = 0;
  std::deque<long long> msg_end;
  std::vector<uint8_t> infofield;
  std::unique_ptr<PChannelHost> host;  // set by load
  // `live`: the channel's PChannelHost (saved in place of `host`)
  void save(std::string &out, const PChannelHost *live = nullptr) const;
  bool load(const uint8_t *src, size_t n);
};

// host mirrors and counters of a burst channel (burst_engine.hip BurstGroup)
struct BurstHost {
  int64_t avail = 0, chunk_n = 0, hb_base = 0, soft_seen = 0;
  int32_t tsu = 0, tblocks = 0, ok_burst = -1, hops_seen = 0, since_run = 0;
  std::unique_ptr<PChannelHost> host;  // set by load
  // `live`: the channel's PChannelHost (saved in place of `host`)
  void save(std::string &out, const PChannelHost *live = nullptr) const;
  bool load(const uint8_t *src, size_t n);
};

}  // namespace aero
