/*
 * chan_blob.cpp — see chan_blob.h: the blob header, the host sections of a
 * continuous and a burst channel, and PChannelHost::save / load (the ISU /
 * R-ISU reassembly and the ACARS defragmenter's messages in flight).
 */
#include "chan_blob.h"

namespace aero {

namespace {

constexpr uint32_t HOST_TAG_CONT = 0x544E4F43;   // "CONT"
constexpr uint32_t HOST_TAG_BURST = 0x54535242;  // "BRST"
constexpr uint32_t PHOST_TAG = 0x54534850;       // "PHST"
// smallest encodings (bounds a count before its loop)
constexpr size_t ISU_MIN = 4 + 5 + 4 + 4, RISU_MIN = ISU_MIN + 12, ACARS_MIN = ISU_MIN + 3 + 12 + 5,
                 FRAG_MIN = ACARS_MIN + 4;

void put_isu(BlobWriter &w, const IsuItem &v) {
  w.u32(v.aesid);
  w.u8(v.gesid);
  w.u8(v.qno);
  w.u8(v.seqno);
  w.u8(v.refno);
  w.u8(v.nooct);
  w.str(v.userdata);
  w.i32(v.count);
}
bool get_isu(BlobReader &r, IsuItem &v) {
  v.aesid = r.u32();
  v.gesid = r.u8();
  v.qno = r.u8();
  v.seqno = r.u8();
  v.refno = r.u8();
  v.nooct = r.u8();
  if (!r.str(v.userdata)) return false;
  v.count = r.i32();
  return r.ok;
}
template <class R>
void put_risu(BlobWriter &w, const R &v) {
  put_isu(w, v.isu);
  w.i32(v.seqind);
  w.i32(v.sutype);
  w.i32(v.filled);
}
template <class R>
bool get_risu(BlobReader &r, R &v) {
  if (!get_isu(r, v.isu)) return false;
  v.seqind = r.i32();
  v.sutype = r.i32();
  v.filled = r.i32();
  return r.ok;
}
void put_acars(BlobWriter &w, const AcarsItem &v) {
  put_isu(w, v.isu);
  w.u8(v.mode);
  w.u8(v.tak);
  w.u8(v.bi);
  w.str(v.label);
  w.str(v.reg);
  w.str(v.message);
  w.u8(v.nonacars);
  w.u8(v.downlink);
  w.u8(v.valid);
  w.u8(v.hastext);
  w.u8(v.more);
}
bool get_acars(BlobReader &r, AcarsItem &v) {
  if (!get_isu(r, v.isu)) return false;
  v.mode = r.u8();
  v.tak = r.u8();
  v.bi = r.u8();
  if (!r.str(v.label) || !r.str(v.reg) || !r.str(v.message)) return false;
  v.nonacars = r.u8() != 0;
  v.downlink = r.u8() != 0;
  v.valid = r.u8() != 0;
  v.hastext = r.u8() != 0;
  v.more = r.u8() != 0;
  return r.ok;
}

void put_phost(BlobWriter &w, const PChannelHost *h) {
  std::string s;
  if (h) h->save(s);
  w.str(s);
}
// a length-prefixed PChannelHost state, which must fill its length exactly
bool get_phost(BlobReader &r, std::unique_ptr<PChannelHost> &h) {
  const uint32_t len = r.u32();
  const uint8_t *q = r.take(len);
  if (!r.ok || !q) return false;
  h.reset(new PChannelHost(false));
  return h->load(q, len);
}

}  // namespace

void PChannelHost::save(std::string &out) const {
  BlobWriter w(out);
  w.u32(PHOST_TAG);
  w.u8(fragments_only_);
  w.u8(downlink_);
  w.u32((uint32_t)risuitems_.size());
  for (const RIsuItem &v : risuitems_) put_risu(w, v);
  put_risu(w, an_risu_);
  put_isu(w, risu_last_);
  w.u32((uint32_t)isuitems_.size());
  for (const IsuItem &v : isuitems_) put_isu(w, v);
  put_isu(w, an_isu_);
  put_isu(w, lastvalid_);
  put_acars(w, an_);
  w.u32((uint32_t)frags_.size());
  for (const Frag &f : frags_) {
    put_acars(w, f.item);
    w.i32(f.count);
  }
}

bool PChannelHost::load(const uint8_t *src, size_t n) {
  PChannelHost t(fragments_only_);
  auto parse = [&]() -> bool {
    if (!src) return false;
    BlobReader r(src, n);
    if (r.u32() != PHOST_TAG || !r.ok) return false;
    t.fragments_only_ = r.u8() != 0;
    t.downlink_ = r.u8() != 0;
    uint32_t c;
    if (!r.count(c, RISU_MIN)) return false;
    t.risuitems_.resize(c);
    for (RIsuItem &v : t.risuitems_)
      if (!get_risu(r, v)) return false;
    if (!get_risu(r, t.an_risu_) || !get_isu(r, t.risu_last_)) return false;
    if (!r.count(c, ISU_MIN)) return false;
    t.isuitems_.resize(c);
    for (IsuItem &v : t.isuitems_)
      if (!get_isu(r, v)) return false;
    if (!get_isu(r, t.an_isu_) || !get_isu(r, t.lastvalid_) || !get_acars(r, t.an_)) return false;
    if (!r.count(c, FRAG_MIN)) return false;
    t.frags_.resize(c);
    for (Frag &f : t.frags_) {
      if (!get_acars(r, f.item)) return false;
      f.count = r.i32();
    }
    return r.ok && r.left() == 0;  // the state fills its bytes exactly
  };
  const bool good = parse();
  if (!good) t = PChannelHost(fragments_only_);  // as newly constructed
  // (items is an output: what this object has emitted stays with it)
  std::vector<aero_acars_item> keep;
  keep.swap(items);
  *this = std::move(t);
  items.swap(keep);
  return good;
}

uint8_t *blob_write(uint8_t *dst, const aero_channel_cfg &cfg, uint32_t flags, uint64_t fingerprint, size_t dev_len,
                    const std::string &host) {
  std::string h;
  BlobWriter w(h);
  w.bytes(BLOB_MAGIC, 8);
  w.u32(BLOB_VERSION);
  w.i32(cfg.bitrate);
  w.i32(cfg.burst);
  w.u32(cfg.fs);
  w.i32(cfg.disable_reassembly);
  w.u32(flags);
  w.u64(fingerprint);
  w.u64((uint64_t)blob_size(dev_len, host.size()));
  w.u64((uint64_t)dev_len);
  memcpy(dst, h.data(), h.size());
  uint8_t *dev = dst + h.size();
  std::string t;
  BlobWriter w2(t);
  w2.u64((uint64_t)host.size());
  memcpy(dev + dev_len, t.data(), 8);
  if (!host.empty()) memcpy(dev + dev_len + 8, host.data(), host.size());
  return dev;
}

bool blob_parse(const uint8_t *src, size_t bytes, BlobHeader &h) {
  if (!src) return false;
  BlobReader r(src, bytes);
  const uint8_t *m = r.take(8);
  if (!m || memcmp(m, BLOB_MAGIC, 8)) return false;
  if (r.u32() != BLOB_VERSION || !r.ok) return false;
  h.cfg.bitrate = r.i32();
  h.cfg.burst = r.i32();
  h.cfg.fs = r.u32();
  h.cfg.disable_reassembly = r.i32();
  h.flags = r.u32();
  h.fingerprint = r.u64();
  h.total = r.u64();
  if (!r.ok || h.total > bytes || h.total < blob_size(0, 0)) return false;
  BlobReader b(src, (size_t)h.total);  // the sections lie inside the blob's own length
  b.take(BLOB_HEADER);
  h.dev_len = b.u64();
  if (!b.ok || h.dev_len > b.left()) return false;
  h.dev = b.take((size_t)h.dev_len);
  h.host_len = b.u64();
  if (!b.ok || h.host_len > b.left()) return false;
  h.host = b.take((size_t)h.host_len);
  return b.ok && b.left() == 0;  // total is exactly the header and the two sections
}

void ContHost::save(std::string &out, const PChannelHost *live) const {
  BlobWriter w(out);
  w.u32(HOST_TAG_CONT);
  w.i64(avail);
  w.i64(nsamp);
  w.i64(hops);
  w.i64(hop_base);
  w.i64(soft_seen);
  w.i64(pre_end);
  w.i32(c_cd);
  w.i32(c_dcd);
  w.i32(c_edges);
  w.u32((uint32_t)msg_end.size());
  for (long long v : msg_end) w.i64(v);
  w.u32((uint32_t)infofield.size());
  w.bytes(infofield.data(), infofield.size());
  put_phost(w, live ? live : host.get());
}

bool ContHost::load(const uint8_t *src, size_t n) {
  if (!src) return false;
  BlobReader r(src, n);
  if (r.u32() != HOST_TAG_CONT || !r.ok) return false;
  avail = r.i64();
  nsamp = r.i64();
  hops = r.i64();
  hop_base = r.i64();
  soft_seen = r.i64();
  pre_end = r.i64();
  c_cd = r.i32();
  c_dcd = r.i32();
  c_edges = r.i32();
  uint32_t c;
  if (!r.count(c, 8)) return false;
  msg_end.clear();
  for (uint32_t k = 0; k < c; k++) msg_end.push_back(r.i64());
  if (!r.count(c, 1)) return false;
  const uint8_t *q = r.take(c);
  if (!r.ok) return false;
  infofield.assign(q, q + c);
  if (!get_phost(r, host)) return false;
  if (!r.ok || r.left() != 0) return false;
  // counters a run indexes rings with: pushed >= demodulated >= 0, the hop
  // count that of the demodulated samples, message ends in order
  if (nsamp < 0 || avail < nsamp || hops < 0 || hop_base < 0 || soft_seen < 0 || pre_end < 0) return false;
  long long last = pre_end;
  for (long long v : msg_end) {
    if (v < last || v > avail) return false;
    last = v;
  }
  return true;
}

void BurstHost::save(std::string &out, const PChannelHost *live) const {
  BlobWriter w(out);
  w.u32(HOST_TAG_BURST);
  w.i64(avail);
  w.i64(chunk_n);
  w.i64(hb_base);
  w.i64(soft_seen);
  w.i32(tsu);
  w.i32(tblocks);
  w.i32(ok_burst);
  w.i32(hops_seen);
  w.i32(since_run);
  put_phost(w, live ? live : host.get());
}

bool BurstHost::load(const uint8_t *src, size_t n) {
  if (!src) return false;
  BlobReader r(src, n);
  if (r.u32() != HOST_TAG_BURST || !r.ok) return false;
  avail = r.i64();
  chunk_n = r.i64();
  hb_base = r.i64();
  soft_seen = r.i64();
  tsu = r.i32();
  tblocks = r.i32();
  ok_burst = r.i32();
  hops_seen = r.i32();
  since_run = r.i32();
  if (!get_phost(r, host)) return false;
  if (!r.ok || r.left() != 0) return false;
  return avail >= 0 && hb_base >= 0 && hb_base <= avail && chunk_n >= 0 && soft_seen >= 0 && since_run >= 0;
}

}  // namespace aero
