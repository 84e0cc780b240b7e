// chan_blob_fuzz.cpp — stand-alone check of PChannelHost::load on malformed
// input (aero-cli_amd/csrc/chan_blob.cpp, acars_host.cpp; no GPU, no Python),
// meant for a sanitizer build:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/chan_blob_fuzz.cpp aero-cli_amd/csrc/chan_blob.cpp aero-cli_amd/csrc/acars_host.cpp \
//       -o chan_blob_fuzz && ./chan_blob_fuzz
//
// A host with ISUs in flight is saved; the state is truncated at every length
// and given 2000 seeded one-byte mutations.  Every load returns true or false
// and the host goes on taking frames; after a false return it behaves as a
// new host (same items, same state afterwards).  The same is done to a whole
// channel blob's header (blob_parse) and host sections (ContHost / BurstHost).
// Exit status 0 when every case held.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../aero-cli_amd/csrc/chan_blob.h"

using namespace aero;

namespace {

struct Frame {
  uint8_t info[312];
  uint32_t mask;
};

// one P-channel frame of 26 SUs: ISUs (0x71) of several AESs with `seq` SSUs to come, then some of their SSUs
Frame make_frame(int round) {
  Frame f{};
  f.mask = 0x3FFFFFF;
  for (int k = 0; k < 26; k++) {
    uint8_t *su = f.info + 12 * k;
    const int aes = 0x400000 + ((round * 7 + k / 2) % 9);
    if (k % 2 == 0) {
      su[0] = 0x71;
      su[1] = (uint8_t)(aes >> 16);
      su[2] = (uint8_t)(aes >> 8);
      su[3] = (uint8_t)aes;
      su[4] = 0x90;
      su[5] = (uint8_t)(((k / 2) & 0xF) << 4 | (round & 0xF));
      su[6] = (uint8_t)(2 + (k + round) % 5);  // SSUs to come
      su[7] = (uint8_t)(((3 + k) % 9) << 4);
      su[8] = (uint8_t)('A' + k);
      su[9] = (uint8_t)('a' + round % 26);
    } else {
      su[0] = (uint8_t)(0xC0 | ((1 + (k + round) % 5) & 0x3F));
      su[1] = (uint8_t)((((k - 1) / 2) & 0xF) << 4 | (round & 0xF));
      for (int i = 2; i < 10; i++) su[i] = (uint8_t)(0x20 + ((i * 5 + k + round) % 90));
    }
  }
  return f;
}

void feed(PChannelHost &h, int from, int to) {
  for (int r = from; r < to; r++) {
    const Frame f = make_frame(r);
    h.frame(f.info, 312, f.mask, 1);
  }
}

uint64_t rng_state = 0xB10B5EEDull;
uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 11);
}

std::string items_of(const PChannelHost &h) {
  std::string s;
  for (const aero_acars_item &it : h.items) s.append(reinterpret_cast<const char *>(&it), offsetof(aero_acars_item, msg) + it.msg_len);
  return s;
}

int failures = 0;
#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
      failures++;                                             \
    }                                                         \
  } while (0)

}  // namespace

int main() {
  const int HEAD = 6, TAIL = 10;
  PChannelHost a(false);
  feed(a, 0, HEAD);
  std::string state;
  a.save(state);
  PChannelHost fresh(false);
  std::string fresh_state;
  fresh.save(fresh_state);
  CHECK(state.size() > fresh_state.size() + 64);
  feed(fresh, HEAD, TAIL);
  const std::string fresh_items = items_of(fresh);
  fresh_state.clear();
  fresh.save(fresh_state);

  int taken = 0, refused = 0;
  auto attempt = [&](const std::string &s) {
    PChannelHost h(false);
    feed(h, 0, HEAD);  // something in it, so that "as a new host" shows
    h.items.clear();
    // (a copy of exactly s.size() bytes: a read past the end is the sanitizer's to see)
    std::vector<uint8_t> buf(s.begin(), s.end());
    const bool ok = h.load(buf.data(), buf.size());
    feed(h, HEAD, TAIL);
    if (ok) {
      taken++;
    } else {
      refused++;
      std::string after;
      h.save(after);
      CHECK(items_of(h) == fresh_items);
      CHECK(after == fresh_state);
    }
    return ok;
  };
  CHECK(attempt(state));
  for (size_t n = 0; n < state.size(); n++) CHECK(!attempt(state.substr(0, n)));
  for (int i = 0; i < 2000; i++) {
    std::string m = state;
    m[rnd() % m.size()] ^= (char)(1 + rnd() % 255);
    attempt(m);
  }

  // a whole blob: the header and the host sections under the same treatment
  ContHost c;
  c.avail = 123456;
  c.nsamp = 120000;
  c.hops = 7;
  c.pre_end = 121000;
  c.msg_end = {122000, 123456};
  c.infofield.assign(40, 0x55);
  std::string chost, bhost;
  c.save(chost, &a);
  BurstHost b;
  b.avail = 5000;
  b.hb_base = 4096;
  b.save(bhost, &a);
  {
    ContHost t;
    CHECK(t.load(reinterpret_cast<const uint8_t *>(chost.data()), chost.size()));
    BurstHost u;
    CHECK(u.load(reinterpret_cast<const uint8_t *>(bhost.data()), bhost.size()));
  }
  const aero_channel_cfg cfg = {10500, 0, 48000, 0};
  std::vector<uint8_t> blob(blob_size(100, chost.size()));
  memset(blob_write(blob.data(), cfg, 0, 0x1234, 100, chost), 0xAB, 100);
  BlobHeader hd;
  CHECK(blob_parse(blob.data(), blob.size(), hd) && hd.dev_len == 100 && hd.host_len == chost.size());
  int blob_taken = 0;
  auto blob_attempt = [&](const std::vector<uint8_t> &v) {
    BlobHeader h;
    if (!blob_parse(v.data(), v.size(), h)) return false;
    CHECK(h.total <= v.size() && h.dev + h.dev_len <= v.data() + v.size() && h.host + h.host_len <= v.data() + v.size());
    ContHost t;
    (void)t.load(h.host, (size_t)h.host_len);
    BurstHost u;
    (void)u.load(h.host, (size_t)h.host_len);
    blob_taken++;
    return true;
  };
  for (size_t n = 0; n < blob.size(); n++) CHECK(!blob_attempt(std::vector<uint8_t>(blob.begin(), blob.begin() + n)));
  for (int i = 0; i < 2000; i++) {
    std::vector<uint8_t> m = blob;
    m[i < 600 ? (size_t)(i % 64) : rnd() % m.size()] ^= (uint8_t)(1 + rnd() % 255);
    blob_attempt(m);
  }
  for (int i = 0; i < 2000; i++) {
    std::string m = i % 2 ? chost : bhost;
    m[rnd() % m.size()] ^= (char)(1 + rnd() % 255);
    ContHost t;
    (void)t.load(reinterpret_cast<const uint8_t *>(m.data()), m.size());
    BurstHost u;
    (void)u.load(reinterpret_cast<const uint8_t *>(m.data()), m.size());
  }
  printf("state %zu bytes: %d loads taken, %d refused; blob %zu bytes: %d mutated blobs parsed; %d failures\n",
         state.size(), taken, refused, blob.size(), blob_taken, failures);
  return failures ? 1 : 0;
}
