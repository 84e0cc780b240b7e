// hostfuzz_main.cpp — stand-alone replay of a corpus of frames and R/T packets
// through PChannelHost (aero-cli_amd/csrc/acars_host.cpp), built with
// AddressSanitizer + UndefinedBehaviorSanitizer (build.py --hostfuzz) and run
// as a program of its own: tools/hostfuzz <corpus>.  The corpus is what
// tests/test_host_su_fuzz.py writes (write_corpus): "AEROHF01", then records
//   'N' u8 disable_reassembly                      a new host
//   'F' u16 len, u32 okmask, u8 formatid, bytes    PChannelHost::frame
//   'Z'                                            PChannelHost::isu_reset
//   'P' u8 kind ('R'/'T'), u16 len, u16 nsus, bytes   PChannelHost::rt_packet
// Every payload is copied into a heap block of exactly its length, so a read
// past an information field is a heap overflow the sanitizer reports.  Prints
// the number of records and items; exit status 0 when the corpus was read to
// its end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../aero-cli_amd/csrc/acars_host.h"

namespace {
struct Reader {
  std::vector<uint8_t> buf;
  size_t pos = 0;
  bool take(void *dst, size_t n) {
    if (n > buf.size() - pos) return false;
    memcpy(dst, buf.data() + pos, n);
    pos += n;
    return true;
  }
  template <class T>
  bool get(T &v) {
    return take(&v, sizeof v);
  }
};
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <corpus>\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  Reader r;
  uint8_t chunk[65536];
  for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) r.buf.insert(r.buf.end(), chunk, chunk + n);
  fclose(f);
  char magic[8];
  if (!r.take(magic, 8) || memcmp(magic, "AEROHF01", 8) != 0) {
    fprintf(stderr, "not a host fuzz corpus\n");
    return 2;
  }
  std::unique_ptr<aero::PChannelHost> host;
  size_t records = 0, items = 0;
  uint8_t type;
  while (r.get(type)) {
    records++;
    if (type == 'N') {
      uint8_t disable;
      if (!r.get(disable)) return 3;
      if (host) items += host->items.size();
      host.reset(new aero::PChannelHost(disable != 0));
      continue;
    }
    if (!host) return 3;
    if (type == 'Z') {
      host->isu_reset();
    } else if (type == 'F') {
      uint16_t len;
      uint32_t mask;
      uint8_t fmt;
      if (!r.get(len) || !r.get(mask) || !r.get(fmt)) return 3;
      std::unique_ptr<uint8_t[]> info(new uint8_t[len ? len : 1]);
      if (!r.take(info.get(), len)) return 3;
      host->frame(info.get(), len, mask, fmt);
    } else if (type == 'P') {
      uint8_t kind;
      uint16_t len, nsus;
      if (!r.get(kind) || !r.get(len) || !r.get(nsus)) return 3;
      std::unique_ptr<uint8_t[]> info(new uint8_t[len ? len : 1]);
      if (!r.take(info.get(), len)) return 3;
      host->rt_packet(kind == 'R', info.get(), len, nsus);
    } else {
      fprintf(stderr, "unknown record %u at %zu\n", type, r.pos);
      return 3;
    }
    if (host->items.size() > 4096) {
      items += host->items.size();
      host->items.clear();
    }
  }
  if (host) items += host->items.size();
  printf("%zu records, %zu items\n", records, items);
  return 0;
}
