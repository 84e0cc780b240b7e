// Host view of the coarse kernel's LDS map (aero-cli_amd/csrc/coarse_lds.h)
// for the 16384-point kinds: the region table and the byte offset of every
// word of the overlapped head's ring image.  tests/test_coarse_lds_map.py
// checks what it reports against the limits the kernel relies on.
#include <cstdint>

#include "../aero-cli_amd/csrc/coarse_lds.h"

using namespace aero;

namespace {
constexpr int L = 14, YLEN = clds::YHI14 - clds::YLO14 + 1;
using Ovl = clds::Map<L, YLEN, true>;
using Plain = clds::Map<L, YLEN, false>;

template <class M>
void fill(int *r) {
  const int v[] = {M::LDS_OFF,   M::LDS_BYTES,   M::TW_OFF,    M::TW_BYTES,  M::SPARE_OFF, M::SPARE_BYTES,
                   M::REDV_OFF,  M::REDV_BYTES,  M::REDI_OFF,  M::REDI_BYTES, M::LOGTAB_OFF, M::LOGTAB_BYTES,
                   M::IMG_OFF,   M::IMG_BYTES,   M::Y_BYTES,   M::TOTAL,      clds::LDS_LIMIT, M::N};
  for (unsigned k = 0; k < sizeof v / sizeof v[0]; ++k) r[k] = v[k];
}
}  // namespace

// regions[18]: offset and size in bytes of lds, s_tw, spare, red_v, red_i,
// logtab and the image, then the bytes of ylds, the total, the limit and N
extern "C" void coarse_lds_regions(int overlap, int *regions) {
  if (overlap)
    fill<Ovl>(regions);
  else
    fill<Plain>(regions);
}

// off[j]: byte offset in the workgroup's LDS of ring word j's place in the
// image, j = 0 .. N-1
extern "C" void coarse_lds_image(int *off) {
  for (int j = 0; j < Ovl::N; ++j) off[j] = Ovl::IMG_OFF + 4 * Ovl::img(j);
}

// byte offset of y bin q's double in ylds
extern "C" int coarse_lds_ybin(int q) { return 8 * clds::ypad(q); }

// The image as the kernel fills it: wave w's i-th direct-to-LDS load brings
// ring words 64 w + lane + 1024 i.  word[lane], off[lane]: the ring word each
// lane loads and the byte offset of its place (tests/test_coarse_lds_map_dma.py)
extern "C" void coarse_lds_image_waveload(int w, int i, int *word, int *off) {
  for (int lane = 0; lane < 64; ++lane) {
    const int j = 64 * w + lane + Ovl::FT * i;
    word[lane] = j;
    off[lane] = Ovl::IMG_OFF + 4 * Ovl::img(j);
  }
}

namespace {
int bitrev14(int p) {
  int r = 0;
  for (int b = 0; b < L; ++b) r |= ((p >> b) & 1) << (L - 1 - b);
  return r;
}
}  // namespace

// The gather's read of the image: thread t = 64 w + lane reads, for its
// element i of a snapshot that starts at sample s0, ring word
// q = (s0 + bitrev14(16 t + i)) & (N - 1).  off[lane]: the byte offset read,
// in this map (old_map = 0) or in the map the image had when it was written
// through registers, one pad word per 16 (old_map = 1), from the same base
extern "C" void coarse_lds_image_read(int w, int i, int s0, int old_map, int *off) {
  for (int lane = 0; lane < 64; ++lane) {
    const int t = 64 * w + lane;
    const int q = (s0 + bitrev14(16 * t + i)) & (Ovl::N - 1);
    off[lane] = Ovl::IMG_OFF + 4 * (old_map ? Ovl::img16(q) : Ovl::img(q));
  }
}
