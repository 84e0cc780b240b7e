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
