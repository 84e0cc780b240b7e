/*
 * coarse_lds.h — where the coarse kernel's workgroup keeps what in its LDS
 * (coarse.hip; checked on the CPU by tools/coarse_lds_sim.cpp,
 * tests/test_coarse_lds_map.py).
 *
 * One raw buffer, carved in this order:
 *
 *   lds     PADDED doubles: the transforms' exchanges, the plain head's ring
 *           image, and in a hop's tail ylds (|X| and y of the bins the fold
 *           reads) in its first YSPAN doubles
 *   s_tw    TWLEN double2: the forward twiddles of the stages served from LDS
 *   spare   what the overlapped head's image needs beyond s_tw (nothing, as
 *           the image is placed now)
 *   red_v, red_i   the fold's per-wave maxima
 *   logtab  (overlapped head only) log's 128-pair table
 *
 * The overlapped head (persistent 16384-point kinds) keeps the next
 * channel's ring image (uint32 words, one pad word per 64) in the hop's tail
 * behind ylds: over the rest of lds and all of s_tw (which the kernel writes
 * again from the twiddle table once the image is read, thread j entry j),
 * ending where s_tw ends.  The image is filled by loads that write the LDS
 * directly: one wave-load puts its 64 words at a wave-uniform base plus
 * lane x 4, so the 64 words of a wave-load (ring words 64 w + lane + 1024 i)
 * are contiguous; the pad word per 64 keeps the bit-reversed read (words 16
 * apart across a wave's lanes) on 64 different banks.
 *
 * Plain constexpr arithmetic only: compiled for the device and for the host.
 */
#pragma once

namespace aero {
namespace clds {

// fft_layout.h ypadn<6>, the padding of ylds (coarse.hip asserts they agree)
constexpr int ypad(int q) { return q + (q >> 6); }
// fft_dit.h TwLds<L>::LEN (coarse.hip asserts they agree)
constexpr int tw_len(int log2n) { return 2 * (log2n >= 14 ? 512 : 256) - 1; }
// the y bins the 16384-point kinds keep (CoarseK<MODE_OQPSK>, <MODE_C8400>)
constexpr int YLO14 = 2815, YHI14 = 13568;

constexpr int LDS_LIMIT = 160 * 1024;  // per workgroup on gfx950

template <int L, int YLEN, bool OVL>
struct Map {
  static constexpr int N = 1 << L, FT = N / 16, PADDED = N + N / 16, TWLEN = tw_len(L);
  // ylds: bin q at double ypad(q), q < YLEN
  static constexpr int YSPAN = ypad(YLEN - 1) + 1;
  static constexpr int Y_BYTES = YSPAN * 8;
  // the image: word j of the ring at uint32 img(j) from IMG_OFF
  static constexpr int img(int j) { return j + (j >> 6); }
  // the map before the image was filled by direct loads (one pad word per 16,
  // as the plain head's image in lds has): kept for the map's tests
  static constexpr int img16(int j) { return j + (j >> 4); }
  static constexpr int IMG_WORDS = img(N - 1) + 1, IMG_BYTES = IMG_WORDS * 4;

  static constexpr int LDS_OFF = 0, LDS_BYTES = PADDED * 8;
  static constexpr int TW_OFF = LDS_OFF + LDS_BYTES, TW_BYTES = TWLEN * 16;
  static constexpr int SPARE_OFF = TW_OFF + TW_BYTES;
  // the image ends where s_tw ends (it covers s_tw whole), as far behind
  // ylds as that allows
  static constexpr int IMG_OFF = SPARE_OFF - IMG_BYTES, IMG_END = IMG_OFF + IMG_BYTES;
  static constexpr int SPARE_BYTES = !OVL || IMG_END <= SPARE_OFF ? 0 : (IMG_END - SPARE_OFF + 7) / 8 * 8;
  static constexpr int REDV_OFF = SPARE_OFF + SPARE_BYTES, REDV_BYTES = FT / 64 * 8;
  static constexpr int REDI_OFF = REDV_OFF + REDV_BYTES, REDI_BYTES = FT / 64 * 4;
  // the overlapped head's copy of log's table (aero_math.h: 128 pairs), so
  // that the log10 loop's lookups do not queue with the table gathers
  static constexpr int LOGTAB_OFF = (REDI_OFF + REDI_BYTES + 15) / 16 * 16, LOGTAB_BYTES = OVL ? 128 * 16 : 0;
  static constexpr int TOTAL = OVL ? LOGTAB_OFF + LOGTAB_BYTES : REDI_OFF + REDI_BYTES;

  static_assert(YSPAN <= PADDED, "ylds inside lds");
  static_assert(TW_OFF % 16 == 0 && REDV_OFF % 8 == 0 && IMG_OFF % 4 == 0, "alignment");
  static_assert(TOTAL <= LDS_LIMIT, "one workgroup's LDS");
  // the overlay: behind ylds, not into red_*, and over s_tw whole (the kernel
  // writes all of s_tw again from the table, thread j entry j) or not at all
  static_assert(!OVL || IMG_OFF >= Y_BYTES, "image and ylds disjoint");
  static_assert(!OVL || IMG_END <= REDV_OFF, "image and red_* disjoint");
  static_assert(!OVL || IMG_END <= TW_OFF || IMG_END >= SPARE_OFF, "s_tw covered whole or not at all");
  static_assert(!OVL || TWLEN <= FT, "one s_tw entry per thread");
};

}  // namespace clds
}  // namespace aero
