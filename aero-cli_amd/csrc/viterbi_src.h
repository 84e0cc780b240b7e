// The soft-value sources viterbi_decode_regs2 (viterbi_dev.h) reads a
// continuous job's decoder input through: BlockSoft for the P-channel
// interleaver blocks (aerol.hip viterbi_kernel), CSoft for the C channel's
// depunctured frames (cchan.hip viterbi_c_kernel).  Shared with the
// diagnostic probe (viterbi_probe.hip), which builds them the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "engine_common.h"

namespace aero {

// soft value p of a job's decoder input: the 62 overlap values of the
// previous block (lane p's ovr), then the block deinterleaved on the fly
// (deinterleave_ba, decode/aerol.cpp:594-613: position j * 64 + l comes from
// row (27 l) mod 64, column j), then erasures (128)
template <int BLK>
struct BlockSoft {
  const uint8_t *blk;
  int ov, ovr;
  // called by every lane; may_ov (wave-uniform): p may be an overlap position
  __device__ __forceinline__ int get(int p, bool may_ov) const {
    const int q = p - ov;
    int v = 128;
    if (q >= 0 && q < BLK) v = blk[(((q & 63) * 27) & 63) * (BLK / 64) + (q >> 6)];
    if (may_ov) {
      const int o = __builtin_amdgcn_ds_bpermute((p & 63) << 2, ovr);
      if (q < 0) v = o;
    }
    return v;
  }
};

// soft value p of a C job's decoder input: the previous frame's last 62
// depunctured values, the 5460 depunctured ones (erasures at 4k + 3), 24 erasures
struct CSoft {
  const uint8_t *blk;
  int ov, ovr;
  __device__ __forceinline__ int get(int p, bool may_ov) const {
    const int qq = p - ov;
    int v = 128;
    if (qq >= 0 && qq < C_BLOCK && (qq & 3) != 3) v = blk[qq];
    if (may_ov) {
      const int o = __builtin_amdgcn_ds_bpermute((p & 63) << 2, ovr);
      if (qq < 0) v = o;
    }
    return v;
  }
};

}  // namespace aero
