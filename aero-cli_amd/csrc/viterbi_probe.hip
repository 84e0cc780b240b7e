/*
 * viterbi_probe.hip — diagnostic only (aero_device_viterbi, tests/test_gpu_viterbi.py)
 *
 * Runs each device decoder of viterbi_dev.h on soft values the caller hands
 * over, so the tests can compare them with the oracle on input the synthetic
 * streams never produce (ties, erasures, noise at the decoding threshold).
 * One wave per codeword, or per pair of codewords:
 *
 *  wave        viterbi_decode_wave, sbuf / hist / obits in LDS (this probe is
 *              the only kernel it is compiled into)
 *  regs        viterbi_decode_regs from an LDS sbuf, as rt_viterbi_kernel calls it
 *  regs2-self  viterbi_decode_regs2(src, src) from a flat source, the second
 *              output ignored: how an unpaired job is decoded
 *  regs2-pair  viterbi_decode_regs2(srcA, srcB), codewords 2k and 2k + 1 in
 *              one wave (an odd batch's last codeword decodes against itself)
 *  block / C   viterbi_decode_regs2 fed by BlockSoft<BLK> / CSoft (viterbi_src.h),
 *              built as viterbi_kernel's source() and viterbi_c_kernel build
 *              them: the old overlap goes into a register, then the last 62
 *              values of this block's stream are written out as the next
 *              overlap.  Blocks pair as in viterbi_kernel, C decodes alone.
 */
#include <hip/hip_runtime.h>

#include "../../include/aero_engine.h"
#include "burst_common.h"
#include "engine_common.h"
#include "viterbi_dev.h"
#include "viterbi_probe.h"
#include "viterbi_src.h"

namespace aero {

static_assert(VP_MAX_NSOFT == RT_BLOCK, "the probe's LDS stream holds the longest R/T block");
static_assert(VP_MAX_NSOFT / 2 <= 64 * 64, "decoded bits fit one 64-bit word per lane");
static_assert(62 + BLOCK + 24 <= VP_MAX_NSOFT && 62 + C_BLOCK + 24 <= VP_MAX_NSOFT, "production streams are no longer");

namespace {

// soft value p of a codeword stored as it is decoded; the decoder fetches
// pairs up to 64 steps past the end (and masks them), so p is bounded here
struct FlatSoft {
  const uint8_t *s;
  int n;
  __device__ __forceinline__ int get(int p, bool) const { return p < n ? s[p] : 128; }
};

// decoded bit b (bit b & 63 of obw in lane b >> 6) to out[b], b < sets
__device__ __forceinline__ void put_bits(uint64_t obw, uint64_t *ow, uint8_t *out, int sets, int lane) {
  __syncthreads();  // the previous codeword's reads of ow are done
  ow[lane] = obw;
  __syncthreads();
  for (int b = lane; b < sets; b += 64) out[b] = (uint8_t)((ow[b >> 6] >> (b & 63)) & 1ULL);
}

template <class Src>
__device__ __forceinline__ void decode2(const Src &a, const Src &b, bool pair, int nsoft, uint64_t *ow, uint8_t *outA,
                                        uint8_t *outB, int lane) {
  uint64_t obwA, obwB;
  viterbi_decode_regs2(a, b, nsoft, obwA, obwB, lane);
  put_bits(obwA, ow, outA, nsoft / 2, lane);
  if (pair) put_bits(obwB, ow, outB, nsoft / 2, lane);
}

__global__ __launch_bounds__(64) void vprobe_wave_kernel(const uint8_t *in, int nsoft, uint8_t *bits) {
  __shared__ uint8_t sbuf[VP_MAX_NSOFT];
  __shared__ unsigned long long hist[HCAP];
  __shared__ uint8_t ob[VP_MAX_NSOFT / 2];
  const int lane = threadIdx.x, sets = nsoft / 2;
  const size_t cw = blockIdx.x;
  for (int k = lane; k < nsoft; k += 64) sbuf[k] = in[cw * nsoft + k];
  for (int k = lane; k < sets; k += 64) ob[k] = 0;
  __syncthreads();
  viterbi_decode_wave(sbuf, nsoft, hist, ob, lane);
  __syncthreads();
  for (int k = lane; k < sets; k += 64) bits[cw * sets + k] = ob[k];
}

__global__ __launch_bounds__(64) void vprobe_regs_kernel(const uint8_t *in, int nsoft, uint8_t *bits) {
  __shared__ uint8_t sbuf[VP_MAX_NSOFT];
  __shared__ uint64_t ow[64];
  const int lane = threadIdx.x, sets = nsoft / 2;
  const size_t cw = blockIdx.x;
  for (int k = lane; k < nsoft; k += 64) sbuf[k] = in[cw * nsoft + k];
  __syncthreads();
  uint64_t obw;
  viterbi_decode_regs(sbuf, nsoft, obw, lane);
  put_bits(obw, ow, bits + cw * sets, sets, lane);
}

// PAIR: block k decodes codewords 2k and 2k + 1, else block k codeword k
template <bool PAIR>
__global__ __launch_bounds__(64) void vprobe_regs2_kernel(const uint8_t *in, int ncw, int nsoft, uint8_t *bits) {
  __shared__ uint64_t ow[64];
  const int lane = threadIdx.x, sets = nsoft / 2;
  const int cwA = PAIR ? 2 * (int)blockIdx.x : (int)blockIdx.x, cwB = cwA + 1;
  const bool pair = PAIR && cwB < ncw;
  const FlatSoft a{in + (size_t)cwA * nsoft, nsoft};
  const FlatSoft b{in + (size_t)(pair ? cwB : cwA) * nsoft, nsoft};
  decode2(a, b, pair, nsoft, ow, bits + (size_t)cwA * sets, bits + (size_t)cwB * sets, lane);
}

// a record: the raw block (BLK bytes, the framing kernels' storage order),
// the overlap the previous block left (62 bytes), the `first` flag, a pad byte
template <class Src, int BLK, bool PAIR>
__global__ __launch_bounds__(64) void vprobe_src_kernel(const uint8_t *in, int ncw, int nsoft, uint8_t *bits,
                                                        uint8_t *ovout) {
  __shared__ uint64_t ow[64];
  constexpr int REC = BLK + 64;
  const int lane = threadIdx.x, sets = nsoft / 2;
  auto source = [&](int cw) -> Src {
    const uint8_t *rec = in + (size_t)cw * REC;
    const int first = rec[BLK + 62] & 1;
    Src b;
    b.blk = rec;
    b.ov = first ? 0 : 62;
    b.ovr = (!first && lane < 62) ? rec[BLK + lane] : 0;
    if (lane < 62) ovout[(size_t)cw * 62 + lane] = (uint8_t)b.get(b.ov + BLK - 62 + lane, false);
    return b;
  };
  const int cwA = PAIR ? 2 * (int)blockIdx.x : (int)blockIdx.x, cwB = cwA + 1;
  const bool pair = PAIR && cwB < ncw;
  const Src a = source(cwA);
  const Src b = pair ? source(cwB) : a;
  decode2(a, b, pair, nsoft, ow, bits + (size_t)cwA * sets, bits + (size_t)cwB * sets, lane);
}

}  // namespace

int viterbi_probe_block(int variant) {
  switch (variant) {
    case AERO_VIT_WAVE:
    case AERO_VIT_REGS:
    case AERO_VIT_REGS2_SELF:
    case AERO_VIT_REGS2_PAIR: return 0;
    case AERO_VIT_BLOCK4992: return BLOCK;
    case AERO_VIT_BLOCK384: return 6 * 64;
    case AERO_VIT_BLOCK576: return 9 * 64;
    case AERO_VIT_CSOFT: return C_BLOCK;
    default: return -1;
  }
}

void launch_viterbi_probe(hipStream_t st, int variant, const uint8_t *in, int ncw, int nsoft, uint8_t *bits,
                          uint8_t *ov) {
  const dim3 one(ncw), two((ncw + 1) / 2), b(64);
  switch (variant) {
    case AERO_VIT_WAVE: hipLaunchKernelGGL(vprobe_wave_kernel, one, b, 0, st, in, nsoft, bits); break;
    case AERO_VIT_REGS: hipLaunchKernelGGL(vprobe_regs_kernel, one, b, 0, st, in, nsoft, bits); break;
    case AERO_VIT_REGS2_SELF: hipLaunchKernelGGL(vprobe_regs2_kernel<false>, one, b, 0, st, in, ncw, nsoft, bits); break;
    case AERO_VIT_REGS2_PAIR: hipLaunchKernelGGL(vprobe_regs2_kernel<true>, two, b, 0, st, in, ncw, nsoft, bits); break;
    case AERO_VIT_BLOCK4992:
      hipLaunchKernelGGL((vprobe_src_kernel<BlockSoft<BLOCK>, BLOCK, true>), two, b, 0, st, in, ncw, nsoft, bits, ov);
      break;
    case AERO_VIT_BLOCK384:
      hipLaunchKernelGGL((vprobe_src_kernel<BlockSoft<6 * 64>, 6 * 64, true>), two, b, 0, st, in, ncw, nsoft, bits, ov);
      break;
    case AERO_VIT_BLOCK576:
      hipLaunchKernelGGL((vprobe_src_kernel<BlockSoft<9 * 64>, 9 * 64, true>), two, b, 0, st, in, ncw, nsoft, bits, ov);
      break;
    case AERO_VIT_CSOFT:
      hipLaunchKernelGGL((vprobe_src_kernel<CSoft, C_BLOCK, false>), one, b, 0, st, in, ncw, nsoft, bits, ov);
      break;
    default: break;
  }
}

}  // namespace aero
