// viterbi_probe.hip's entry points (diagnostic: aero_device_viterbi in engine.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace aero {

constexpr int VP_MAX_NSOFT = 6080;  // the longest codeword production decodes (an R/T block)
constexpr int VP_MAX_CW = 65536;

// Block length of a production-source variant (AERO_VIT_BLOCK4992 .. AERO_VIT_CSOFT), 0 for the flat variants,
// -1 for an unknown variant
int viterbi_probe_block(int variant);

// One wave per codeword (or per pair of codewords): `in` holds ncw records
// (nsoft soft values each for the flat variants, block + 64 bytes for the
// production-source ones, include/aero_engine.h), bits takes ncw * (nsoft / 2)
// bytes, ov ncw * 62 bytes (production-source variants only).  The caller
// has validated variant, ncw and nsoft.
void launch_viterbi_probe(hipStream_t st, int variant, const uint8_t *in, int ncw, int nsoft, uint8_t *bits,
                          uint8_t *ov);

}  // namespace aero
