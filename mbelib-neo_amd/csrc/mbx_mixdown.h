// mbx_mixdown.h -- the arithmetic of mix-down out (include/mbx_mixdown.h): one input sample times its Q12 gain, the sum of a bus, the
// clamp and the output form, stated ONCE for the host definition (mbx_mixdown_host, mbx_mixdown.hip), for the two kernels that sum on
// the device (mixdown_kernel, mixdown_long_kernel, mbx_mixdown.hip) and for the CPU program that holds them to a naive int64 loop
// (tests/mixdown_check.cpp).  Host-visible in the manner of mbx_compand.h: plain C++, nothing here needs a device compile, no HIP types.
//
//   term = (x * gain_q12 + 2048) >> 12      an int32 product (|x * g| <= 2^30), the shift arithmetic: a floor, half an LSB rounds up
//   acc  = sum of the terms                 int32: |term| <= 2^18 + 1, at most 4096 of them, so |acc| < 2^31 -- no overflow, and a sum
//                                           of integers, so every order and every partition of it gives the same bits
//   y    = clamp(acc, -32768, 32767)        once, after the sum; then the form: y itself, or its G.711 byte (mbx_compand.h)
#pragma once

#include <stdint.h>

#include "mbx_compand.h"

namespace mbx {

constexpr int kMixdownPcm16 = 0, kMixdownUlaw = 1, kMixdownAlaw = 2;   // MBX_MIXDOWN_PCM16 / _ULAW / _ALAW
constexpr int kMixdownUnity = 4096;                                     // MBX_MIXDOWN_UNITY: the Q12 gain 1.0
constexpr int kMixdownMaxInputs = 4096;                                 // MBX_MIXDOWN_MAX_INPUTS: inputs of one bus
constexpr int kMixdownPiece = 8;                                        // samples a lane owns: 16 B of an int16 row
constexpr int kMixdownPieces = 160 / kMixdownPiece;                     // 20 pieces, so 20 adjacent lanes read one 320-byte row
constexpr int kMixdownSlices = 12;                                      // long form: input slices of a workgroup (12 * 20 = 240 lanes)

static_assert((long long)kMixdownMaxInputs * ((1ll << 18) + 1) < (1ll << 31), "the sum of a full bus stays in int32");

MBX_COMPAND_FN bool mixdown_form_ok(int form) { return form == kMixdownPcm16 || form == kMixdownUlaw || form == kMixdownAlaw; }

// NOT a form, and no public number: what the sums instances of the bus kernels write (include/mbx_limit.h) -- acc itself as int32, in
// front of the clamp.  The sums launches name it beside the forms (mixdown_by_out, mbx_mixdown_plan.h); mixdown_form_ok stays as it is.
constexpr int kMixdownSums = 3;

MBX_COMPAND_FN int32_t mixdown_term(int16_t x, int16_t gain_q12) { return ((int32_t)x * (int32_t)gain_q12 + 2048) >> 12; }

MBX_COMPAND_FN int16_t mixdown_clamp(int32_t acc) { return (int16_t)(acc < -32768 ? -32768 : (acc > 32767 ? 32767 : acc)); }

// one input's piece of 8 samples into the eight sums of a lane
MBX_COMPAND_FN void mixdown_add_piece(const int16_t x[kMixdownPiece], int16_t gain_q12, int32_t acc[kMixdownPiece]) {
    for (int i = 0; i < kMixdownPiece; ++i) {
        acc[i] += mixdown_term(x[i], gain_q12);
    }
}

// the byte of a byte form (kMixdownUlaw, kMixdownAlaw) for a sum
MBX_COMPAND_FN uint8_t mixdown_byte(int form, int32_t acc) {
    return pcm16_compand(form == kMixdownAlaw ? kLawAlaw : kLawUlaw, mixdown_clamp(acc));
}

}  // namespace mbx
