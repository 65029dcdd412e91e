// mbx_mixdown_lanes.h -- what a lane of the mix-down kernels does with its PIECE of 8 samples of one bus: add one input's 16 bytes times
// its gain, walk the inputs of a bus four at a time, store the piece in the form of the instance.  Device code, shared as it is by
// the kernels of mbx_mixdown.hip and by their gated twins in mbx_levels.hip (include/mbx_levels.h); the arithmetic is mbx_mixdown.h.
#pragma once

#include "mbx_device.h"
#include "mbx_mixdown.h"
#include "mbx_mixdown_plan.h"

namespace mbx {

// one input's piece: the 16 bytes of the row at the lane's piece, times the gain, into the lane's sums
__device__ __forceinline__ void mixdown_add_input(const int16_t* __restrict__ pcm16, const MixdownInput in, int piece, int32_t acc[kMixdownPiece]) {
    const uint4 v = *reinterpret_cast<const uint4*>(pcm16 + (size_t)in.row * 160u + (size_t)(piece * kMixdownPiece));
    const int16_t x[kMixdownPiece] = {(int16_t)(v.x & 0xFFFFu), (int16_t)(v.x >> 16), (int16_t)(v.y & 0xFFFFu), (int16_t)(v.y >> 16),
                                      (int16_t)(v.z & 0xFFFFu), (int16_t)(v.z >> 16), (int16_t)(v.w & 0xFFFFu), (int16_t)(v.w >> 16)};
    mixdown_add_piece(x, (int16_t)in.gain, acc);
}

// The lane's loop: inputs first, first + kStep, ... below count of one bus (`input` is the bus's first), FOUR at a time -- four input
// words, then four row loads, in flight together; a trip count that is no multiple of four is filled up with the batch's first input at
// a gain of 0, whose terms are (x * 0 + 2048) >> 12 = 0, so that no bus length falls back to one dependent load pair after another.
template <int kStep>
__device__ __forceinline__ void mixdown_sum(const int16_t* __restrict__ pcm16, const MixdownInput* __restrict__ input, int32_t first, int32_t count,
                                            int piece, int32_t acc[kMixdownPiece]) {
    constexpr int kBatch = 4;
    for (int32_t i = first; i < count; i += kBatch * kStep) {   // (count <= 4096: no sum here leaves int32)
        MixdownInput in[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            const int32_t k = i + j * kStep;
            in[j] = input[k < count ? k : i];
            in[j].gain = k < count ? in[j].gain : 0;
        }
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
            mixdown_add_input(pcm16, in[j], piece, acc);
        }
    }
}

// the lane's eight sums -> the piece of the bus row, in the form of the instance: one 16-byte or one 8-byte store
template <int kOut>
__device__ __forceinline__ void mixdown_store(void* __restrict__ out, int bus, int piece, const int32_t acc[kMixdownPiece]) {
    const size_t at = (size_t)bus * 160u + (size_t)(piece * kMixdownPiece);
    if constexpr (kOut == kMixdownPcm16) {
        const auto pair = [&](int i) { return (uint32_t)(uint16_t)mixdown_clamp(acc[i]) | ((uint32_t)(uint16_t)mixdown_clamp(acc[i + 1]) << 16); };
        *reinterpret_cast<uint4*>(static_cast<int16_t*>(out) + at) = uint4{pair(0), pair(2), pair(4), pair(6)};
    } else {
        const auto four = [&](int i) {
            return (uint32_t)mixdown_byte(kOut, acc[i]) | ((uint32_t)mixdown_byte(kOut, acc[i + 1]) << 8) | ((uint32_t)mixdown_byte(kOut, acc[i + 2]) << 16)
                   | ((uint32_t)mixdown_byte(kOut, acc[i + 3]) << 24);
        };
        *reinterpret_cast<uint2*>(static_cast<uint8_t*>(out) + at) = uint2{four(0), four(4)};
    }
}

}  // namespace mbx
