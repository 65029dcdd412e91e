// mbx_mixdown_lanes.h -- what a lane of the bus kernels does with its PIECE of 8 samples of one bus: find its bus, load one input's 16
// bytes and add them times the gain, walk the inputs of a bus four at a time, pass the piece through the 12 slices of a long bus, store
// it in the form of the instance; and how the keys of a long bus lie over a workgroup.  Device code, stated once for the kernels
// of THREE units: mbx_mixdown.hip, their gated twins in mbx_levels.hip (include/mbx_levels.h) and the held ones in mbx_hold.hip
// (include/mbx_hold.h).  The arithmetic is mbx_mixdown.h.
#pragma once

#include "mbx_device.h"
#include "mbx_mixdown.h"
#include "mbx_mixdown_plan.h"

namespace mbx {

// ---- the bus of a lane or of a workgroup --------------------------------------------------------------------------------------------
struct MixdownBus {
    int     bus;         // in the caller's order
    int32_t lo, count;   // its inputs: input[lo .. lo + count)
};
// bus_of: short_bus[] or long_bus[] of the plan's tables; at: the slot of a short launch, the workgroup of a long one
__device__ __forceinline__ MixdownBus mixdown_bus_at(const int32_t* __restrict__ bus_offset, const int32_t* __restrict__ bus_of, size_t at) {
    const int bus = bus_of[at];
    const int32_t lo = bus_offset[bus], count = bus_offset[bus + 1] - lo;
    return MixdownBus{bus, lo, count};
}

// a lane of a short launch: lane = slot * 20 + piece, flat over the grid.  Slots from n_short on are not live: their lanes leave, and
// only a live lane asks for the bus of its slot.
struct MixdownSlot {
    size_t slot;
    int    piece;
};
__device__ __forceinline__ MixdownSlot mixdown_short_slot() {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t slot = g / kMixdownPieces;
    return MixdownSlot{slot, (int)(g - slot * kMixdownPieces)};
}

// ---- one input ----------------------------------------------------------------------------------------------------------------------
// the 16 bytes of the input's row at the lane's piece, as eight samples
__device__ __forceinline__ void mixdown_load_piece(const int16_t* __restrict__ pcm16, const MixdownInput in, int piece, int16_t x[kMixdownPiece]) {
    const uint4 v = *reinterpret_cast<const uint4*>(pcm16 + (size_t)in.row * 160u + (size_t)(piece * kMixdownPiece));
    x[0] = (int16_t)(v.x & 0xFFFFu), x[1] = (int16_t)(v.x >> 16), x[2] = (int16_t)(v.y & 0xFFFFu), x[3] = (int16_t)(v.y >> 16);
    x[4] = (int16_t)(v.z & 0xFFFFu), x[5] = (int16_t)(v.z >> 16), x[6] = (int16_t)(v.w & 0xFFFFu), x[7] = (int16_t)(v.w >> 16);
}

// one input's piece times the gain, into the lane's sums
__device__ __forceinline__ void mixdown_add_input(const int16_t* __restrict__ pcm16, const MixdownInput in, int piece, int32_t acc[kMixdownPiece]) {
    int16_t x[kMixdownPiece];
    mixdown_load_piece(pcm16, in, piece, x);
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

// the lane's eight sums -> the piece of the bus row, in the form of the instance: one 16-byte or one 8-byte store; a sums instance
// (kMixdownSums, include/mbx_limit.h) stores the eight sums themselves, two 16-byte stores
template <int kOut>
__device__ __forceinline__ void mixdown_store(void* __restrict__ out, int bus, int piece, const int32_t acc[kMixdownPiece]) {
    const size_t at = (size_t)bus * 160u + (size_t)(piece * kMixdownPiece);
    if constexpr (kOut == kMixdownSums) {
        int4* const to = reinterpret_cast<int4*>(static_cast<int32_t*>(out) + at);
        to[0] = int4{acc[0], acc[1], acc[2], acc[3]};
        to[1] = int4{acc[4], acc[5], acc[6], acc[7]};
    } else if constexpr (kOut == kMixdownPcm16) {
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

// ---- the tail of a long bus ---------------------------------------------------------------------------------------------------------
// A workgroup of 256 is 12 input SLICES x 20 pieces (lanes 240 .. 255 only keep the barriers company).  A kernel declares
//     __shared__ __attribute__((aligned(16))) MixdownPart part;
// has every lane of a slice PUT its sums into its slice's row, reaches __syncthreads(), and has its first 20 lanes ADD the 12 rows of
// their piece to sums that start at zero, and store.  The loop over the rows stays in the kernel: a helper that holds it reaches the
// kernel unrolled, and the compiler then orders the operands of the adds another way than it does for the kernel's own loop.
typedef int32_t MixdownPart[kMixdownSlices][160];

__device__ __forceinline__ void mixdown_part_put(MixdownPart& part, int slice, int piece, const int32_t acc[kMixdownPiece]) {
    int4* const to = reinterpret_cast<int4*>(&part[slice][piece * kMixdownPiece]);
    to[0] = int4{acc[0], acc[1], acc[2], acc[3]};
    to[1] = int4{acc[4], acc[5], acc[6], acc[7]};
}

__device__ __forceinline__ void mixdown_part_add(const MixdownPart& part, int slice, int piece, int32_t acc[kMixdownPiece]) {
    const int4* const from = reinterpret_cast<const int4*>(&part[slice][piece * kMixdownPiece]);
    const int4 a = from[0], b = from[1];
    acc[0] += a.x, acc[1] += a.y, acc[2] += a.z, acc[3] += a.w, acc[4] += b.x, acc[5] += b.y, acc[6] += b.z, acc[7] += b.w;
}

// ---- the keys of a long bus ---------------------------------------------------------------------------------------------------------
// The 256 lanes of a workgroup hold the keys of a bus, lane tid those of inputs tid, tid + 256, ...: at most 16, in registers; a
// workgroup-wide maximum over them is a 64-lane reduction per wave and one word per wave through LDS.  (The N rounds themselves are
// written out in mixdown_gated_long_kernel and in hold_long_kernel: behind a shared helper, whole or in parts, the compiler states the
// branch conditions of the rounds another way in both, and a kernel whose code changes keeps its own body.)
constexpr int kGateKeysPerLane = kMixdownMaxInputs / kMixdownBlock;   // 16
constexpr int kGateWaves = kMixdownBlock / 64;                        // 4: the kernels of this library are built for 64-lane waves
static_assert(kGateKeysPerLane * kMixdownBlock == kMixdownMaxInputs, "the lanes of a workgroup hold the keys of a full bus");

}  // namespace mbx
