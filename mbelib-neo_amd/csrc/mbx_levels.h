// mbx_levels.h -- the arithmetic of levels out and of the gated mix-down (include/mbx_levels.h): the level of a row, the RANK KEY that
// orders the inputs of a bus, and "the N-th largest key of a bus", stated ONCE for the host definitions (mbx_pcm_levels_host,
// mbx_mixdown_gated_host, mbx_levels.hip), for the kernels (pcm_levels_kernel, mixdown_gated_kernel, mixdown_gated_long_kernel,
// mbx_levels.hip) and for the CPU program that holds them to a plain sort (tests/levels_check.cpp).  Host-visible in the manner of
// mbx_mixdown.h: plain C++, nothing here needs a device compile, no HIP types, no globals.
//
//   level    energy = sum x^2 (uint64: 160 * 2^30 < 2^38), peak = max |x| with |x| an int32 (32768 for -32768), clipped = the count
//            of 32767 and -32768.  Sums and maxima of integers: any partition over lanes gives the same record.
//   key      0 for a CLOSED input (peak < open_peak), else ((energy << 12) | (4095 - k)) + 1 for the input at position k of its bus:
//            energy < 2^38 and k < 2^12, so a key has at most 51 bits, is never 0 for an open input, and two inputs of one bus never
//            share one.  A larger key is a louder input; at equal energy the smaller k has the larger key.
//   gate     threshold = the N-th largest key of the bus (N = loudest_n), or 1 where N is 0 or the bus has fewer than N open inputs;
//            an input is CHOSEN iff its key >= threshold.  Keys are unique, so exactly min(N, open) inputs are chosen when N > 0.
#pragma once

#include <stdint.h>

#include "mbx_mixdown.h"   // (this directory's: the forms, kMixdownMaxInputs, MBX_COMPAND_FN)

namespace mbx {

constexpr int kGateMaxLoudest = 8;     // MBX_GATE_MAX_LOUDEST
constexpr int kGateMaxPeak = 32768;    // the largest peak a row can have: an open_peak above it is refused

// pcm_levels_kernel's partition (mbx_levels.hip): 16 lanes per row, 4 rows per 64-lane wave; lane j of a row owns the ten samples
// 10 j .. 10 j + 9
constexpr int kLevelLanes = 16;
constexpr int kLevelSamples = 160 / kLevelLanes;

static_assert(kMixdownMaxInputs <= (1 << 12), "a position in a bus fits the 12 low bits of a key");

struct Level {   // a row's level, or a part of it
    uint64_t energy = 0;
    uint32_t peak = 0;
    uint32_t clipped = 0;
};

MBX_COMPAND_FN void level_add_sample(Level& l, int16_t x) {
    const int32_t a = x < 0 ? -(int32_t)x : (int32_t)x;   // 0 .. 32768
    l.energy += (uint64_t)((uint32_t)a * (uint32_t)a);     // (a^2 <= 2^30)
    l.peak = (uint32_t)a > l.peak ? (uint32_t)a : l.peak;
    l.clipped += (x == 32767 || x == -32768) ? 1u : 0u;
}

MBX_COMPAND_FN void level_merge(Level& l, const Level& other) {
    l.energy += other.energy;
    l.peak = other.peak > l.peak ? other.peak : l.peak;
    l.clipped += other.clipped;
}

// the level of a row of 160 samples, straight
MBX_COMPAND_FN Level level_of_row(const int16_t* x) {
    Level l;
    for (int n = 0; n < 160; ++n) {
        level_add_sample(l, x[n]);
    }
    return l;
}

// the record's second 8 bytes: peak in bits 0 .. 15 (32768 fits uint16), clipped in bits 16 .. 31, zero above
MBX_COMPAND_FN uint32_t level_peak_word(const Level& l) { return l.peak | (l.clipped << 16); }

// the rank key of the input at position k of its bus, from its row's energy and peak
MBX_COMPAND_FN uint64_t gate_key(uint64_t energy, uint32_t peak, int32_t k, uint32_t open_peak) {
    return peak >= open_peak ? ((energy << 12) | (uint64_t)(4095 - k)) + 1u : 0u;
}
MBX_COMPAND_FN int32_t gate_key_position(uint64_t key) { return 4095 - (int32_t)((key - 1u) & 4095u); }   // of an open input's key

// the largest keys seen so far, in decreasing order (zeros: none yet): one more key
MBX_COMPAND_FN void gate_insert(uint64_t top[kGateMaxLoudest], uint64_t key) {
    for (int i = 0; i < kGateMaxLoudest; ++i) {
        const uint64_t t = top[i];
        const bool up = key > t;
        top[i] = up ? key : t;
        key = up ? t : key;
    }
}

// the threshold from those: the N-th largest, or 1 (every open input) where N is 0 or fewer than N keys are open
MBX_COMPAND_FN uint64_t gate_threshold_of(const uint64_t top[kGateMaxLoudest], int loudest_n) {
    uint64_t t = 0;
    for (int i = 0; i < kGateMaxLoudest; ++i) {
        t = i == loudest_n - 1 ? top[i] : t;
    }
    return t ? t : 1u;
}

// THE definition: the threshold of a bus from the keys of its inputs
MBX_COMPAND_FN uint64_t gate_threshold(const uint64_t* keys, int32_t count, int loudest_n) {
    uint64_t top[kGateMaxLoudest] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int32_t k = 0; loudest_n > 0 && k < count; ++k) {
        gate_insert(top, keys[k]);
    }
    return gate_threshold_of(top, loudest_n);
}

}  // namespace mbx
