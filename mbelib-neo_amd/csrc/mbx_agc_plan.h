// mbx_agc_plan.h -- levelled rows (include/mbx_agc.h) before they reach a device: what mbx_pcm_agc, mbx_agc_state_set / _get / _reset,
// mbx_session_next_agc and the host definition refuse, the grid of the launch, and the arithmetic the host definition and the kernel
// share -- the DECISION of one row (envelope, wanted gain, slewed gain), the gain g(n) of a sample and the SCALED sample -- stated
// once.  Integer work alone: no HIP, no locks, no globals, so that a CPU program can check it under a sanitizer (tests/agc_check.cpp),
// in the manner of mbx_hold_plan.h.  The pointers are taken as numbers and never dereferenced.  Private to mbx_agc.hip and
// mbx_session.hip.
#pragma once

#include <cstddef>
#include <cstdint>

#include "mbx_compand.h"   // (MBX_COMPAND_FN: __host__ __device__ under hipcc, plain inline elsewhere)

namespace mbx {

constexpr int      kAgcUnity = 1024;        // MBX_AGC_UNITY_Q10
constexpr int      kAgcMaxGain = 32768;     // MBX_AGC_MAX_GAIN_Q10
constexpr int      kAgcMaxPeak = 32768;     // the largest peak a row can have (mbx_levels.h), and the largest envelope
constexpr int      kAgcMaxRampLog2 = 7;     // MBX_AGC_MAX_RAMP_LOG2 = MBX_HOLD_MAX_RAMP_LOG2
constexpr uint32_t kAgcFreshWord = 1024u;   // {gain_q10 1024, env 0} as one little-endian word
constexpr int      kAgcBlock = 256;         // lanes of a workgroup of pcm_agc_kernel: 16 entries
constexpr int      kAgcLanes = 16;          // lanes per entry: a DPP row; lane j owns the ten samples 10 j .. 10 j + 9 of every row
constexpr int      kAgcSamples = 160 / kAgcLanes;
constexpr size_t   kAgcMaxRows = (size_t)INT32_MAX;

// the bounds of include/mbx_agc.h
static_assert((long long)kAgcMaxGain * 32768 + 512 < (1ll << 31), "x * g + 512 stays in int32");
static_assert((long long)kAgcMaxGain * (1 << kAgcMaxRampLog2) < (1ll << 23), "(g1 - g0) * R stays in int32");
static_assert((long long)kAgcMaxPeak * 255 + 255 < (1ll << 24) && (long long)kAgcMaxGain * 255 + 255 < (1ll << 24), "the decay and the rise terms");
static_assert((32767ll << 10) < (1ll << 25), "target_peak << 10");

// ---- the state record: {uint16 gain_q10, uint16 env} as one little-endian word ---------------------------------------------------------
MBX_COMPAND_FN uint32_t agc_word(uint32_t gain, uint32_t env) { return gain | (env << 16); }
MBX_COMPAND_FN uint32_t agc_word_gain(uint32_t w) { return w & 0xFFFFu; }
MBX_COMPAND_FN uint32_t agc_word_env(uint32_t w) { return w >> 16; }
// a record a caller gives (mbx_agc_state_set, mbx_pcm_agc_host): a gain, and an envelope a row can have
MBX_COMPAND_FN bool agc_word_ok(uint32_t w) {
    return agc_word_gain(w) >= 1u && agc_word_gain(w) <= (uint32_t)kAgcMaxGain && agc_word_env(w) <= (uint32_t)kAgcMaxPeak;
}

// ---- the decision of one row ------------------------------------------------------------------------------------------------------------
struct AgcParams {   // mbx_agc as the kernel takes it
    uint32_t target_peak, floor_peak, min_gain, max_gain, release_q8, rise_q8;
    int      ramp_log2;
};
enum AgcEvent : uint32_t { kAgcFreeze = 0, kAgcHold = 1, kAgcFall = 2, kAgcRiseSlewed = 3, kAgcRiseReached = 4 };
struct AgcDecision {
    uint32_t gain, env;   // (g1, env): the state behind the row
    uint32_t want;        // the clamped wanted gain (a frozen row: g0)
    uint32_t event;       // AgcEvent
};
// from the peak p of the row and the state (g0, env0) in front of it
MBX_COMPAND_FN AgcDecision agc_decide(uint32_t p, uint32_t g0, uint32_t env0, const AgcParams& a) {
    if (p < a.floor_peak) {
        return AgcDecision{g0, env0, g0, kAgcFreeze};
    }
    const uint32_t decayed = env0 - ((env0 * a.release_q8 + 255u) >> 8);   // (the term is at most env0)
    const uint32_t env = p > decayed ? p : decayed;                        // >= p >= floor_peak >= 1
    const uint32_t raw = (a.target_peak << 10) / env;
    const uint32_t want = raw < a.min_gain ? a.min_gain : raw > a.max_gain ? a.max_gain : raw;
    if (want <= g0) {
        return AgcDecision{want, env, want, want == g0 ? kAgcHold : kAgcFall};
    }
    const uint32_t slewed = g0 + ((g0 * a.rise_q8 + 255u) >> 8);
    return want <= slewed ? AgcDecision{want, env, want, kAgcRiseReached} : AgcDecision{slewed, env, want, kAgcRiseSlewed};
}

// g(n), n = 0 .. 159: from g0 to g1 over R = 1 << ramp_log2 samples; the shift is arithmetic
MBX_COMPAND_FN int32_t agc_gain_at(int32_t g0, int32_t g1, int n, int ramp_log2) {
    const int32_t R = 1 << ramp_log2;
    const int32_t up = n + 1 < R ? n + 1 : R;
    return g0 + (((g1 - g0) * up) >> ramp_log2);
}
// y = clamp((x * g + 512) >> 10), the shift arithmetic
MBX_COMPAND_FN int16_t agc_scaled(int16_t x, int32_t g) {
    const int32_t y = ((int32_t)x * g + 512) >> 10;
    return (int16_t)(y < -32768 ? -32768 : y > 32767 ? 32767 : y);
}

// ---- refusals -----------------------------------------------------------------------------------------------------------------------
enum AgcRefusal {
    kAgcOk = 0,
    kAgcNull,         // no agc
    kAgcTarget,       // target_peak outside 1 .. 32767
    kAgcFloor,        // floor_peak outside 1 .. 32768
    kAgcGain,         // a gain outside 1 .. 32768
    kAgcGainOrder,    // min_gain_q10 > max_gain_q10
    kAgcRamp,         // ramp_log2 > kAgcMaxRampLog2
    kAgcZero,         // zero != 0
    kAgcNoState,      // no state
    kAgcCounts,       // a negative n or T (or streams, on the host)
    kAgcRows,         // n * T above 2^31 - 1
    kAgcPointers,     // a NULL d_in or d_out
    kAgcAlign,        // d_in or d_out below 16
    kAgcOverlap,      // d_out overlaps d_in and is not d_in
    kAgcRange,        // first / count outside the records of a state
    kAgcNoHost,       // no host memory for records
    kAgcRecord,       // a record that is not a gain and an envelope
    kAgcRefusals
};
static inline const char* agc_refusal_text(AgcRefusal r) {
    switch (r) {
    case kAgcNull: return "an agc is needed";
    case kAgcTarget: return "target_peak is 1 .. 32767";
    case kAgcFloor: return "floor_peak is 1 .. 32768";
    case kAgcGain: return "min_gain_q10 and max_gain_q10 are 1 .. 32768";
    case kAgcGainOrder: return "min_gain_q10 is above max_gain_q10";
    case kAgcRamp: return "ramp_log2 is above MBX_AGC_MAX_RAMP_LOG2";
    case kAgcZero: return "the zero field is not 0";
    case kAgcNoState: return "a state is needed (mbx_agc_state_create)";
    case kAgcCounts: return "a negative count";
    case kAgcRows: return "more than 2^31-1 rows in one launch";
    case kAgcPointers: return "the rows in and out are needed";
    case kAgcAlign: return "a pointer is below the alignment of its kind (include/mbx_agc.h, Alignment)";
    case kAgcOverlap: return "the rows out overlap the rows in without being the same array";
    case kAgcRange: return "first and count name records the state does not hold";
    case kAgcNoHost: return "host memory for the records is needed";
    case kAgcRecord: return "a state record whose gain_q10 is 0 or above 32768, or whose env is above 32768";
    default: return "";
    }
}

// the parameters alone (also what mbx_session_next_agc and mbx_pcm_agc_host refuse of them); the fields as numbers
static inline AgcRefusal agc_refused(bool have_agc, unsigned target_peak, unsigned floor_peak, unsigned min_gain, unsigned max_gain, unsigned ramp_log2,
                                     unsigned zero) {
    if (!have_agc) {
        return kAgcNull;
    }
    if (target_peak < 1u || target_peak > 32767u) {
        return kAgcTarget;
    }
    if (floor_peak < 1u || floor_peak > (unsigned)kAgcMaxPeak) {
        return kAgcFloor;
    }
    if (min_gain < 1u || min_gain > (unsigned)kAgcMaxGain || max_gain < 1u || max_gain > (unsigned)kAgcMaxGain) {
        return kAgcGain;
    }
    if (min_gain > max_gain) {
        return kAgcGainOrder;
    }
    if (ramp_log2 > (unsigned)kAgcMaxRampLog2) {
        return kAgcRamp;
    }
    return zero != 0u ? kAgcZero : kAgcOk;
}

// the shape of a call: counts, rows, the two arrays (align: 16 on the device, 0 on the host: not looked at)
static inline AgcRefusal agc_rows_refused(long long n, long long T, const void* in, const void* out, unsigned align) {
    if (n < 0 || T < 0) {
        return kAgcCounts;
    }
    if ((unsigned long long)n * (unsigned long long)T > (unsigned long long)kAgcMaxRows) {   // (both below 2^31: the product fits)
        return kAgcRows;
    }
    if (!in || !out) {
        return kAgcPointers;
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    if (align && ((a | b) & (uintptr_t)(align - 1u)) != 0) {
        return kAgcAlign;
    }
    const uintptr_t bytes = (uintptr_t)n * (uintptr_t)T * 320u;
    if (a != b && a < b + bytes && b < a + bytes) {
        return kAgcOverlap;
    }
    return kAgcOk;
}

// mbx_pcm_agc: the parameters, the state, then the shape
static inline AgcRefusal agc_launch_refused(bool have_agc, unsigned target_peak, unsigned floor_peak, unsigned min_gain, unsigned max_gain, unsigned ramp_log2,
                                            unsigned zero, bool have_state, long long n, long long T, const void* d_in, const void* d_out) {
    const AgcRefusal agc = agc_refused(have_agc, target_peak, floor_peak, min_gain, max_gain, ramp_log2, zero);
    if (agc != kAgcOk) {
        return agc;
    }
    if (!have_state) {
        return kAgcNoState;
    }
    return agc_rows_refused(n, T, d_in, d_out, 16u);
}

// mbx_agc_state_reset / _get / _set: records first .. first + count - 1 of `streams`
static inline AgcRefusal agc_range_refused(bool have_state, long long streams, long long first, long long count) {
    if (!have_state) {
        return kAgcNoState;
    }
    return first < 0 || count < 0 || first + count > streams ? kAgcRange : kAgcOk;
}

// n records as words (mbx_agc_state_set, mbx_pcm_agc_host)
static inline AgcRefusal agc_records_refused(const uint32_t* words, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        if (!agc_word_ok(words[i])) {
            return kAgcRecord;
        }
    }
    return kAgcOk;
}

// ---- the grid and the allocation ------------------------------------------------------------------------------------------------------
// pcm_agc_kernel: 16 lanes per entry, whatever T
static inline uint32_t agc_grid(size_t n) { return (uint32_t)((n * (size_t)kAgcLanes + kAgcBlock - 1) / kAgcBlock); }
static inline size_t agc_state_bytes(int32_t streams) { return (size_t)streams * 4u; }
static inline size_t agc_alloc_bytes(int32_t streams) {   // whole 16s, never empty
    const size_t bytes = (agc_state_bytes(streams) + 15u) & ~(size_t)15u;
    return bytes ? bytes : 16u;
}

}  // namespace mbx

// the handle of the public header: made and destroyed by mbx_agc.hip; mbx_session.hip reads its device and its size
struct mbx_agc_state {
    int       device = -1;
    int32_t   streams = 0;
    uint32_t* d_state = nullptr;   // `streams` records on `device`
};
