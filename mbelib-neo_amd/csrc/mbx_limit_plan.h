// mbx_limit_plan.h -- limited buses (include/mbx_limit.h) before they reach a device: what mbx_bus_limit, mbx_limit_state_set / _get /
// _reset, mbx_session_next_limit and the host definition refuse, the grid of the launch, and the arithmetic the host definition and the
// kernel share -- the magnitude of a clamped sum, the two quotients and the DECISION of one row (attack, hold, release), the gain g(n)
// of a sample and the SCALED sample in its output form -- stated once.  Integer work alone: no HIP, no locks, no globals, so that a CPU
// program can check it under a sanitizer (tests/limit_check.cpp), in the manner of mbx_agc_plan.h.  The pointers are taken as numbers and
// never dereferenced.  Private to mbx_limit.hip and mbx_session.hip.
#pragma once

#include <cstddef>
#include <cstdint>

#include "mbx_compand.h"   // (MBX_COMPAND_FN: __host__ __device__ under hipcc, plain inline elsewhere; the G.711 bytes)
#include "mbx_mixdown.h"   // (the numbering of the output forms: kMixdownPcm16 / kMixdownUlaw / kMixdownAlaw)

namespace mbx {

constexpr int      kLimitUnity = 32768;        // MBX_LIMIT_UNITY_Q15
constexpr int      kLimitMinCeiling = 1024;    // MBX_LIMIT_MIN_CEILING
constexpr int      kLimitMaxCeiling = 32767;   // MBX_LIMIT_MAX_CEILING
constexpr int      kLimitMaxHold = 255;        // the largest hold counter a record can have
constexpr int      kLimitMaxRampLog2 = 7;      // MBX_LIMIT_MAX_RAMP_LOG2 = MBX_HOLD_MAX_RAMP_LOG2
constexpr int      kLimitRangeLog2 = 22;       // MBX_LIMIT_RANGE_LOG2: the limiter's range is 128 x full scale
constexpr int32_t  kLimitRange = 1 << kLimitRangeLog2;
constexpr uint32_t kLimitFreshWord = 32768u;   // {gain_q15 32768, hold_left 0} as one little-endian word
constexpr int      kLimitBlock = 256;          // lanes of a workgroup of bus_limit_kernel: 16 buses
constexpr int      kLimitLanes = 16;           // lanes per bus: a DPP row; lane j owns the ten samples 10 j .. 10 j + 9 of every row
constexpr int      kLimitSamples = 160 / kLimitLanes;
constexpr size_t   kLimitMaxRows = (size_t)INT32_MAX;

// the bounds of include/mbx_limit.h
static_assert(((long long)kLimitMaxCeiling << 15) < (1ll << 30), "ceiling << 15, and with it every |s' * g(n)|, stays below 2^30");
static_assert(((long long)kLimitMinCeiling << 15) / kLimitRange >= 8, "need is at least 8");
static_assert((long long)kLimitUnity * (1 << kLimitMaxRampLog2) <= (1ll << 22), "(g0 - g1) * R stays in int32");
static_assert((long long)kLimitUnity * 255 + 255 < (1ll << 24), "the release term");

// ---- the state record: {uint16 gain_q15, uint16 hold_left} as one little-endian word ----------------------------------------------------
MBX_COMPAND_FN uint32_t limit_word(uint32_t gain, uint32_t hold) { return gain | (hold << 16); }
MBX_COMPAND_FN uint32_t limit_word_gain(uint32_t w) { return w & 0xFFFFu; }
MBX_COMPAND_FN uint32_t limit_word_hold(uint32_t w) { return w >> 16; }
// a record a caller gives (mbx_limit_state_set, mbx_bus_limit_host): a gain, and a hold counter hold_frames can have set
MBX_COMPAND_FN bool limit_word_ok(uint32_t w) {
    return limit_word_gain(w) >= 1u && limit_word_gain(w) <= (uint32_t)kLimitUnity && limit_word_hold(w) <= (uint32_t)kLimitMaxHold;
}

// ---- one sample in ------------------------------------------------------------------------------------------------------------------
MBX_COMPAND_FN int32_t  limit_clamped(int32_t s) { return s < -kLimitRange ? -kLimitRange : s > kLimitRange ? kLimitRange : s; }   // s'
MBX_COMPAND_FN uint32_t limit_magnitude(int32_t clamped) { return (uint32_t)(clamped < 0 ? -clamped : clamped); }                   // a

// ---- the decision of one row --------------------------------------------------------------------------------------------------------
struct LimitParams {   // mbx_limit as the kernel takes it
    uint32_t ceiling, release_q8, hold_frames;
    int      ramp_log2;
};
enum LimitEvent : uint32_t { kLimitAttack = 0, kLimitHeld = 1, kLimitReleaseSlewed = 2, kLimitReleaseStopped = 3, kLimitIdle = 4 };
struct LimitDecision {
    uint32_t gain, hold;   // (g1, h1): the record behind the row
    uint32_t need;         // the largest gain the row's peak allows
    uint32_t event;        // LimitEvent
};
// thr0 of the record in front of a row: a * g0 > ceiling << 15  <=>  a > thr0, without the wide product (g0 >= 1)
MBX_COMPAND_FN uint32_t limit_threshold(uint32_t ceiling, uint32_t g0) { return (ceiling << 15) / g0; }
// from the peak P of the clamped row, n* (the first sample above thr0, else 160) and the record (g0, h0) in front of the row
MBX_COMPAND_FN LimitDecision limit_decide(uint32_t P, uint32_t first, uint32_t g0, uint32_t h0, const LimitParams& p) {
    const uint32_t need = P <= p.ceiling ? (uint32_t)kLimitUnity : (p.ceiling << 15) / P;
    if (first < 160u) {   // (exactly need < g0)
        return LimitDecision{need, p.hold_frames, need, kLimitAttack};
    }
    if (h0 > 0u) {
        return LimitDecision{g0, h0 - 1u, need, kLimitHeld};
    }
    const uint32_t risen = g0 + ((((uint32_t)kLimitUnity - g0) * p.release_q8 + 255u) >> 8);
    if (need < risen) {
        return LimitDecision{need, 0u, need, kLimitReleaseStopped};
    }
    return LimitDecision{risen, 0u, need, g0 == (uint32_t)kLimitUnity ? kLimitIdle : kLimitReleaseSlewed};
}

// g(n), n = 0 .. 159, in ONE shape for both kinds of row: g(n) = base + ((delta * clamp(k0 + step * n, 0, R)) >> ramp_log2).
//   an attack:  base = g1, delta = g0 - g1, the weight clamp(n* - n, 0, R): g0 until R samples in front of n* = first, g1 from n* on;
//   otherwise:  base = g0, delta = g1 - g0, the weight min(n + 1, R) = clamp(1 + n, 0, R): the AGC's ramp from g0 up to g1.
// delta is never negative (an attack has g1 < g0, every other row g1 >= g0), so the shift is of a non-negative number.
struct LimitRamp {
    int32_t base, delta, k0, step;
};
MBX_COMPAND_FN LimitRamp limit_ramp(bool attack, int32_t g0, int32_t g1, int first) {
    return attack ? LimitRamp{g1, g0 - g1, first, -1} : LimitRamp{g0, g1 - g0, 1, 1};
}
MBX_COMPAND_FN int32_t limit_gain_at(const LimitRamp& r, int n, int ramp_log2) {
    const int32_t R = 1 << ramp_log2, k = r.k0 + r.step * n;
    return r.base + ((r.delta * (k < 0 ? 0 : k > R ? R : k)) >> ramp_log2);
}
// y = (s' * g + 16384) >> 15, the shift arithmetic; |s' * g| <= ceiling << 15 < 2^30 (include/mbx_limit.h, BOUNDS), so |y| <= ceiling
MBX_COMPAND_FN int16_t limit_scaled(int32_t clamped, int32_t g) { return (int16_t)((clamped * g + 16384) >> 15); }
// y in a byte form
MBX_COMPAND_FN uint8_t limit_byte(int form, int16_t y) { return pcm16_compand(form == kMixdownAlaw ? kLawAlaw : kLawUlaw, y); }

// ---- refusals -----------------------------------------------------------------------------------------------------------------------
enum LimitRefusal {
    kLimitOk = 0,
    kLimitNull,         // no limit
    kLimitCeiling,      // ceiling outside 1024 .. 32767
    kLimitRamp,         // ramp_log2 > kLimitMaxRampLog2
    kLimitZero,         // a reserved byte != 0
    kLimitNoState,      // no state
    kLimitCounts,       // a negative n or T (or buses)
    kLimitRows,         // n * T above 2^31 - 1
    kLimitForm,         // not one of the three forms
    kLimitPointers,     // a NULL d_sums or d_out
    kLimitAlign,        // d_sums below 16, d_out below 16 (int16) or 8 (bytes)
    kLimitOverlap,      // d_out overlaps d_sums
    kLimitBuses,        // n above the buses of the state
    kLimitRange_,       // first / count outside the records of a state
    kLimitNoHost,       // no host memory for records
    kLimitRecord,       // a record that is not a gain and a hold counter
    kLimitRefusals
};
static inline const char* limit_refusal_text(LimitRefusal r) {
    switch (r) {
    case kLimitNull: return "a limit is needed";
    case kLimitCeiling: return "ceiling is 1024 .. 32767";
    case kLimitRamp: return "ramp_log2 is above MBX_LIMIT_MAX_RAMP_LOG2";
    case kLimitZero: return "the zero bytes are not 0";
    case kLimitNoState: return "a state is needed (mbx_limit_state_create)";
    case kLimitCounts: return "a negative count";
    case kLimitRows: return "more than 2^31-1 rows in one launch";
    case kLimitForm: return "form is MBX_MIXDOWN_PCM16, MBX_MIXDOWN_ULAW or MBX_MIXDOWN_ALAW";
    case kLimitPointers: return "the sums in and the rows out are needed";
    case kLimitAlign: return "a pointer is below the alignment of its kind (include/mbx_limit.h, Alignment)";
    case kLimitOverlap: return "the rows out overlap the sums in";
    case kLimitBuses: return "n is above the buses of the state";
    case kLimitRange_: return "first and count name records the state does not hold";
    case kLimitNoHost: return "host memory for the records is needed";
    case kLimitRecord: return "a state record whose gain_q15 is 0 or above 32768, or whose hold_left is above 255";
    default: return "";
    }
}

// the parameters alone (also what mbx_session_next_limit and mbx_bus_limit_host refuse of them); the fields as numbers, zero the OR of
// the three reserved bytes
static inline LimitRefusal limit_refused(bool have_limit, unsigned ceiling, unsigned ramp_log2, unsigned zero) {
    if (!have_limit) {
        return kLimitNull;
    }
    if (ceiling < (unsigned)kLimitMinCeiling || ceiling > (unsigned)kLimitMaxCeiling) {
        return kLimitCeiling;
    }
    if (ramp_log2 > (unsigned)kLimitMaxRampLog2) {
        return kLimitRamp;
    }
    return zero != 0u ? kLimitZero : kLimitOk;
}

static inline size_t limit_sample_bytes(int form) { return form == kMixdownPcm16 ? 2u : 1u; }

// the shape of a call: counts, rows, the form, the two arrays (device: the alignment is looked at; the host definition passes false)
static inline LimitRefusal limit_rows_refused(long long n, long long T, int form, const void* sums, const void* out, bool device) {
    if (n < 0 || T < 0) {
        return kLimitCounts;
    }
    if ((unsigned long long)n * (unsigned long long)T > (unsigned long long)kLimitMaxRows) {   // (both below 2^31: the product fits)
        return kLimitRows;
    }
    if (!mixdown_form_ok(form)) {
        return kLimitForm;
    }
    if (!sums || !out) {
        return kLimitPointers;
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(sums), b = reinterpret_cast<uintptr_t>(out);
    if (device && ((a & 15u) != 0 || (b & (form == kMixdownPcm16 ? 15u : 7u)) != 0)) {
        return kLimitAlign;
    }
    const uintptr_t rows = (uintptr_t)n * (uintptr_t)T;
    const uintptr_t a_bytes = rows * 640u, b_bytes = rows * 160u * limit_sample_bytes(form);
    if (a < b + b_bytes && b < a + a_bytes) {
        return kLimitOverlap;
    }
    return kLimitOk;
}

// mbx_bus_limit: the parameters, the state, the shape, then n against the state (state_buses is looked at only with a state)
static inline LimitRefusal limit_launch_refused(bool have_limit, unsigned ceiling, unsigned ramp_log2, unsigned zero, bool have_state, long long state_buses,
                                                long long n, long long T, int form, const void* d_sums, const void* d_out) {
    const LimitRefusal lim = limit_refused(have_limit, ceiling, ramp_log2, zero);
    if (lim != kLimitOk) {
        return lim;
    }
    if (!have_state) {
        return kLimitNoState;
    }
    const LimitRefusal rows = limit_rows_refused(n, T, form, d_sums, d_out, true);
    if (rows != kLimitOk) {
        return rows;
    }
    return n > state_buses ? kLimitBuses : kLimitOk;
}

// mbx_limit_state_reset / _get / _set: records first .. first + count - 1 of `buses`
static inline LimitRefusal limit_range_refused(bool have_state, long long buses, long long first, long long count) {
    if (!have_state) {
        return kLimitNoState;
    }
    return first < 0 || count < 0 || first + count > buses ? kLimitRange_ : kLimitOk;
}

// n records as words (mbx_limit_state_set, mbx_bus_limit_host)
static inline LimitRefusal limit_records_refused(const uint32_t* words, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        if (!limit_word_ok(words[i])) {
            return kLimitRecord;
        }
    }
    return kLimitOk;
}

// ---- the grid and the allocation ------------------------------------------------------------------------------------------------------
// bus_limit_kernel: 16 lanes per bus, whatever T
static inline uint32_t limit_grid(size_t n) { return (uint32_t)((n * (size_t)kLimitLanes + kLimitBlock - 1) / kLimitBlock); }
static inline size_t limit_state_bytes(int32_t buses) { return (size_t)buses * 4u; }
// the records in whole 16s (never empty), and behind them the scratch of buses * 160 sums, which so starts 16-byte aligned
static inline size_t limit_records_room(int32_t buses) {
    const size_t bytes = (limit_state_bytes(buses) + 15u) & ~(size_t)15u;
    return bytes ? bytes : 16u;
}
static inline size_t limit_sums_bytes(int32_t buses) { return (size_t)buses * 640u; }
static inline size_t limit_alloc_bytes(int32_t buses) { return limit_records_room(buses) + limit_sums_bytes(buses); }

}  // namespace mbx

// the handle of the public header: made and destroyed by mbx_limit.hip; mbx_session.hip reads its device, its size and its scratch
struct mbx_limit_state {
    int       device = -1;
    int32_t   buses = 0;
    uint32_t* d_state = nullptr;   // `buses` records on `device`, one allocation with ...
    int32_t*  d_sums = nullptr;    // ... the scratch: buses * 160 int32, 16-byte aligned
};
