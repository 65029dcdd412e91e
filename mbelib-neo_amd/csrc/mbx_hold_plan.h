// mbx_hold_plan.h -- the held gate (include/mbx_hold.h) before it reaches a device: what mbx_mixdown_held, mbx_gate_state_set and the
// host definition refuse, the grids of its launches, and the arithmetic the host definition and the kernels share -- the DECISION of
// one input, the CODE of its transition, the WEIGHT q(n) of a sample and the RAMPED term -- stated once.  Integer work alone: no HIP,
// no locks, no globals, so that a CPU program can check it under a sanitizer (tests/hold_check.cpp), in the manner of
// mbx_levels_plan.h, whose check of a gated launch the held one reuses.  The pointers are taken as numbers and never dereferenced.
// Private to mbx_hold.hip and mbx_session.hip.
#pragma once

#include <cstddef>
#include <cstdint>

#include "mbx_levels.h"        // (this directory's: the rank key)
#include "mbx_levels_plan.h"

namespace mbx {

constexpr int kHoldMaxRampLog2 = 7;    // MBX_HOLD_MAX_RAMP_LOG2: fades of at most 128 samples, within the frame
constexpr int kHoldDecideBlock = 256;  // lanes of a workgroup of hold_decide_kernel: one lane per short bus

// |ramped| <= |term| + 1 (hold_ramped), |term| <= 2^18 + 1 (mbx_mixdown.h)
static_assert((long long)kMixdownMaxInputs * ((1ll << 18) + 2) < (1ll << 31), "the held sum of a full bus stays in int32");
static_assert(((1ll << 18) + 1) * (1ll << kHoldMaxRampLog2) + (1ll << (kHoldMaxRampLog2 - 1)) < (1ll << 31), "term * q + R / 2 stays in int32");

// ---- the state record: {uint16 hang_left, uint8 open, uint8 on} as one little-endian word -------------------------------------------
MBX_COMPAND_FN uint32_t hold_state_word(uint32_t hang, uint32_t open, uint32_t on) { return hang | (open << 16) | (on << 24); }
MBX_COMPAND_FN uint32_t hold_word_hang(uint32_t w) { return w & 0xFFFFu; }
MBX_COMPAND_FN uint32_t hold_word_open(uint32_t w) { return (w >> 16) & 0xFFu; }
MBX_COMPAND_FN uint32_t hold_word_on(uint32_t w) { return w >> 24; }
// a record a caller gives (mbx_gate_state_set, mbx_mixdown_held_host): open and on are 0 or 1, and nothing is on without being open
MBX_COMPAND_FN bool hold_word_ok(uint32_t w) { return hold_word_open(w) <= 1u && hold_word_on(w) <= 1u && hold_word_on(w) <= hold_word_open(w); }

// ---- the decision of one input ------------------------------------------------------------------------------------------------------
struct HoldParams {   // mbx_mixdown_hold as the kernels take it
    uint32_t open_peak, close_peak, hang_frames;
    int      loudest_n, ramp_log2;
};
struct HoldDecision {
    uint32_t open, hang;
};
MBX_COMPAND_FN HoldDecision hold_decide(uint32_t peak, uint32_t open_prev, uint32_t hang_prev, uint32_t open_peak, uint32_t close_peak,
                                        uint32_t hang_frames) {
    if (peak >= open_peak || (open_prev && peak >= close_peak)) {
        return HoldDecision{1u, hang_frames};
    }
    if (open_prev && hang_prev > 0) {
        return HoldDecision{1u, hang_prev - 1u};
    }
    return HoldDecision{0u, 0u};
}
// its rank key: that of mbx_levels.h, "open" as just decided (a key under open_peak 0 is that of an open input)
MBX_COMPAND_FN uint64_t hold_key(const HoldDecision& d, uint64_t energy, int32_t k) { return d.open ? gate_key(energy, 0u, k, 0u) : 0u; }

// ---- the transition and the weight --------------------------------------------------------------------------------------------------
enum HoldCode : uint32_t { kHoldOff = 0, kHoldSteady = 1, kHoldRising = 2, kHoldFalling = 3 };
MBX_COMPAND_FN uint32_t hold_code(uint32_t on_prev, uint32_t on) { return on ? (on_prev ? kHoldSteady : kHoldRising) : (on_prev ? kHoldFalling : kHoldOff); }

// q(n), n = 0 .. 159, R = 1 << ramp_log2
MBX_COMPAND_FN int32_t hold_weight(uint32_t code, int n, int ramp_log2) {
    const int32_t R = 1 << ramp_log2;
    const int32_t up = n + 1 < R ? n + 1 : R;
    return code == kHoldSteady ? R : code == kHoldRising ? up : code == kHoldFalling ? R - up : 0;
}
// (term * q + R / 2) >> ramp_log2, the shift arithmetic: term itself at q = R, 0 at q = 0
MBX_COMPAND_FN int32_t hold_ramped(int32_t term, int32_t q, int ramp_log2) { return (term * q + ((1 << ramp_log2) >> 1)) >> ramp_log2; }

// what a lane that owns the 8 samples of `piece` does with an input of this code: from sample R - 1 on a rising input weighs R and a
// falling one 0, so a piece that starts there takes the steady path or leaves the row alone
enum HoldPiece { kHoldPieceSkip = 0, kHoldPieceSteady = 1, kHoldPieceRamp = 2 };
MBX_COMPAND_FN int hold_piece_mode(uint32_t code, int piece, int ramp_log2) {
    const bool past = piece * kMixdownPiece + 1 >= (1 << ramp_log2);
    if (code == kHoldOff || (code == kHoldFalling && past)) {
        return kHoldPieceSkip;
    }
    return code == kHoldSteady || past ? kHoldPieceSteady : kHoldPieceRamp;
}

// ---- refusals -----------------------------------------------------------------------------------------------------------------------
enum HoldRefusal {
    kHoldOk = 0,
    kHoldNull,        // no hold
    kHoldClose,       // close_peak > open_peak
    kHoldPeak,        // open_peak > 32768
    kHoldLoudest,     // loudest_n > kGateMaxLoudest
    kHoldRamp,        // ramp_log2 > kHoldMaxRampLog2
    kHoldNoState,     // no state
    kHoldForeign,     // a state of another plan
    kHoldRecord,      // a state record that is not {hang, 0 / 1, 0 / 1} or is on without open
    kHoldGated,       // what mbx_mixdown_gated refuses: the LevelsRefusal (and the MixdownRefusal) say which
};
static inline const char* hold_refusal_text(HoldRefusal r) {
    switch (r) {
    case kHoldNull: return "a hold is needed (a caller without one has mbx_mixdown_gated)";
    case kHoldClose: return "close_peak is above open_peak";
    case kHoldPeak: return "open_peak is above 32768, the largest peak a row can have";
    case kHoldLoudest: return "loudest_n is above MBX_GATE_MAX_LOUDEST";
    case kHoldRamp: return "ramp_log2 is above MBX_HOLD_MAX_RAMP_LOG2";
    case kHoldNoState: return "a state is needed (mbx_gate_state_create)";
    case kHoldForeign: return "the state was made for another plan";
    case kHoldRecord: return "a state record whose open or on is not 0 or 1, or that is on without open";
    default: return "";
    }
}

// the hold alone (also what mbx_session_next_mixdown_held and mbx_mixdown_held_host refuse of it); the fields as numbers
static inline HoldRefusal hold_refused(bool have_hold, unsigned open_peak, unsigned close_peak, unsigned loudest_n, unsigned ramp_log2) {
    if (!have_hold) {
        return kHoldNull;
    }
    if (open_peak > (unsigned)kGateMaxPeak) {
        return kHoldPeak;
    }
    if (close_peak > open_peak) {
        return kHoldClose;
    }
    if (loudest_n > (unsigned)kGateMaxLoudest) {
        return kHoldLoudest;
    }
    if (ramp_log2 > (unsigned)kHoldMaxRampLog2) {
        return kHoldRamp;
    }
    return kHoldOk;
}

// the state beside the plan of the call: `state_plan` is the plan the state was made for
static inline HoldRefusal hold_state_refused(bool have_state, const void* state_plan, const void* plan) {
    if (!have_state) {
        return kHoldNoState;
    }
    return state_plan != plan ? kHoldForeign : kHoldOk;
}

// n records as words (mbx_gate_state_set, mbx_mixdown_held_host)
static inline HoldRefusal hold_records_refused(const uint32_t* words, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        if (!hold_word_ok(words[i])) {
            return kHoldRecord;
        }
    }
    return kHoldOk;
}

// mbx_mixdown_held: the hold, the state, then everything mbx_mixdown_gated refuses under the gate {open_peak, loudest_n}
// (*levels and *mix say what when kHoldGated comes back; sums: as gated_launch_refused has it)
static inline HoldRefusal held_launch_refused(const MixdownPlan* plan, const void* plan_handle, bool have_hold, unsigned open_peak, unsigned close_peak,
                                              unsigned loudest_n, unsigned ramp_log2, bool have_state, const void* state_plan, int form,
                                              const void* d_pcm16, size_t nrows, const void* d_levels, const void* d_out, LevelsRefusal* levels,
                                              MixdownRefusal* mix, bool sums = false) {
    *levels = kLevelsOk;
    *mix = kMixdownOk;
    const HoldRefusal hold = hold_refused(have_hold, open_peak, close_peak, loudest_n, ramp_log2);
    if (hold != kHoldOk) {
        return hold;
    }
    if (!have_state) {
        return kHoldNoState;
    }
    *levels = gated_launch_refused(plan, true, open_peak, loudest_n, form, d_pcm16, nrows, d_levels, d_out, mix, sums);
    if (*levels != kLevelsOk) {
        return kHoldGated;
    }
    return hold_state_refused(true, state_plan, plan_handle);   // (behind the plan's own check: a missing plan is named as that)
}

// ---- grids --------------------------------------------------------------------------------------------------------------------------
// hold_decide_kernel: one lane per short bus.  The sums: the grids of the plan (short_grid: 20 lanes per short bus; long_grid: one
// workgroup per long bus, which decides and sums its bus by itself).
static inline uint32_t hold_decide_grid(const MixdownPlan& plan) { return (uint32_t)(((uint64_t)plan.n_short + kHoldDecideBlock - 1) / kHoldDecideBlock); }
// the state object's one allocation: the records, then a code byte per input; never empty
static inline size_t hold_state_bytes(int32_t inputs) { return (size_t)inputs * 4u; }
static inline size_t hold_alloc_bytes(int32_t inputs) {
    const size_t bytes = ((size_t)inputs * 5u + 15u) & ~(size_t)15u;
    return bytes ? bytes : 16u;
}

}  // namespace mbx

// the handle of the public header: made and destroyed by mbx_hold.hip; mbx_session.hip reads the plan it is tied to
struct mbx_gate_state {
    const mbx_mixdown_plan* plan = nullptr;   // the plan it was made for: the same pointer, or mbx_mixdown_held refuses it
    int       device = -1;
    int32_t   inputs = 0;
    uint32_t* d_state = nullptr;   // one allocation on `device`: `inputs` records ...
    uint8_t*  d_code = nullptr;    // ... and behind them a code byte per input, written by hold_decide_kernel for hold_sum_kernel
};
