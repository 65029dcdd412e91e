// mbx_levels_plan.h -- what mbx_pcm_levels and mbx_mixdown_gated (include/mbx_levels.h) refuse of their arguments before a device is
// asked for, and the grid of the levels launch.  Integer work on the host alone: no HIP, no locks, no globals -- so that a CPU program
// can check it under a sanitizer (tests/levels_check.cpp), in the manner of mbx_mixdown_plan.h, whose check of a mix-down launch the
// gated one reuses.  The pointers are taken as numbers and never dereferenced.  Private to mbx_levels.hip and mbx_session.hip.
#pragma once

#include <cstddef>
#include <cstdint>

#include "mbx_levels.h"
#include "mbx_mixdown_plan.h"

namespace mbx {

constexpr int    kLevelsBlock = 256;                        // lanes of a workgroup of pcm_levels_kernel: 16 rows
constexpr size_t kLevelsMaxRows = (size_t)INT32_MAX;        // rows of one launch: row numbers are int32 everywhere (mbx_mixdown_plan.h)
constexpr size_t kLevelBytes = 16;                          // sizeof(mbx_row_level)

enum LevelsRefusal {
    kLevelsOk = 0,
    kLevelsPointers,       // a NULL d_pcm16 or d_levels
    kLevelsAlign,          // d_pcm16 or d_levels below 16
    kLevelsRows,           // more than kLevelsMaxRows rows
    kLevelsOverlap,        // d_levels overlaps d_pcm16 (or, gated, d_out)
    kGateNull,             // no gate
    kGateLoudest,          // loudest_n > kGateMaxLoudest
    kGatePeak,             // open_peak > kGateMaxPeak
    kGateMixdown,          // what mbx_mixdown refuses: the MixdownRefusal says which
};
static inline const char* levels_refusal_text(LevelsRefusal r) {
    switch (r) {
    case kLevelsPointers: return "d_pcm16 and d_levels are needed";
    case kLevelsAlign: return "a pointer is below the alignment of its kind (include/mbx_levels.h, Alignment)";
    case kLevelsRows: return "more than 2^31-1 rows in one launch";
    case kLevelsOverlap: return "d_levels overlaps d_pcm16 or d_out";
    case kGateNull: return "a gate is needed (an ungated caller has mbx_mixdown)";
    case kGateLoudest: return "loudest_n is above MBX_GATE_MAX_LOUDEST";
    case kGatePeak: return "open_peak is above 32768, the largest peak a row can have";
    default: return "";
    }
}

static inline uint32_t levels_grid(size_t nrows) { return (uint32_t)((nrows * (size_t)kLevelLanes + kLevelsBlock - 1) / kLevelsBlock); }

static inline bool ranges_overlap(uintptr_t a, uintptr_t a_bytes, uintptr_t b, uintptr_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

// mbx_pcm_levels: d_pcm16 16 (a lane loads a piece of 8 samples at once), d_levels 16 (a record is one store)
static inline LevelsRefusal levels_launch_refused(const void* d_pcm16, size_t nrows, const void* d_levels) {
    if (!d_pcm16 || !d_levels) {
        return kLevelsPointers;
    }
    const uintptr_t in = reinterpret_cast<uintptr_t>(d_pcm16), to = reinterpret_cast<uintptr_t>(d_levels);
    if ((in & 15u) != 0 || (to & 15u) != 0) {
        return kLevelsAlign;
    }
    if (nrows > kLevelsMaxRows) {
        return kLevelsRows;
    }
    if (ranges_overlap(in, (uintptr_t)nrows * 320u, to, (uintptr_t)nrows * kLevelBytes)) {
        return kLevelsOverlap;
    }
    return kLevelsOk;
}

// the gate alone (also what mbx_session_next_mixdown_gated and mbx_mixdown_gated_host refuse of it); the fields as numbers
static inline LevelsRefusal gate_refused(bool have_gate, unsigned open_peak, unsigned loudest_n) {
    if (!have_gate) {
        return kGateNull;
    }
    if (loudest_n > (unsigned)kGateMaxLoudest) {
        return kGateLoudest;
    }
    if (open_peak > (unsigned)kGateMaxPeak) {
        return kGatePeak;
    }
    return kLevelsOk;
}

// mbx_mixdown_gated: the gate, d_levels by itself, then everything mbx_mixdown refuses (*mix says what when kGateMixdown comes back),
// then d_levels against the two arrays of that launch.  sums: the sums twin (include/mbx_limit.h) -- `form` is not looked at, d_out is int32
static inline LevelsRefusal gated_launch_refused(const MixdownPlan* plan, bool have_gate, unsigned open_peak, unsigned loudest_n, int form,
                                                 const void* d_pcm16, size_t nrows, const void* d_levels, const void* d_out, MixdownRefusal* mix,
                                                 bool sums = false) {
    *mix = kMixdownOk;
    const int out = sums ? kMixdownSums : mixdown_out_of_form(form);
    const LevelsRefusal gate = gate_refused(have_gate, open_peak, loudest_n);
    if (gate != kLevelsOk) {
        return gate;
    }
    if (!d_levels) {
        return kLevelsPointers;
    }
    const uintptr_t lv = reinterpret_cast<uintptr_t>(d_levels);
    if ((lv & 15u) != 0) {
        return kLevelsAlign;
    }
    *mix = mixdown_out_refused(plan, out, d_pcm16, nrows, d_out);
    if (*mix != kMixdownOk) {
        return kGateMixdown;
    }
    if (nrows > kLevelsMaxRows) {
        return kLevelsRows;
    }
    const uintptr_t lv_bytes = (uintptr_t)nrows * kLevelBytes;
    if (ranges_overlap(lv, lv_bytes, reinterpret_cast<uintptr_t>(d_pcm16), (uintptr_t)nrows * 320u)
        || ranges_overlap(lv, lv_bytes, reinterpret_cast<uintptr_t>(d_out), (uintptr_t)plan->n_buses * 160u * mixdown_sample_bytes(out))) {
        return kLevelsOverlap;
    }
    return kLevelsOk;
}

}  // namespace mbx
