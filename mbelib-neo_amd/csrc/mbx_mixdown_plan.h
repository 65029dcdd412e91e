// mbx_mixdown_plan.h -- what a mix-down plan (include/mbx_mixdown.h) is before it reaches a device: the caller's CSR arrays checked,
// rows_needed, the split of the buses into SHORT ones (flat lanes, mixdown_kernel) and LONG ones (one workgroup each,
// mixdown_long_kernel), the two grid sizes, the words of the tables the kernels read, what mbx_mixdown refuses of its arguments, and
// what the three host definitions share.  Integer work on the host alone: no HIP, no locks, no globals -- so that a CPU program can
// check it under a sanitizer (tests/mixdown_check.cpp), in the manner of mbx_group_plan.h, mbx_launch_plan.h and mbe_flush_plan.h.
// At its end, for hipcc alone: the handle's way to a launch, shared by mbx_mixdown.hip, mbx_levels.hip and mbx_hold.hip.  Private;
// nothing here is exported.
#pragma once

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "mbx_mixdown.h"

namespace mbx {

// A bus with MORE inputs than this takes the long form, unless the caller states the split (mbx_mixdown_plan_create_split).  The long
// form spreads the inputs over 12 slices and pays a barrier and a pass through LDS for it, so below a couple of trips per slice there
// is nothing to win.  MEASURED on one MI355X (EXPERIMENTS.md, "Mix-down out"): 65,536 rows dealt into equal buses, the short form is
// ahead up to 20 inputs, the two are level at 22 and the long form is ahead from 24 (two trips per slice) on.
constexpr int kMixdownLongAbove = 22;

constexpr int kMixdownBlock = 256;   // lanes of a workgroup, both forms

enum MixdownRefusal {
    kMixdownOk = 0,
    kMixdownNoHandle,     // no place for the handle
    kMixdownBuses,        // n_buses < 1
    kMixdownNull,         // bus_offset is NULL, or src_row is NULL while a bus has an input
    kMixdownFirst,        // bus_offset[0] != 0
    kMixdownDecreasing,   // bus_offset decreases
    kMixdownTooLong,      // a bus with more than kMixdownMaxInputs inputs (the total fits int32 by its type: bus_offset is int32)
    kMixdownRow,          // a negative src_row
    kMixdownRowMost,      // a src_row of 2^31 - 1: rows_needed would not fit int32
    kMixdownSplit,        // a negative long_above
    // mbx_mixdown's arguments
    kMixdownForm,
    kMixdownPointers,
    kMixdownAlign,
    kMixdownRows,
    kMixdownOverlap,
};
static inline const char* mixdown_refusal_text(MixdownRefusal r) {
    switch (r) {
    case kMixdownNoHandle: return "no place for the handle";
    case kMixdownBuses: return "n_buses must be at least 1";
    case kMixdownNull: return "bus_offset and src_row are needed (only gain_q12 may be NULL: unity)";
    case kMixdownFirst: return "bus_offset[0] must be 0";
    case kMixdownDecreasing: return "bus_offset must not decrease";
    case kMixdownTooLong: return "a bus has more than MBX_MIXDOWN_MAX_INPUTS inputs";
    case kMixdownRow: return "a negative src_row";
    case kMixdownRowMost: return "a src_row of 2^31-1: the rows needed must fit int32";
    case kMixdownSplit: return "long_above must not be negative (0: the library's default)";
    case kMixdownForm: return "form is MBX_MIXDOWN_PCM16, MBX_MIXDOWN_ULAW or MBX_MIXDOWN_ALAW";
    case kMixdownPointers: return "a plan, d_pcm16 and d_out are needed";
    case kMixdownAlign: return "a pointer is below the alignment of its kind (include/mbx_mixdown.h, Alignment)";
    case kMixdownRows: return "nrows is below mbx_mixdown_plan_rows(): an input would lie outside d_pcm16";
    case kMixdownOverlap: return "d_pcm16 and d_out overlap";
    default: return "";
    }
}

// one input as the kernels read it: 8 bytes, one load
struct alignas(8) MixdownInput {
    int32_t row;    // src_row
    int32_t gain;   // gain_q12, sign-extended
};

// The plan.  The tables are ONE array of int32 words (the device copy is one allocation):
//   bus_offset[n_buses + 1] | short_bus[n_short] | long_bus[n_long] | (one word of padding where the inputs would start odd) |
//   input[inputs] (MixdownInput, 8-byte aligned in an 8-byte aligned array)
// short_bus[slot] / long_bus[workgroup] name the bus a slot of the short launch / a workgroup of the long launch sums, both in the
// caller's bus order; every bus is in exactly one of them, so the two launches together write every bus row once.
struct MixdownPlan {
    int      n_buses = 0;
    int32_t  inputs = 0;        // bus_offset[n_buses]
    int32_t  rows_needed = 0;   // 1 + the largest src_row; 0: no bus has an input
    int      long_above = 0;    // the split in force
    int      n_short = 0, n_long = 0;
    uint32_t short_grid = 0;    // workgroups of kMixdownBlock lanes: 20 lanes per short bus, flat
    uint32_t long_grid = 0;     // one workgroup per long bus
    size_t   at_short = 0, at_long = 0, at_inputs = 0, words = 0;   // word offsets into the tables, and their length
};

// THE check and the counts.  long_above: 0 takes kMixdownLongAbove; any value >= kMixdownMaxInputs makes every bus short.
static inline MixdownRefusal plan_mixdown(int n_buses, const int32_t* bus_offset, const int32_t* src_row, int long_above, MixdownPlan* out) {
    *out = MixdownPlan();
    if (n_buses < 1) {
        return kMixdownBuses;
    }
    if (!bus_offset) {
        return kMixdownNull;
    }
    if (long_above < 0) {
        return kMixdownSplit;
    }
    if (bus_offset[0] != 0) {
        return kMixdownFirst;
    }
    const int above = long_above ? long_above : kMixdownLongAbove;
    int n_long = 0;
    for (int b = 0; b < n_buses; ++b) {
        const int64_t count = (int64_t)bus_offset[b + 1] - (int64_t)bus_offset[b];
        if (count < 0) {
            return kMixdownDecreasing;
        }
        if (count > kMixdownMaxInputs) {
            return kMixdownTooLong;
        }
        n_long += count > above;
    }
    const int32_t total = bus_offset[n_buses];   // (non-decreasing from 0 in int32: it fits)
    if (total > 0 && !src_row) {
        return kMixdownNull;
    }
    int32_t most = -1;
    for (int32_t k = 0; k < total; ++k) {
        if (src_row[k] < 0) {
            return kMixdownRow;
        }
        if (src_row[k] == INT32_MAX) {
            return kMixdownRowMost;
        }
        most = src_row[k] > most ? src_row[k] : most;
    }
    out->n_buses = n_buses;
    out->inputs = total;
    out->rows_needed = most + 1;
    out->long_above = above;
    out->n_long = n_long;
    out->n_short = n_buses - n_long;
    out->short_grid = (uint32_t)(((uint64_t)out->n_short * kMixdownPieces + kMixdownBlock - 1) / kMixdownBlock);
    out->long_grid = (uint32_t)n_long;
    out->at_short = (size_t)n_buses + 1;
    out->at_long = out->at_short + (size_t)out->n_short;
    out->at_inputs = (out->at_long + (size_t)n_long + 1) & ~(size_t)1;
    out->words = out->at_inputs + 2 * (size_t)total;
    return kMixdownOk;
}

// the words of the tables: `words` has plan.words of them; the arrays are those plan_mixdown accepted
static inline void fill_mixdown_tables(const MixdownPlan& plan, const int32_t* bus_offset, const int32_t* src_row, const int16_t* gain_q12,
                                       int32_t* words) {
    size_t ns = plan.at_short, nl = plan.at_long;
    for (int b = 0; b < plan.n_buses; ++b) {
        words[b] = bus_offset[b];
        const int32_t count = bus_offset[b + 1] - bus_offset[b];
        if (count > plan.long_above) {
            words[nl++] = b;
        } else {
            words[ns++] = b;
        }
    }
    words[plan.n_buses] = plan.inputs;
    if (plan.at_inputs > plan.at_long + (size_t)plan.n_long) {
        words[plan.at_inputs - 1] = 0;   // the padding word
    }
    for (int32_t k = 0; k < plan.inputs; ++k) {
        words[plan.at_inputs + 2 * (size_t)k] = src_row[k];
        words[plan.at_inputs + 2 * (size_t)k + 1] = gain_q12 ? (int32_t)gain_q12[k] : kMixdownUnity;
    }
}

// bytes of a sample out: of a form, or of the sums (kMixdownSums, include/mbx_limit.h)
static inline size_t mixdown_sample_bytes(int out) { return out == kMixdownSums ? 4 : out == kMixdownPcm16 ? 2 : 1; }

// what a bus launch refuses of its buffers, before a device is asked for: `out` is a form that was checked, or kMixdownSums.  The
// pointers are never dereferenced.
// Alignment: d_pcm16 16 (a piece of 8 samples is one 16-byte load), d_out 16 as int16 or int32 and 8 as bytes (a piece is one store, or two).
static inline MixdownRefusal mixdown_buffers_refused(const MixdownPlan* plan, int out, const void* d_pcm16, size_t nrows, const void* d_out) {
    if (!d_pcm16 || !d_out) {
        return kMixdownPointers;
    }
    const uintptr_t in = reinterpret_cast<uintptr_t>(d_pcm16), to = reinterpret_cast<uintptr_t>(d_out);
    if ((in & 15u) != 0 || (to & (mixdown_sample_bytes(out) > 1 ? 15u : 7u)) != 0) {
        return kMixdownAlign;
    }
    if (!plan) {   // (behind the pointers' own checks: those need no plan, and a host without a device can make none)
        return kMixdownPointers;
    }
    if (nrows < (size_t)plan->rows_needed) {
        return kMixdownRows;
    }
    // (the caller's nrows rows, whether the plan reads them all or not, and the output as far as it is written)
    const uintptr_t in_bytes = (uintptr_t)nrows * 320u, to_bytes = (uintptr_t)plan->n_buses * 160u * mixdown_sample_bytes(out);
    if (in < to + to_bytes && to < in + in_bytes) {
        return kMixdownOverlap;
    }
    return kMixdownOk;
}

// what mbx_mixdown refuses of its arguments: the form, then the buffers
static inline MixdownRefusal mixdown_launch_refused(const MixdownPlan* plan, int form, const void* d_pcm16, size_t nrows, const void* d_out) {
    return mixdown_form_ok(form) ? mixdown_buffers_refused(plan, form, d_pcm16, nrows, d_out) : kMixdownForm;
}
// a caller's form as the `out` of a path a launch shares with its sums twin: never kMixdownSums, whatever number the caller gave
static inline int mixdown_out_of_form(int form) { return mixdown_form_ok(form) ? form : -1; }
// a public launch (a form, checked) or its sums twin (kMixdownSums, which no caller can give: the twins have no form argument)
static inline MixdownRefusal mixdown_out_refused(const MixdownPlan* plan, int out, const void* d_pcm16, size_t nrows, const void* d_out) {
    return out == kMixdownSums ? mixdown_buffers_refused(plan, out, d_pcm16, nrows, d_out) : mixdown_launch_refused(plan, out, d_pcm16, nrows, d_out);
}

// ---- the host definitions (mbx_mixdown_host, mbx_mixdown_gated_host, mbx_mixdown_held_host) -----------------------------------------
// what all three refuse of these arguments, in this order, behind what each refuses of its gate or hold: the form, the plan's own, the
// pointers, rows short of the plan.  nullptr: nothing, and *plan is the plan of the arrays.
// (mixdown_host_arrays_refused: all of it but the form, for the sums twins of include/mbx_limit.h, whose callers give no form)
static inline const char* mixdown_host_arrays_refused(int n_buses, const int32_t* bus_offset, const int32_t* src_row, const int16_t* pcm16, size_t nrows,
                                                      const void* out, MixdownPlan* plan) {
    const MixdownRefusal why = plan_mixdown(n_buses, bus_offset, src_row, 0, plan);
    if (why != kMixdownOk) {
        return mixdown_refusal_text(why);
    }
    if (!out || (!pcm16 && plan->rows_needed > 0)) {
        return "pcm16 and out are needed";
    }
    return nrows < (size_t)plan->rows_needed ? mixdown_refusal_text(kMixdownRows) : nullptr;
}
static inline const char* mixdown_host_refused(int form, int n_buses, const int32_t* bus_offset, const int32_t* src_row, const int16_t* pcm16,
                                               size_t nrows, const void* out, MixdownPlan* plan) {
    return mixdown_form_ok(form) ? mixdown_host_arrays_refused(n_buses, bus_offset, src_row, pcm16, nrows, out, plan) : mixdown_refusal_text(kMixdownForm);
}
// a public host definition (a form) or its sums twin (kMixdownSums)
static inline const char* mixdown_host_out_refused(int out_kind, int n_buses, const int32_t* bus_offset, const int32_t* src_row, const int16_t* pcm16,
                                                   size_t nrows, const void* out, MixdownPlan* plan) {
    return out_kind == kMixdownSums ? mixdown_host_arrays_refused(n_buses, bus_offset, src_row, pcm16, nrows, out, plan)
                                    : mixdown_host_refused(out_kind, n_buses, bus_offset, src_row, pcm16, nrows, out, plan);
}

// the 160 sums of bus b into row b of out, in `form`: the clamp, or the byte; or (kMixdownSums) as they are
static inline void mixdown_put_row(int form, const int32_t acc[160], int b, void* out) {
    for (int n = 0; n < 160; ++n) {
        if (form == kMixdownSums) {
            static_cast<int32_t*>(out)[(size_t)b * 160u + n] = acc[n];
        } else if (form == kMixdownPcm16) {
            static_cast<int16_t*>(out)[(size_t)b * 160u + n] = mixdown_clamp(acc[n]);
        } else {
            static_cast<uint8_t*>(out)[(size_t)b * 160u + n] = mixdown_byte(form, acc[n]);
        }
    }
}

// f(k) with k() the form as a constant, for the kernel instance of that form
template <class F>
static inline void mixdown_by_form(int form, F f) {
    if (form == kMixdownPcm16) {
        f(std::integral_constant<int, kMixdownPcm16>());
    } else if (form == kMixdownUlaw) {
        f(std::integral_constant<int, kMixdownUlaw>());
    } else {
        f(std::integral_constant<int, kMixdownAlaw>());
    }
}
// the same for what a launch writes: a form, or -- BESIDE the forms, not among them -- the sums
template <class F>
static inline void mixdown_by_out(int out, F f) {
    if (out == kMixdownSums) {
        f(std::integral_constant<int, kMixdownSums>());
    } else {
        mixdown_by_form(out, f);
    }
}

}  // namespace mbx

// the handle of the public header: the plan and where its tables are.  Made and destroyed by mbx_mixdown.hip; mbx_levels.hip and
// mbx_hold.hip launch their kernels from the same tables.
struct mbx_mixdown_plan {
    mbx::MixdownPlan plan;
    int      device = -1;
    int32_t* d_words = nullptr;   // the tables, one allocation on `device`
};

#ifdef __HIPCC__   // the launch side of the handle: for the units that launch from it, not for the CPU programs that check the plan
#include "mbx_host.h"

namespace mbx {

// what the kernels of a launch read of the plan's tables
struct MixdownTables {
    const int32_t *bus_offset, *short_bus, *long_bus;
    const MixdownInput* input;
};

// the handle -> its tables, for a launch on the current device: that device ready (mbx_init), and the plan made on it or refused
// (t may be NULL: mbx_gate_state_create wants the check alone)
static inline int mixdown_tables(const char* who, const mbx_mixdown_plan* p, MixdownTables* t) {
    int dev = -1;
    const int rc = ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    if (dev != p->device) {
        char text[160];
        snprintf(text, sizeof(text), "the plan was made on device %d, the current device is %d", p->device, dev);
        return refuse(who, text);
    }
    if (t) {
        *t = MixdownTables{p->d_words, p->d_words + p->plan.at_short, p->d_words + p->plan.at_long,
                           reinterpret_cast<const MixdownInput*>(p->d_words + p->plan.at_inputs)};
    }
    return 0;
}

}  // namespace mbx
#endif
