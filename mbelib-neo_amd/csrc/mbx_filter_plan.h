// mbx_filter_plan.h -- filtered rows (include/mbx_filter.h) before they reach a device: what mbx_pcm_filter, mbx_filter_state_set / _get /
// _reset, mbx_session_next_filter and the host definition refuse, the grid of the launch, and the arithmetic the host definition and the
// kernel share -- ONE SAMPLE THROUGH ONE SECTION (filter_section) and the state record as eight little-endian words -- stated once.
// Integer work alone: no HIP, no locks, no globals, so that a CPU program can check it under a sanitizer (tests/filter_check.cpp), in the
// manner of mbx_agc_plan.h.  The pointers are taken as numbers and never dereferenced.  Private to mbx_filter.hip and mbx_session.hip.
#pragma once

#include <cstddef>
#include <cstdint>

#include "mbx_compand.h"   // (MBX_COMPAND_FN: __host__ __device__ under hipcc, plain inline elsewhere)

#if defined(__HIPCC__)
#define MBX_FILTER_UNROLL _Pragma("unroll")   // (the state of a chain lives in registers under static indices)
#else
#define MBX_FILTER_UNROLL
#endif

namespace mbx {

constexpr int    kFilterMaxSections = 4;     // MBX_FILTER_MAX_SECTIONS
constexpr int    kFilterUnity = 16384;        // MBX_FILTER_UNITY_Q14
constexpr int    kFilterShift = 14;
constexpr int    kFilterCoeffBound = 65535;   // MBX_FILTER_COEFF_BOUND
constexpr int    kFilterRecordWords = 8;      // a record is 32 bytes
constexpr int    kFilterBlock = 64;           // lanes of a workgroup of pcm_filter_kernel: one wave, a lane per entry
constexpr int    kFilterRowWords = 80;        // a row of 160 int16
constexpr int    kFilterRowStride = 81;       // ... and its stride in LDS: odd, so that the 32 lanes of a half-wave walk 32 banks
constexpr size_t kFilterMaxRows = (size_t)INT32_MAX;

// the bounds of include/mbx_filter.h
static_assert(32768ll * kFilterCoeffBound < (1ll << 31), "ff and fb stay in int32");
static_assert(2 * 32768ll * kFilterCoeffBound + 16383 < (1ll << 33), "acc needs 34 bits signed");
static_assert(((2 * 32768ll * kFilterCoeffBound + 16383) >> kFilterShift) < (1ll << 19), "|q| < 2^19");
static_assert(kFilterRowStride % 2 == 1 && kFilterRowStride > kFilterRowWords, "the padded row");

// ---- one sample through one section ---------------------------------------------------------------------------------------------------
struct FilterCoeffs {   // a section of mbx_filter as the kernel takes it: int16 values, Q14
    int16_t b0, b1, b2, a1, a2;
};
struct FilterParams {   // mbx_filter as the kernel takes it, by value
    FilterCoeffs sec[kFilterMaxSections];
};
// y[n] of the section from its input x, the two inputs and the two outputs in front of it and the saved fraction e (in and out).
// ff and fb are int32 sums of 16 x 16-bit products; their combination is taken in 64 bits and shifted once; the shift floors.
MBX_COMPAND_FN int32_t filter_section(const FilterCoeffs& c, int32_t x, int32_t x1, int32_t x2, int32_t y1, int32_t y2, uint32_t& e) {
    const int32_t ff = (int32_t)c.b0 * x + (int32_t)c.b1 * x1 + (int32_t)c.b2 * x2;
    const int32_t fb = (int32_t)c.a1 * y1 + (int32_t)c.a2 * y2;
    const int64_t acc = (int64_t)ff - (int64_t)fb + (int64_t)e;
    const int32_t q = (int32_t)(acc >> kFilterShift);   // |q| < 2^19
    e = (uint32_t)acc & (uint32_t)(kFilterUnity - 1);   // acc - (q << 14): the low 14 bits of the two's complement
    return q < -32768 ? -32768 : q > 32767 ? 32767 : q;
}

// ---- the state record: 16 halfwords {x1, x2, (y1, y2, e) x 4, 0, 0} as eight little-endian words -------------------------------------
// halfword h of a record: x1 is 0, x2 is 1, and y1, y2, e of section s are 2 + 3 s, 3 + 3 s, 4 + 3 s
MBX_COMPAND_FN uint32_t filter_half(const uint32_t* w, int h) { return (w[h >> 1] >> (16 * (h & 1))) & 0xFFFFu; }
MBX_COMPAND_FN int32_t filter_sext(uint32_t half) { return (int32_t)(int16_t)(uint16_t)half; }
// a record a caller gives (mbx_filter_state_set, mbx_pcm_filter_host): every e a fraction, the pad zero
MBX_COMPAND_FN bool filter_record_ok(const uint32_t* w) {
    for (int s = 0; s < kFilterMaxSections; ++s) {
        if (filter_half(w, 4 + 3 * s) >= (uint32_t)kFilterUnity) {
            return false;
        }
    }
    return w[kFilterRecordWords - 1] == 0u;
}

// One sample through S sections over the unpacked record: x1[0], x2[0] are the inputs in front of section 0; y1[s], y2[s] the outputs
// in front of section s, which are the inputs in front of section s + 1.  Returns y of the last section.
template <int S>
MBX_COMPAND_FN int32_t filter_chain(const FilterParams& f, int32_t x, int32_t& x1, int32_t& x2, int32_t (&y1)[kFilterMaxSections],
                                    int32_t (&y2)[kFilterMaxSections], uint32_t (&e)[kFilterMaxSections]) {
    int32_t in = x, in1 = x1, in2 = x2;
    x2 = x1, x1 = x;
    MBX_FILTER_UNROLL
    for (int s = 0; s < S; ++s) {
        const int32_t y = filter_section(f.sec[s], in, in1, in2, y1[s], y2[s], e[s]);
        in1 = y1[s], in2 = y2[s];   // what section s + 1 has in front of it
        y2[s] = y1[s], y1[s] = y;
        in = y;
    }
    return in;
}

// ---- refusals -----------------------------------------------------------------------------------------------------------------------
enum FilterRefusal {
    kFilterOk = 0,
    kFilterNull,         // no filter
    kFilterSections,     // sections outside 1 .. 4
    kFilterZero,         // a zero byte that is not 0
    kFilterBound,        // a section whose |b0| + |b1| + |b2| or |a1| + |a2| is above 65535
    kFilterBeyond,       // a non-zero coefficient beyond `sections`
    kFilterNoState,      // no state
    kFilterCounts,       // a negative n or T (or streams, on the host)
    kFilterRows,         // n * T above 2^31 - 1
    kFilterPointers,     // a NULL d_in or d_out
    kFilterAlign,        // d_in or d_out below 16
    kFilterOverlap,      // d_out overlaps d_in and is not d_in
    kFilterRange,        // first / count outside the records of a state
    kFilterNoHost,       // no host memory for records
    kFilterRecord,       // a record with an e above 16383 or a non-zero pad
    kFilterRefusals
};
static inline const char* filter_refusal_text(FilterRefusal r) {
    switch (r) {
    case kFilterNull: return "a filter is needed";
    case kFilterSections: return "sections is 1 .. MBX_FILTER_MAX_SECTIONS";
    case kFilterZero: return "the zero bytes are not 0";
    case kFilterBound: return "a section whose |b0| + |b1| + |b2| or |a1| + |a2| is above 65535";
    case kFilterBeyond: return "a non-zero coefficient beyond sections";
    case kFilterNoState: return "a state is needed (mbx_filter_state_create)";
    case kFilterCounts: return "a negative count";
    case kFilterRows: return "more than 2^31-1 rows in one launch";
    case kFilterPointers: return "the rows in and out are needed";
    case kFilterAlign: return "a pointer is below the alignment of its kind (include/mbx_filter.h, Alignment)";
    case kFilterOverlap: return "the rows out overlap the rows in without being the same array";
    case kFilterRange: return "first and count name records the state does not hold";
    case kFilterNoHost: return "host memory for the records is needed";
    case kFilterRecord: return "a state record whose e is above 16383, or whose pad is not 0";
    default: return "";
    }
}

// the filter alone (also what mbx_session_next_filter and mbx_pcm_filter_host refuse of it): `coeffs` is the 20 int16 of sec[4], read
// only where there is a filter
static inline FilterRefusal filter_refused(bool have_filter, unsigned sections, unsigned zero, const int16_t* coeffs) {
    if (!have_filter) {
        return kFilterNull;
    }
    if (sections < 1u || sections > (unsigned)kFilterMaxSections) {
        return kFilterSections;
    }
    if (zero != 0u) {
        return kFilterZero;
    }
    const auto mag = [](int16_t v) { return v < 0 ? -(int32_t)v : (int32_t)v; };
    for (unsigned s = 0; s < sections; ++s) {
        const int16_t* const c = coeffs + 5u * s;
        if (mag(c[0]) + mag(c[1]) + mag(c[2]) > kFilterCoeffBound || mag(c[3]) + mag(c[4]) > kFilterCoeffBound) {
            return kFilterBound;
        }
    }
    for (unsigned k = 5u * sections; k < 5u * (unsigned)kFilterMaxSections; ++k) {
        if (coeffs[k] != 0) {
            return kFilterBeyond;
        }
    }
    return kFilterOk;
}

// the shape of a call: counts, rows, the two arrays (align: 16 on the device, 0 on the host: not looked at)
static inline FilterRefusal filter_rows_refused(long long n, long long T, const void* in, const void* out, unsigned align) {
    if (n < 0 || T < 0) {
        return kFilterCounts;
    }
    if ((unsigned long long)n * (unsigned long long)T > (unsigned long long)kFilterMaxRows) {   // (both below 2^31: the product fits)
        return kFilterRows;
    }
    if (!in || !out) {
        return kFilterPointers;
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    if (align && ((a | b) & (uintptr_t)(align - 1u)) != 0) {
        return kFilterAlign;
    }
    const uintptr_t bytes = (uintptr_t)n * (uintptr_t)T * 320u;
    if (a != b && a < b + bytes && b < a + bytes) {
        return kFilterOverlap;
    }
    return kFilterOk;
}

// mbx_pcm_filter: the filter, the state, then the shape
static inline FilterRefusal filter_launch_refused(bool have_filter, unsigned sections, unsigned zero, const int16_t* coeffs, bool have_state, long long n,
                                                  long long T, const void* d_in, const void* d_out) {
    const FilterRefusal why = filter_refused(have_filter, sections, zero, coeffs);
    if (why != kFilterOk) {
        return why;
    }
    if (!have_state) {
        return kFilterNoState;
    }
    return filter_rows_refused(n, T, d_in, d_out, 16u);
}

// mbx_filter_state_reset / _get / _set: records first .. first + count - 1 of `streams`
static inline FilterRefusal filter_range_refused(bool have_state, long long streams, long long first, long long count) {
    if (!have_state) {
        return kFilterNoState;
    }
    return first < 0 || count < 0 || first + count > streams ? kFilterRange : kFilterOk;
}

// n records as words, eight each (mbx_filter_state_set, mbx_pcm_filter_host)
static inline FilterRefusal filter_records_refused(const uint32_t* words, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        if (!filter_record_ok(words + i * (size_t)kFilterRecordWords)) {
            return kFilterRecord;
        }
    }
    return kFilterOk;
}

// ---- the grid and the allocation ------------------------------------------------------------------------------------------------------
// pcm_filter_kernel: a lane per entry, whatever T
static inline uint32_t filter_grid(size_t n) { return (uint32_t)((n + kFilterBlock - 1) / kFilterBlock); }
static inline size_t filter_state_bytes(int32_t streams) { return (size_t)streams * 32u; }
static inline size_t filter_alloc_bytes(int32_t streams) {   // never empty
    const size_t bytes = filter_state_bytes(streams);
    return bytes ? bytes : 32u;
}

}  // namespace mbx

// the handle of the public header: made and destroyed by mbx_filter.hip; mbx_session.hip reads its device and its size
struct mbx_filter_state {
    int       device = -1;
    int32_t   streams = 0;
    uint32_t* d_state = nullptr;   // `streams` records of eight words on `device`
};
