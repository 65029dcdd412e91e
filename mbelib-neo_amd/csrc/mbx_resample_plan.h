// mbx_resample_plan.h -- wide rows (include/mbx_resample.h) before they reach a device: what mbx_pcm_resample, mbx_resample_state_set /
// _get / _reset, mbx_session_next_resample and the host definition refuse, the phase-sum check, the PACKING of the taps as the kernel
// takes them, the grid of the launch, the sizes, and the arithmetic the host definition and the kernel share -- the dot product of two
// packed pairs, the rounded and clamped sample, and resample_sample(), the one place the sum over the taps is written.  Integer work
// alone: no HIP, no locks, no globals, so that a CPU program can check it under a sanitizer (tests/resample_check.cpp), in the manner of
// mbx_agc_plan.h.  The pointers of a call are taken as numbers and never dereferenced.  Private to mbx_resample.hip and mbx_session.hip.
#pragma once

#include <cstddef>
#include <cstdint>

#include "mbx_compand.h"   // (MBX_COMPAND_FN: __host__ __device__ under hipcc, plain inline elsewhere)

namespace mbx {

constexpr int    kResampleMaxTaps = 192;      // MBX_RESAMPLE_MAX_TAPS
constexpr int    kResampleUnity = 16384;      // MBX_RESAMPLE_UNITY_Q14
constexpr int    kResampleHistory = 32;       // MBX_RESAMPLE_HISTORY: samples of a record
constexpr int    kResampleMaxK = 32;          // taps per phase
constexpr int    kResampleMaxL = 6;
constexpr int    kResamplePhaseBound = 65535; // the largest sum of |taps| a phase may have
constexpr int    kResampleRound = 8192;       // half of 1 << 14
constexpr int    kResampleBlock = 256;        // lanes of a workgroup of pcm_resample_kernel: 16 rows
constexpr int    kResampleLanes = 16;         // lanes per row; lane j owns the ten input samples 10 j .. 10 j + 9 and their 10 L outputs
constexpr int    kResampleSamples = 160 / kResampleLanes;
constexpr int    kResampleRecordWords = kResampleHistory / 2;                 // a record as dwords: one per lane of a row
constexpr int    kResampleWindowWords = (kResampleHistory + 160) / 2;         // x_ext of a row as dwords: 96
constexpr int    kResamplePairs = kResampleMaxTaps / 2;                       // packed tap pairs: 96 dwords, 384 bytes
constexpr size_t kResampleMaxOut = (size_t)INT32_MAX;                         // samples out of one launch

// the bound of include/mbx_resample.h
static_assert((long long)kResamplePhaseBound * 32768 == 2147450880ll, "|acc| <= 65535 * 32768");
static_assert((long long)kResamplePhaseBound * 32768 + kResampleRound < (1ll << 31), "acc + 8192 stays in int32");
static_assert(kResampleHistory >= kResampleMaxK - 1 && kResampleHistory % 2 == 0, "the record holds every earlier sample a row's first output needs");
static_assert(kResampleRecordWords % 4 == 0 && kResampleWindowWords % 4 == 0, "a record and a window are whole 16-byte pieces");

static inline bool resample_L_ok(unsigned L) { return L == 2u || L == 3u || L == 4u || L == 6u; }
static inline bool resample_K_ok(unsigned K) { return K >= 2u && K <= (unsigned)kResampleMaxK && (K & 1u) == 0u; }

// ---- the taps as the kernel takes them --------------------------------------------------------------------------------------------------
// Two taps per dword, for the packed 16-bit dot product: pair (kk, p), kk = 0 .. K/2 - 1, is the taps k = 2 kk and k + 1 of phase p,
// (h[p + k*L], h[p + (k+1)*L]).  The tap of the OLDER sample, h[p + (k+1)*L], is the LOW half: x_ext[n - k - 1] lies below x_ext[n - k] in
// memory, so a dword of the window meets its pair as it is loaded.  Pairs are kk-major: the loop over kk reads L dwords in a row.
struct ResampleTaps {
    uint32_t pair[kResamplePairs];
    int32_t  half;   // K / 2: pairs per phase
};
MBX_COMPAND_FN uint32_t resample_pair(int16_t newer /* h[p + k*L] */, int16_t older /* h[p + (k+1)*L] */) {
    return (uint32_t)(uint16_t)older | ((uint32_t)(uint16_t)newer << 16);
}
static inline ResampleTaps resample_pack(const int16_t* taps, int L, int K) {
    ResampleTaps f = {};
    f.half = K / 2;
    for (int kk = 0; kk < K / 2; ++kk) {
        for (int p = 0; p < L; ++p) {
            f.pair[kk * L + p] = resample_pair(taps[p + 2 * kk * L], taps[p + (2 * kk + 1) * L]);
        }
    }
    return f;
}

// ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
// acc + x.lo * h.lo + x.hi * h.hi, the halves signed 16-bit, in int32 without saturation: v_dot2_i32_i16 on the device
MBX_COMPAND_FN int32_t resample_dot2(uint32_t x, uint32_t h, int32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short resample_i16x2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(resample_i16x2, x), __builtin_bit_cast(resample_i16x2, h), acc, false);
#else
    return acc + (int32_t)(int16_t)(x & 0xFFFFu) * (int32_t)(int16_t)(h & 0xFFFFu) + (int32_t)(int16_t)(x >> 16) * (int32_t)(int16_t)(h >> 16);
#endif
}
// y = clamp((acc + 8192) >> 14), the shift arithmetic
MBX_COMPAND_FN int16_t resample_rounded(int32_t acc) {
    const int32_t y = (acc + kResampleRound) >> 14;
    return (int16_t)(y < -32768 ? -32768 : y > 32767 ? 32767 : y);
}
// THE definition of one output sample, y[n*L + p]: `at` points at x_ext[n], with K - 1 samples in front of it
MBX_COMPAND_FN int16_t resample_sample(const ResampleTaps& f, int L, int p, const int16_t* at) {
    int32_t acc = 0;
    for (int kk = 0; kk < f.half; ++kk) {
        const uint32_t x = (uint32_t)(uint16_t)at[-2 * kk - 1] | ((uint32_t)(uint16_t)at[-2 * kk] << 16);
        acc = resample_dot2(x, f.pair[kk * L + p], acc);
    }
    return resample_rounded(acc);
}

// ---- refusals -----------------------------------------------------------------------------------------------------------------------
enum ResampleRefusal {
    kResampleOk = 0,
    kResampleNull,        // no filter
    kResampleL,           // L is none of 2, 3, 4, 6
    kResampleK,           // K odd or outside 2 .. 32
    kResampleZero,        // a zero byte != 0
    kResampleBeyond,      // a nonzero tap beyond K * L
    kResamplePhase,       // a phase whose |taps| sum to more than 65535
    kResampleNoState,     // no state
    kResampleCounts,      // a negative n or T (or streams, on the host)
    kResampleSize,        // n * T * 160 * L above 2^31 - 1
    kResamplePointers,    // a NULL d_in or d_out
    kResampleAlign,       // d_in or d_out below 16
    kResampleOverlap,     // d_out overlaps d_in
    kResampleRange,       // first / count outside the records of a state
    kResampleNoHost,      // no host memory for records
    kResampleRefusals
};
static inline const char* resample_refusal_text(ResampleRefusal r) {
    switch (r) {
    case kResampleNull: return "a resampler is needed";
    case kResampleL: return "L is 2, 3, 4 or 6";
    case kResampleK: return "K is even, 2 .. 32";
    case kResampleZero: return "the zero bytes are not 0";
    case kResampleBeyond: return "a nonzero tap beyond K * L";
    case kResamplePhase: return "a phase whose taps sum to more than 65535 in magnitude";
    case kResampleNoState: return "a state is needed (mbx_resample_state_create)";
    case kResampleCounts: return "a negative count";
    case kResampleSize: return "more than 2^31-1 samples out of one launch";
    case kResamplePointers: return "the rows in and out are needed";
    case kResampleAlign: return "a pointer is below the alignment of its kind (include/mbx_resample.h, Alignment)";
    case kResampleOverlap: return "the rows out overlap the rows in";
    case kResampleRange: return "first and count name records the state does not hold";
    case kResampleNoHost: return "host memory for the records is needed";
    default: return "";
    }
}

// the largest sum of |taps| over the phases of h[0 .. K*L-1]
static inline long long resample_phase_sum(const int16_t* taps, int L, int K) {
    long long worst = 0;
    for (int p = 0; p < L; ++p) {
        long long sum = 0;
        for (int k = 0; k < K; ++k) {
            const long long h = taps[p + k * L];
            sum += h < 0 ? -h : h;
        }
        worst = sum > worst ? sum : worst;
    }
    return worst;
}

// the filter alone (also what mbx_session_next_resample and mbx_pcm_resample_host refuse of it); taps: MBX_RESAMPLE_MAX_TAPS of them
static inline ResampleRefusal resample_refused(bool have, unsigned L, unsigned K, unsigned zero, const int16_t* taps) {
    if (!have) {
        return kResampleNull;
    }
    if (!resample_L_ok(L)) {
        return kResampleL;
    }
    if (!resample_K_ok(K)) {
        return kResampleK;
    }
    if (zero != 0u) {
        return kResampleZero;
    }
    for (int i = (int)(K * L); i < kResampleMaxTaps; ++i) {
        if (taps[i] != 0) {
            return kResampleBeyond;
        }
    }
    return resample_phase_sum(taps, (int)L, (int)K) > (long long)kResamplePhaseBound ? kResamplePhase : kResampleOk;
}

// the shape of a call: counts, samples out, the two arrays (align: 16 on the device, 0 on the host: not looked at)
static inline ResampleRefusal resample_rows_refused(long long n, long long T, unsigned L, const void* in, const void* out, unsigned align) {
    if (n < 0 || T < 0) {
        return kResampleCounts;
    }
    // (n and T are below 2^31 and L is at most 6: n * T fits 64 bits, and is compared before it is multiplied further)
    if ((unsigned long long)n * (unsigned long long)T > (unsigned long long)kResampleMaxOut / (160ull * L)) {
        return kResampleSize;
    }
    if (!in || !out) {
        return kResamplePointers;
    }
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    if (align && ((a | b) & (uintptr_t)(align - 1u)) != 0) {
        return kResampleAlign;
    }
    const uintptr_t in_bytes = (uintptr_t)n * (uintptr_t)T * 320u, out_bytes = in_bytes * L;
    if (a < b + out_bytes && b < a + in_bytes) {
        return kResampleOverlap;
    }
    return kResampleOk;
}

// mbx_pcm_resample: the filter, the state, then the shape
static inline ResampleRefusal resample_launch_refused(bool have, unsigned L, unsigned K, unsigned zero, const int16_t* taps, bool have_state, long long n,
                                                      long long T, const void* d_in, const void* d_out) {
    const ResampleRefusal rs = resample_refused(have, L, K, zero, taps);
    if (rs != kResampleOk) {
        return rs;
    }
    if (!have_state) {
        return kResampleNoState;
    }
    return resample_rows_refused(n, T, L, d_in, d_out, 16u);
}

// mbx_resample_state_reset / _get / _set: records first .. first + count - 1 of `streams`
static inline ResampleRefusal resample_range_refused(bool have_state, long long streams, long long first, long long count) {
    if (!have_state) {
        return kResampleNoState;
    }
    return first < 0 || count < 0 || first + count > streams ? kResampleRange : kResampleOk;
}

// ---- the grid, the allocation and the sizes ---------------------------------------------------------------------------------------------
// pcm_resample_kernel: 16 lanes per ROW
static inline uint32_t resample_grid(size_t rows) { return (uint32_t)((rows * (size_t)kResampleLanes + kResampleBlock - 1) / kResampleBlock); }
static inline size_t resample_state_bytes(int32_t streams) { return (size_t)streams * 64u; }
static inline size_t resample_alloc_bytes(int32_t streams) {   // never empty
    const size_t bytes = resample_state_bytes(streams);
    return bytes ? bytes : 64u;
}
// `rows` rows out at L: what a caller's wide buffer holds, and the wide buffer of a session's slot (rows: its buses)
static inline size_t resample_wide_bytes(size_t rows, int L) { return rows * 160u * (size_t)L * sizeof(int16_t); }

}  // namespace mbx

// the handle of the public header: made and destroyed by mbx_resample.hip; mbx_session.hip reads its device and its size
struct mbx_resample_state {
    int       device = -1;
    int32_t   streams = 0;
    uint32_t* d_state = nullptr;   // `streams` records of 16 dwords on `device`
};
