// mbx_bands_plan.h -- band records (include/mbx_bands.h) in integers alone: the bound of a bank, the bytes of the records, what
// mbx_band_bank_create, mbx_pcm_bands and mbx_pcm_bands_host refuse and in which order, and the arithmetic of a record, stated ONCE for
// the kernel (pcm_bands_kernel, mbx_bands.hip), for the host definition (mbx_pcm_bands_host) and for the CPU program that holds them to
// __int128 (tests/bands_check.cpp).  No HIP, no locks, no globals, in the manner of mbx_levels_plan.h and mbx_resample_plan.h.  The
// pointers of a launch are taken as numbers and never dereferenced.  Private to mbx_bands.hip and mbx_session.hip.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "mbx_compand.h"   // (MBX_COMPAND_FN)

struct mbx_band_bank {   // include/mbx_bands.h: immutable after mbx_band_bank_create
    int       device = -1;
    int       K = 0;
    uint32_t* d_probes = nullptr;   // K probes of 160 dwords, c and s interleaved by the dword (mbx::bands_interleave)
};

namespace mbx {

constexpr int      kBandsMaxProbes = 32;       // MBX_BANDS_MAX_PROBES
constexpr uint32_t kBandsVectorBound = 65535;  // MBX_BANDS_VECTOR_BOUND
constexpr int      kBandsComplex = 0, kBandsPower = 1;   // MBX_BANDS_COMPLEX, MBX_BANDS_POWER
constexpr int      kBandsVector = 160;                    // samples of a row and of a vector
constexpr int      kBandsProbeWords = kBandsVector;       // dwords of a probe: 80 of c and 80 of s
constexpr size_t   kBandsProbeBytes = 4u * kBandsProbeWords;   // 640
constexpr size_t   kBandsMaxBytes = (size_t)INT32_MAX;    // nrows * K * record_bytes of one launch
// pcm_bands_kernel's partition (mbx_bands.hip): that of pcm_levels_kernel -- 16 lanes per row of ten samples each, 4 rows per wave, 16
// rows per workgroup; a workgroup walks the 16-row groups blockIdx.x, blockIdx.x + gridDim.x, ... with the bank in LDS all the while
constexpr int      kBandsLanes = 16;
constexpr int      kBandsSamples = kBandsVector / kBandsLanes;   // 10: five dwords
constexpr int      kBandsBlock = 256;
constexpr int      kBandsBlockRows = kBandsBlock / kBandsLanes;  // 16
constexpr uint32_t kBandsMaxGrid = 2048;       // 256 CUs x the 8 workgroups of 20,480 B of LDS a CU holds

static inline bool   bands_form_ok(int form) { return form == kBandsComplex || form == kBandsPower; }
static inline size_t bands_record_bytes(int form) { return form == kBandsComplex ? 8u : 4u; }
static inline size_t bands_bank_bytes(int K) { return (size_t)K * kBandsProbeBytes; }
// the records of nrows rows; the caller has checked the form and K (nrows * 256 does not wrap for any nrows a launch accepts)
static inline size_t bands_out_bytes(size_t nrows, int K, int form) { return nrows * (size_t)K * bands_record_bytes(form); }
static inline uint32_t bands_grid(size_t nrows) {
    const size_t groups = (nrows + kBandsBlockRows - 1) / kBandsBlockRows;
    return (uint32_t)(groups < kBandsMaxGrid ? groups : kBandsMaxGrid);
}

// ---- refusals, in their order ------------------------------------------------------------------------------------------------------
enum BandsRefusal {
    kBandsOk = 0,
    kBandsPointers,    // a NULL: the handle's place, the probes, the bank, the rows or the records
    kBandsProbes,      // K outside 1 .. kBandsMaxProbes
    kBandsBound,       // a vector whose |v[n]| sum to more than kBandsVectorBound (bands_bound_text names it)
    kBandsForm,        // a form that is neither COMPLEX nor POWER
    kBandsSize,        // nrows * K * record_bytes above 2^31 - 1
    kBandsAlign,       // d_pcm16 or d_out below 16
    kBandsOverlap,     // d_out overlaps d_pcm16
};
static inline const char* bands_refusal_text(BandsRefusal r) {
    switch (r) {
    case kBandsPointers: return "a bank (or the probes and a place for its handle), the rows and a place for the records are needed";
    case kBandsProbes: return "K is 1 .. MBX_BANDS_MAX_PROBES";
    case kBandsBound: return "a vector of a probe is above MBX_BANDS_VECTOR_BOUND";
    case kBandsForm: return "form is MBX_BANDS_COMPLEX or MBX_BANDS_POWER";
    case kBandsSize: return "nrows * K * record_bytes is above 2^31-1";
    case kBandsAlign: return "a pointer is below the alignment of its kind (include/mbx_bands.h, Alignment)";
    case kBandsOverlap: return "d_out overlaps d_pcm16";
    default: return "";
    }
}

// the sum of |v[n]| of one vector: at most 160 * 32768 < 2^23
static inline uint32_t bands_vector_sum(const int16_t* v) {
    uint32_t sum = 0;
    for (int n = 0; n < kBandsVector; ++n) {
        sum += (uint32_t)(v[n] < 0 ? -(int32_t)v[n] : (int32_t)v[n]);
    }
    return sum;
}
// the first vector of a bank over the bound: *probe is its probe and *which is 'c' or 's'; false: the bank meets the bound
static inline bool bands_over_bound(const int16_t* probes, int K, int* probe, char* which, uint32_t* sum) {
    for (int k = 0; k < K; ++k) {
        for (int v = 0; v < 2; ++v) {
            const uint32_t total = bands_vector_sum(probes + ((size_t)k * 2u + (size_t)v) * kBandsVector);
            if (total > kBandsVectorBound) {
                *probe = k, *which = v ? 's' : 'c', *sum = total;
                return true;
            }
        }
    }
    return false;
}
// the text of kBandsBound: "probe 3: the |s[n]| sum to 65536, above MBX_BANDS_VECTOR_BOUND (65535)"
static inline void bands_bound_text(char* text, size_t room, int probe, char which, uint32_t sum) {
    snprintf(text, room, "probe %d: the |%c[n]| sum to %u, above MBX_BANDS_VECTOR_BOUND (65535)", probe, which, (unsigned)sum);
}

// a bank as mbx_band_bank_create and mbx_pcm_bands_host are given it: the pointers, K, the bound (*probe, *which, *sum say what broke it)
static inline BandsRefusal bands_bank_refused(bool have_place, const int16_t* probes, int K, int* probe, char* which, uint32_t* sum) {
    if (!have_place || !probes) {
        return kBandsPointers;
    }
    if (K < 1 || K > kBandsMaxProbes) {
        return kBandsProbes;
    }
    return bands_over_bound(probes, K, probe, which, sum) ? kBandsBound : kBandsOk;
}

// the form and the size, of the launch and of the host definition (K is a bank's: 1 .. 32)
static inline BandsRefusal bands_shape_refused(int K, int form, size_t nrows) {
    if (!bands_form_ok(form)) {
        return kBandsForm;
    }
    if (nrows > kBandsMaxBytes / ((size_t)K * bands_record_bytes(form))) {
        return kBandsSize;
    }
    return kBandsOk;
}

static inline bool bands_ranges_overlap(uintptr_t a, uintptr_t a_bytes, uintptr_t b, uintptr_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

// mbx_pcm_bands: K is the bank's (0: no bank)
static inline BandsRefusal bands_launch_refused(int K, int form, const void* d_pcm16, size_t nrows, const void* d_out) {
    if (K == 0 || !d_pcm16 || !d_out) {
        return kBandsPointers;
    }
    const BandsRefusal shape = bands_shape_refused(K, form, nrows);
    if (shape != kBandsOk) {
        return shape;
    }
    const uintptr_t in = reinterpret_cast<uintptr_t>(d_pcm16), to = reinterpret_cast<uintptr_t>(d_out);
    if ((in & 15u) != 0 || (to & 15u) != 0) {
        return kBandsAlign;
    }
    if (bands_ranges_overlap(in, (uintptr_t)nrows * 320u, to, (uintptr_t)bands_out_bytes(nrows, K, form))) {
        return kBandsOverlap;
    }
    return kBandsOk;
}

// ---- the arithmetic ------------------------------------------------------------------------------------------------------------------
// acc + x.lo * v.lo + x.hi * v.hi, the halves signed 16-bit, in int32 without saturation: v_dot2_i32_i16 on the device.  Under the
// bound no partial sum leaves int32, so the order of the pairs and the partition over lanes do not matter.
MBX_COMPAND_FN int32_t bands_dot2(uint32_t x, uint32_t v, int32_t acc) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short bands_i16x2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(bands_i16x2, x), __builtin_bit_cast(bands_i16x2, v), acc, false);
#else
    return acc + (int32_t)(int16_t)(x & 0xFFFFu) * (int32_t)(int16_t)(v & 0xFFFFu) + (int32_t)(int16_t)(x >> 16) * (int32_t)(int16_t)(v >> 16);
#endif
}
// a probe as the kernel reads it: 80 pairs { dword i of c, dword i of s }, a dword being the samples 2 i (low half) and 2 i + 1
static inline void bands_interleave(const int16_t* probe /* c[160], s[160] */, uint32_t* image /* 160 dwords */) {
    for (int i = 0; i < kBandsVector / 2; ++i) {
        for (int v = 0; v < 2; ++v) {
            const int16_t* const at = probe + v * kBandsVector + 2 * i;
            image[2 * i + v] = (uint32_t)(uint16_t)at[0] | ((uint32_t)(uint16_t)at[1] << 16);
        }
    }
}
// THE definition of re and of im: a row against one vector
MBX_COMPAND_FN int32_t bands_sum(const int16_t* x, const int16_t* v) {
    int32_t acc = 0;
    for (int n = 0; n < kBandsVector; n += 2) {
        acc = bands_dot2((uint32_t)(uint16_t)x[n] | ((uint32_t)(uint16_t)x[n + 1] << 16), (uint32_t)(uint16_t)v[n] | ((uint32_t)(uint16_t)v[n + 1] << 16), acc);
    }
    return acc;
}
// THE definition of the power record: (re^2 + im^2) >> 31, below 2^32 for every re and im a bank under the bound can give
MBX_COMPAND_FN uint32_t bands_power(int32_t re, int32_t im) {
    const uint64_t p = (uint64_t)((int64_t)re * (int64_t)re) + (uint64_t)((int64_t)im * (int64_t)im);
    return (uint32_t)(p >> 31);
}

}  // namespace mbx
