// mbx_limit.hip -- limited buses (include/mbx_limit.h): a look-ahead peak limiter over the int32 sums the bus kernels wrote, in ONE launch
// behind them, with one 4-byte state record per bus kept on the device between calls.  The arithmetic and the checks are
// mbx_limit_plan.h, host-only and shared with the host definition below.  (The sums themselves are instances of the six bus kernels, in
// the units of their parents: mbx_mixdown.hip, mbx_levels.hip, mbx_hold.hip.)
//
// The two rules of mbx_agc.hip shape the launch.  REPLAY: a captured graph that holds one call must advance the state once per replay,
// so nothing about the state is decided on the host -- the kernel reads the record of the last frame and writes the record of this one
// IN PLACE.  OWNERSHIP: no wave reads a record another wave writes -- a bus (its T rows) belongs to 16 lanes of ONE wave, which all load
// its record, and lane 0 of them stores it once, behind the last row.
//
// bus_limit_kernel<form>.  The lane map is that of pcm_agc_kernel: 16 LANES PER ROW of TEN SAMPLES each, 4 buses per 64-lane wave.  The
// input is int32, so a lane's ten samples are 40 bytes at its 40-byte offset (8-byte aligned) and a wave reads 2,560 contiguous bytes;
// it writes 20 bytes (int16) or 10 bytes (G.711) at the same pitch.  TWO reductions over the 16 lanes, which are a DPP row (quad_perm,
// quad_perm, row_half_mirror, row_mirror; no LDS): the peak P as a maximum, and n* as a minimum of lane * 10 + i over the samples above
// thr0.  Both are ready at once, because thr0 depends on the record alone, not on the peak.  Two unsigned divisions per row (thr0 and
// need), computed identically in all 16 lanes.  Each lane then scales its ten samples under g(n) and stores them; the group steps to row
// t + 1 of its bus with the gain and the hold counter in registers, the next row's sums already requested.  Buses beyond n load and
// store nothing and still walk the reductions (T is uniform), so that no lane reads a lane that has left.  Plain loads and stores, no
// LDS, no atomics, no scratch.
#include <new>
#include <vector>

#include "mbx_host.h"
#include "mbx_kernels.h"
#include <mbx_limit.h>     // the public header: include/, first on the include path
#include "mbx_limit_plan.h"
#include "mbx_mixdown_plan.h"   // (mixdown_by_form: the kernel instance of a form)

namespace mbx {

static_assert(sizeof(mbx_limit) == 8 && offsetof(mbx_limit, ceiling) == 0 && offsetof(mbx_limit, release_q8) == 2 && offsetof(mbx_limit, hold_frames) == 3
                  && offsetof(mbx_limit, ramp_log2) == 4 && offsetof(mbx_limit, zero) == 5,
              "the limit is 8 bytes");
static_assert(sizeof(mbx_limit_record) == 4 && offsetof(mbx_limit_record, gain_q15) == 0 && offsetof(mbx_limit_record, hold_left) == 2,
              "a state record is one little-endian word: gain_q15, hold_left (limit_word)");
static_assert(MBX_LIMIT_UNITY_Q15 == kLimitUnity && MBX_LIMIT_MIN_CEILING == kLimitMinCeiling && MBX_LIMIT_MAX_CEILING == kLimitMaxCeiling
                  && MBX_LIMIT_RANGE_LOG2 == kLimitRangeLog2 && MBX_LIMIT_MAX_RAMP_LOG2 == kLimitMaxRampLog2,
              "one set of limits, in the public header and in mbx_limit_plan.h");
static_assert(kLimitLanes * kLimitSamples == 160 && kLimitSamples % 2 == 0 && 64 % kLimitLanes == 0 && kLimitBlock % 64 == 0, "the lane map");

// A lane's share of a row of sums: ten int32 at the lane's 40-byte offset (8-byte aligned, no more) ...
struct alignas(8) LimitShare {
    int32_t s[kLimitSamples];
};
// ... and of a row out: ten int16 at its 20-byte offset, or ten bytes at its 10-byte offset
struct alignas(4) LimitOut16 {
    uint32_t w[kLimitSamples / 2];
};
struct alignas(2) LimitOut8 {
    uint16_t h[kLimitSamples / 2];
};

// the value of lane `lane ^ m` of the 16 lanes of a bus, m = 1, 2, 4, 8 (lowest first: mbx_agc.hip says why)
template <int kXor>
__device__ __forceinline__ uint32_t limit_row_xor(uint32_t v) {
    constexpr int kCtrl = kXor == 1 ? 0xB1 /* quad_perm [1,0,3,2] */ : kXor == 2 ? 0x4E /* quad_perm [2,3,0,1] */
                        : kXor == 4 ? 0x141 /* row_half_mirror */ : 0x140 /* row_mirror */;
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, false);
}
// one step of both reductions: the peak as a maximum, n* as a minimum
template <int kXor>
__device__ __forceinline__ void limit_merge_row(uint32_t& peak, uint32_t& first) {
    const uint32_t p = limit_row_xor<kXor>(peak), f = limit_row_xor<kXor>(first);
    peak = p > peak ? p : peak;
    first = f < first ? f : first;
}

// sums: n * T rows of 160 int32, bus-major (16-byte aligned); out: as many rows of int16 or of bytes; state: the records of the n buses, in place
template <int kOut>
__global__ void __launch_bounds__(kLimitBlock)
bus_limit_kernel(LimitParams p, uint32_t* state, int n, int T, const int32_t* __restrict__ sums, void* __restrict__ out) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t bus = g / kLimitLanes;
    const int j = (int)(g % kLimitLanes);
    const bool live = bus < (size_t)n;
    uint32_t gain = (uint32_t)kLimitUnity, hold = 0;
    if (live) {
        const uint32_t word = state[bus];
        gain = limit_word_gain(word), hold = limit_word_hold(word);
    }
    const size_t at = bus * (size_t)T * 160u + (size_t)(j * kLimitSamples);   // this lane's samples of row 0 of its bus
    LimitShare next = {};
    if (live) {
        next = *reinterpret_cast<const LimitShare*>(sums + at);
    }
    for (int t = 0; t < T; ++t) {
        LimitShare mine = next;
        if (live && t + 1 < T) {   // the next row's sums, requested in front of this row's work
            next = *reinterpret_cast<const LimitShare*>(sums + at + (size_t)(t + 1) * 160u);
        }
        const uint32_t thr0 = limit_threshold(p.ceiling, gain);
        uint32_t peak = 0, first = 160u;
#pragma unroll
        for (int i = kLimitSamples - 1; i >= 0; --i) {   // (downwards: the last one to set `first` is the lane's earliest)
            mine.s[i] = limit_clamped(mine.s[i]);
            const uint32_t a = limit_magnitude(mine.s[i]);
            peak = a > peak ? a : peak;
            first = a > thr0 ? (uint32_t)(j * kLimitSamples + i) : first;
        }
        limit_merge_row<1>(peak, first);
        limit_merge_row<2>(peak, first);
        limit_merge_row<4>(peak, first);
        limit_merge_row<8>(peak, first);
        const LimitDecision d = limit_decide(peak, first, gain, hold, p);
        const LimitRamp ramp = limit_ramp(first < 160u, (int32_t)gain, (int32_t)d.gain, (int)first);
        const auto y = [&](int i) { return limit_scaled(mine.s[i], limit_gain_at(ramp, j * kLimitSamples + i, p.ramp_log2)); };
        const size_t to = at + (size_t)t * 160u;
        if constexpr (kOut == kMixdownPcm16) {
            LimitOut16 o;
#pragma unroll
            for (int i = 0; i < kLimitSamples / 2; ++i) {
                o.w[i] = (uint32_t)(uint16_t)y(2 * i) | ((uint32_t)(uint16_t)y(2 * i + 1) << 16);
            }
            if (live) {
                *reinterpret_cast<LimitOut16*>(static_cast<int16_t*>(out) + to) = o;
            }
        } else {
            LimitOut8 o;
#pragma unroll
            for (int i = 0; i < kLimitSamples / 2; ++i) {
                o.h[i] = (uint16_t)((uint32_t)limit_byte(kOut, y(2 * i)) | ((uint32_t)limit_byte(kOut, y(2 * i + 1)) << 8));
            }
            if (live) {
                *reinterpret_cast<LimitOut8*>(static_cast<uint8_t*>(out) + to) = o;
            }
        }
        gain = d.gain, hold = d.hold;
    }
    if (live && j == 0) {
        state[bus] = limit_word(gain, hold);
    }
}
template __global__ void bus_limit_kernel<kMixdownPcm16>(LimitParams, uint32_t*, int, int, const int32_t*, void*);
template __global__ void bus_limit_kernel<kMixdownUlaw>(LimitParams, uint32_t*, int, int, const int32_t*, void*);
template __global__ void bus_limit_kernel<kMixdownAlaw>(LimitParams, uint32_t*, int, int, const int32_t*, void*);

}  // namespace mbx

namespace {

using mbx::refuse;

int refuse(const char* who, mbx::LimitRefusal why) {
    if (why == mbx::kLimitAlign) {
        return mbx::misaligned(who, "mbx_limit.h");
    }
    return refuse(who, mbx::limit_refusal_text(why));
}

unsigned zero_of(const mbx_limit& l) { return (unsigned)l.zero[0] | (unsigned)l.zero[1] | (unsigned)l.zero[2]; }

mbx::LimitParams params_of(const mbx_limit& l) { return mbx::LimitParams{l.ceiling, l.release_q8, l.hold_frames, (int)l.ramp_log2}; }

// what limit_records_refused says of n records a caller gave
mbx::LimitRefusal records_refused(const mbx_limit_record* r, size_t n) {
    std::vector<uint32_t> words(n);
    for (size_t k = 0; k < n; ++k) {
        words[k] = mbx::limit_word(r[k].gain_q15, r[k].hold_left);
    }
    return mbx::limit_records_refused(words.data(), words.size());
}

// the range of a state call, and the host memory behind it
mbx::LimitRefusal range_refused(const mbx_limit_state* st, int first, int count, const void* host, bool needs_host) {
    const mbx::LimitRefusal why = mbx::limit_range_refused(st != nullptr, st ? st->buses : 0, first, count);
    return why == mbx::kLimitOk && needs_host && !host && count > 0 ? mbx::kLimitNoHost : why;
}

}  // namespace

extern "C" {

int mbx_limit_state_create(mbx_limit_state** out, int buses) {
    const char* const who = "mbx_limit_state_create";
    if (!out) {
        return refuse(who, "no place for the handle");
    }
    *out = nullptr;
    if (buses < 0) {
        return refuse(who, mbx::kLimitCounts);
    }
    int dev = -1;
    const int rc = mbx::ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    mbx_limit_state* st = new (std::nothrow) mbx_limit_state();
    if (!st) {
        return refuse(who, "out of memory");
    }
    st->device = dev;
    st->buses = buses;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&st->d_state), mbx::limit_alloc_bytes(buses));
    if (e == hipSuccess) {   // (the records; the scratch is written before it is read)
        e = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(st->d_state), (int)mbx::kLimitFreshWord, mbx::limit_records_room(buses) / 4u);
    }
    if (e == hipSuccess) {   // (the fill is on the null stream, and the launches that read it may be on a non-blocking one)
        e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) {
        (void)hipFree(st->d_state);
        delete st;
        return mbx::hip_failed("", "mbx_limit_state_create: the records", e);
    }
    st->d_sums = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(st->d_state) + mbx::limit_records_room(buses));
    *out = st;
    return 0;
}

int mbx_limit_state_destroy(mbx_limit_state* st) {
    if (st) {
        (void)hipFree(st->d_state);
        (void)hipGetLastError();
        delete st;
    }
    return 0;
}

int mbx_limit_state_buses(const mbx_limit_state* st) { return st ? st->buses : MBE_STATUS_INVALID_ARGUMENT; }

int32_t* mbx_limit_state_sums(const mbx_limit_state* st) { return st ? st->d_sums : nullptr; }

int mbx_limit_state_reset(mbx_limit_state* st, int first, int count, void* stream) {
    const mbx::LimitRefusal why = range_refused(st, first, count, nullptr, false);
    if (why != mbx::kLimitOk) {
        return refuse("mbx_limit_state_reset", why);
    }
    if (count == 0) {
        return 0;
    }
    const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(st->d_state + first), (int)mbx::kLimitFreshWord, (size_t)count, (hipStream_t)stream);
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_limit_state_reset: hipMemsetD32Async", e);
}

int mbx_limit_state_get(const mbx_limit_state* st, int first, int count, mbx_limit_record* host, void* stream) {
    const mbx::LimitRefusal why = range_refused(st, first, count, host, true);
    if (why != mbx::kLimitOk) {
        return refuse("mbx_limit_state_get", why);
    }
    hipError_t e = hipSuccess;
    if (count > 0) {
        e = hipMemcpyAsync(host, st->d_state + first, mbx::limit_state_bytes(count), hipMemcpyDeviceToHost, (hipStream_t)stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize((hipStream_t)stream);
    }
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_limit_state_get: copy of the records", e);
}

int mbx_limit_state_set(mbx_limit_state* st, int first, int count, const mbx_limit_record* host, void* stream) {
    const char* const who = "mbx_limit_state_set";
    const mbx::LimitRefusal why = range_refused(st, first, count, host, true);
    if (why != mbx::kLimitOk) {
        return refuse(who, why);
    }
    if (records_refused(host, (size_t)count) != mbx::kLimitOk) {
        return refuse(who, mbx::kLimitRecord);
    }
    hipError_t e = hipSuccess;
    if (count > 0) {
        e = hipMemcpyAsync(st->d_state + first, host, mbx::limit_state_bytes(count), hipMemcpyHostToDevice, (hipStream_t)stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize((hipStream_t)stream);
    }
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_limit_state_set: copy of the records", e);
}

int mbx_bus_limit_host(const mbx_limit* limit, mbx_limit_record* records, int n, int T, const int32_t* sums, int form, void* out) {
    const char* const who = "mbx_bus_limit_host";
    mbx::LimitRefusal why = mbx::limit_refused(limit != nullptr, limit ? limit->ceiling : 0u, limit ? limit->ramp_log2 : 0u, limit ? zero_of(*limit) : 0u);
    if (why == mbx::kLimitOk) {
        why = mbx::limit_rows_refused(n, T, form, sums, out, false);
    }
    if (why == mbx::kLimitOk && !records && n > 0) {
        why = mbx::kLimitNoState;
    }
    if (why == mbx::kLimitOk) {
        why = records_refused(records, (size_t)n);
    }
    if (why != mbx::kLimitOk) {
        return refuse(who, why);
    }
    const mbx::LimitParams p = params_of(*limit);
    int32_t x[160];
    for (int i = 0; i < n; ++i) {
        uint32_t gain = records[i].gain_q15, hold = records[i].hold_left;
        for (int t = 0; t < T; ++t) {
            const size_t row = ((size_t)i * (size_t)T + (size_t)t) * 160u;
            const uint32_t thr0 = mbx::limit_threshold(p.ceiling, gain);
            uint32_t peak = 0, first = 160u;
            for (int k = 159; k >= 0; --k) {
                x[k] = mbx::limit_clamped(sums[row + k]);
                const uint32_t a = mbx::limit_magnitude(x[k]);
                peak = a > peak ? a : peak;
                first = a > thr0 ? (uint32_t)k : first;
            }
            const mbx::LimitDecision d = mbx::limit_decide(peak, first, gain, hold, p);   // THE definition
            const mbx::LimitRamp ramp = mbx::limit_ramp(first < 160u, (int32_t)gain, (int32_t)d.gain, (int)first);
            for (int k = 0; k < 160; ++k) {
                const int16_t y = mbx::limit_scaled(x[k], mbx::limit_gain_at(ramp, k, p.ramp_log2));
                if (form == mbx::kMixdownPcm16) {
                    static_cast<int16_t*>(out)[row + k] = y;
                } else {
                    static_cast<uint8_t*>(out)[row + k] = mbx::limit_byte(form, y);
                }
            }
            gain = d.gain, hold = d.hold;
        }
        records[i] = mbx_limit_record{(uint16_t)gain, (uint16_t)hold};
    }
    return 0;
}

int mbx_bus_limit(const mbx_limit* limit, mbx_limit_state* state, int n, int T, const int32_t* d_sums, int form, void* d_out, void* stream) {
    const char* const who = "mbx_bus_limit";
    const mbx::LimitRefusal why = mbx::limit_launch_refused(limit != nullptr, limit ? limit->ceiling : 0u, limit ? limit->ramp_log2 : 0u,
                                                            limit ? zero_of(*limit) : 0u, state != nullptr, state ? state->buses : 0, n, T, form, d_sums, d_out);
    if (why != mbx::kLimitOk) {
        return refuse(who, why);
    }
    if (n == 0 || T == 0) {
        return 0;
    }
    int dev = -1;
    const int rc = mbx::ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    if (state->device != dev) {
        return refuse(who, "a state of another device than the current one");
    }
    const dim3 grid(mbx::limit_grid((size_t)n)), block(mbx::kLimitBlock);
    const mbx::LimitParams p = params_of(*limit);
    mbx::mixdown_by_form(form, [&](auto k) {
        hipLaunchKernelGGL(mbx::bus_limit_kernel<k()>, grid, block, 0, (hipStream_t)stream, p, state->d_state, n, T, d_sums, d_out);
    });
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", "bus_limit_kernel", e);
}

}  // extern "C"
