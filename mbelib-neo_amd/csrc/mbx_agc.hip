// mbx_agc.hip -- levelled rows (include/mbx_agc.h): a per-stream automatic gain control over the int16 rows a step wrote, in ONE launch
// behind the step, with one 4-byte state record per stream kept on the device between calls.  The arithmetic and the checks are
// mbx_agc_plan.h, host-only and shared with the host definition below.
//
// Two rules shape the launch, as they shape mbx_hold.hip.  REPLAY: a captured graph that holds one call must advance the state once per
// replay, so nothing about the state is decided on the host -- the kernel reads the record of the last frame and writes the record of
// this one IN PLACE.  OWNERSHIP: no wave reads a record another wave writes -- an entry (a stream's T rows) belongs to 16 lanes of ONE
// wave, which all load its record, and lane 0 of them stores it once, behind the last row.
//
// pcm_agc_kernel.  The lane map is that of pcm_levels_kernel (mbx_levels.hip): 16 LANES PER ROW of TEN SAMPLES each, 4 entries per
// 64-lane wave; ten samples are five dwords at the lane's 20-byte offset (one 16-byte and one 4-byte access, 4-byte aligned, a wave
// moving 1,280 contiguous bytes each way); the peak of the row is a maximum over the 16 lanes, which are a DPP row: four
// v_max_u32_dpp-style steps (quad_perm, quad_perm, row_half_mirror, row_mirror), no LDS.  After the reduction all 16 lanes hold the
// peak and take the same decision (agc_decide: one unsigned division per row), each scales its ten samples under g(n) and stores
// them; then the group steps to row t + 1 of its entry with the gain in registers, the next row's samples already requested.  A lane
// reads all its samples of a row before it stores any, so d_out may be d_in.  Entries beyond n load and store nothing and still walk
// the reduction (T is uniform), so that no lane reads a lane that has left.  An entry whose record index is outside the state is
// passed through at unity, frozen, and stores no record.  Plain loads and stores, no LDS, no atomics, no scratch.
#include <new>
#include <vector>

#include "mbx_host.h"
#include "mbx_kernels.h"
#include <mbx_agc.h>       // the public header: include/, first on the include path
#include "mbx_agc_plan.h"

namespace mbx {

static_assert(sizeof(mbx_agc) == 12 && offsetof(mbx_agc, target_peak) == 0 && offsetof(mbx_agc, floor_peak) == 2 && offsetof(mbx_agc, min_gain_q10) == 4
                  && offsetof(mbx_agc, max_gain_q10) == 6 && offsetof(mbx_agc, release_q8) == 8 && offsetof(mbx_agc, rise_q8) == 9
                  && offsetof(mbx_agc, ramp_log2) == 10 && offsetof(mbx_agc, zero) == 11,
              "the agc is 12 bytes");
static_assert(sizeof(mbx_agc_record) == 4 && offsetof(mbx_agc_record, gain_q10) == 0 && offsetof(mbx_agc_record, env) == 2,
              "a state record is one little-endian word: gain_q10, env (agc_word)");
static_assert(MBX_AGC_UNITY_Q10 == kAgcUnity && MBX_AGC_MAX_GAIN_Q10 == kAgcMaxGain && MBX_AGC_MAX_RAMP_LOG2 == kAgcMaxRampLog2,
              "one set of limits, in the public header and in mbx_agc_plan.h");
static_assert(kAgcLanes * kAgcSamples == 160 && kAgcSamples % 2 == 0 && 64 % kAgcLanes == 0 && kAgcBlock % 64 == 0, "the lane map");

// A lane's share of a row: ten samples, five dwords at the lane's 20-byte offset (4-byte aligned, no more)
struct alignas(4) AgcShare {
    uint32_t w[kAgcSamples / 2];
};
typedef unsigned short agc_u16x2 __attribute__((ext_vector_type(2)));
typedef short          agc_i16x2 __attribute__((ext_vector_type(2)));

// |x| of the two samples of a dword, both halves at once: s = x >> 15 (0 or -1), (x ^ s) - s as uint16 is |x|, 32768 for -32768
__device__ __forceinline__ agc_u16x2 agc_abs_pair(uint32_t w) {
    const agc_i16x2 x = __builtin_bit_cast(agc_i16x2, w);
    const agc_i16x2 s = x >> (agc_i16x2){15, 15};
    return __builtin_bit_cast(agc_u16x2, (agc_i16x2)(x ^ s)) - __builtin_bit_cast(agc_u16x2, s);
}

// the value of lane `lane ^ m` of the 16 lanes of an entry, m = 1, 2, 4, 8 (lowest first: once the lanes that differ in the lower bits
// hold equal values, the mirrors of 8 and of 16 lanes reach a lane that holds what lane ^ m holds)
template <int kXor>
__device__ __forceinline__ uint32_t agc_row_xor(uint32_t v) {
    constexpr int kCtrl = kXor == 1 ? 0xB1 /* quad_perm [1,0,3,2] */ : kXor == 2 ? 0x4E /* quad_perm [2,3,0,1] */
                        : kXor == 4 ? 0x141 /* row_half_mirror */ : 0x140 /* row_mirror */;
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, 0xF, 0xF, false);
}
template <int kXor>
__device__ __forceinline__ uint32_t agc_max_row(uint32_t v) {
    const uint32_t o = agc_row_xor<kXor>(v);
    return o > v ? o : v;
}

// in, out: n * T rows, stream-major (16-byte aligned; out may be in); state: `streams` records, in place; d_stream: n entries or nullptr
__global__ void __launch_bounds__(kAgcBlock)
pcm_agc_kernel(AgcParams a, uint32_t* state, int streams, const int32_t* __restrict__ d_stream, int n, int T, const int16_t* in, int16_t* out) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t entry = g / kAgcLanes;
    const int j = (int)(g % kAgcLanes);
    const bool live = entry < (size_t)n;
    int32_t record = -1;
    if (live) {
        record = d_stream ? d_stream[entry] : (int32_t)entry;
    }
    const bool owns = live && record >= 0 && record < streams;   // (an entry outside the state: passed through, no record touched)
    uint32_t gain = (uint32_t)kAgcUnity, env = 0;
    if (owns) {
        const uint32_t word = state[record];
        gain = agc_word_gain(word), env = agc_word_env(word);
    }
    const size_t at = entry * (size_t)T * 160u + (size_t)(j * kAgcSamples);   // this lane's samples of row 0 of its entry
    AgcShare next = {};
    if (live) {
        next = *reinterpret_cast<const AgcShare*>(in + at);
    }
    for (int t = 0; t < T; ++t) {
        const AgcShare mine = next;
        if (live && t + 1 < T) {   // the next row's samples, requested in front of this row's work
            next = *reinterpret_cast<const AgcShare*>(in + at + (size_t)(t + 1) * 160u);
        }
        agc_u16x2 peak2 = {0, 0};
#pragma unroll
        for (int i = 0; i < kAgcSamples / 2; ++i) {
            peak2 = __builtin_elementwise_max(peak2, agc_abs_pair(mine.w[i]));
        }
        uint32_t p = peak2.x > peak2.y ? peak2.x : peak2.y;
        p = agc_max_row<1>(p);
        p = agc_max_row<2>(p);
        p = agc_max_row<4>(p);
        p = agc_max_row<8>(p);
        AgcDecision d{gain, env, gain, kAgcFreeze};
        if (owns) {
            d = agc_decide(p, gain, env, a);
        }
        AgcShare y;
#pragma unroll
        for (int i = 0; i < kAgcSamples / 2; ++i) {
            const int nn = j * kAgcSamples + 2 * i;
            const int16_t lo = agc_scaled((int16_t)(mine.w[i] & 0xFFFFu), agc_gain_at((int32_t)gain, (int32_t)d.gain, nn, a.ramp_log2));
            const int16_t hi = agc_scaled((int16_t)(mine.w[i] >> 16), agc_gain_at((int32_t)gain, (int32_t)d.gain, nn + 1, a.ramp_log2));
            y.w[i] = (uint32_t)(uint16_t)lo | ((uint32_t)(uint16_t)hi << 16);
        }
        if (live) {
            *reinterpret_cast<AgcShare*>(out + at + (size_t)t * 160u) = y;
        }
        gain = d.gain, env = d.env;
    }
    if (owns && j == 0) {
        state[record] = agc_word(gain, env);
    }
}

}  // namespace mbx

namespace {

using mbx::refuse;

int refuse(const char* who, mbx::AgcRefusal why) {
    if (why == mbx::kAgcAlign) {
        return mbx::misaligned(who, "mbx_agc.h");
    }
    return refuse(who, mbx::agc_refusal_text(why));
}

mbx::AgcRefusal params_refused(const mbx_agc* a) {
    return mbx::agc_refused(a != nullptr, a ? a->target_peak : 0u, a ? a->floor_peak : 0u, a ? a->min_gain_q10 : 0u, a ? a->max_gain_q10 : 0u,
                            a ? a->ramp_log2 : 0u, a ? a->zero : 0u);
}

mbx::AgcParams params_of(const mbx_agc& a) {
    return mbx::AgcParams{a.target_peak, a.floor_peak, a.min_gain_q10, a.max_gain_q10, a.release_q8, a.rise_q8, (int)a.ramp_log2};
}

// what agc_records_refused says of n records a caller gave
mbx::AgcRefusal records_refused(const mbx_agc_record* r, size_t n) {
    std::vector<uint32_t> words(n);
    for (size_t k = 0; k < n; ++k) {
        words[k] = mbx::agc_word(r[k].gain_q10, r[k].env);
    }
    return mbx::agc_records_refused(words.data(), words.size());
}

// the range of a state call, and the host memory behind it
mbx::AgcRefusal range_refused(const mbx_agc_state* st, int first, int count, const void* host, bool needs_host) {
    const mbx::AgcRefusal why = mbx::agc_range_refused(st != nullptr, st ? st->streams : 0, first, count);
    return why == mbx::kAgcOk && needs_host && !host && count > 0 ? mbx::kAgcNoHost : why;
}

}  // namespace

extern "C" {

int mbx_agc_state_create(mbx_agc_state** out, int streams) {
    const char* const who = "mbx_agc_state_create";
    if (!out) {
        return refuse(who, "no place for the handle");
    }
    *out = nullptr;
    if (streams < 0) {
        return refuse(who, mbx::kAgcCounts);
    }
    int dev = -1;
    const int rc = mbx::ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    mbx_agc_state* st = new (std::nothrow) mbx_agc_state();
    if (!st) {
        return refuse(who, "out of memory");
    }
    st->device = dev;
    st->streams = streams;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&st->d_state), mbx::agc_alloc_bytes(streams));
    if (e == hipSuccess) {
        e = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(st->d_state), (int)mbx::kAgcFreshWord, mbx::agc_alloc_bytes(streams) / 4u);
    }
    if (e == hipSuccess) {   // (the fill is on the null stream, and the launches that read it may be on a non-blocking one)
        e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) {
        (void)hipFree(st->d_state);
        delete st;
        return mbx::hip_failed("", "mbx_agc_state_create: the records", e);
    }
    *out = st;
    return 0;
}

int mbx_agc_state_destroy(mbx_agc_state* st) {
    if (st) {
        (void)hipFree(st->d_state);
        (void)hipGetLastError();
        delete st;
    }
    return 0;
}

int mbx_agc_state_streams(const mbx_agc_state* st) { return st ? st->streams : MBE_STATUS_INVALID_ARGUMENT; }

int mbx_agc_state_reset(mbx_agc_state* st, int first, int count, void* stream) {
    const mbx::AgcRefusal why = range_refused(st, first, count, nullptr, false);
    if (why != mbx::kAgcOk) {
        return refuse("mbx_agc_state_reset", why);
    }
    if (count == 0) {
        return 0;
    }
    const hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(st->d_state + first), (int)mbx::kAgcFreshWord, (size_t)count, (hipStream_t)stream);
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_agc_state_reset: hipMemsetD32Async", e);
}

int mbx_agc_state_get(const mbx_agc_state* st, int first, int count, mbx_agc_record* host, void* stream) {
    const mbx::AgcRefusal why = range_refused(st, first, count, host, true);
    if (why != mbx::kAgcOk) {
        return refuse("mbx_agc_state_get", why);
    }
    hipError_t e = hipSuccess;
    if (count > 0) {
        e = hipMemcpyAsync(host, st->d_state + first, mbx::agc_state_bytes(count), hipMemcpyDeviceToHost, (hipStream_t)stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize((hipStream_t)stream);
    }
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_agc_state_get: copy of the records", e);
}

int mbx_agc_state_set(mbx_agc_state* st, int first, int count, const mbx_agc_record* host, void* stream) {
    const char* const who = "mbx_agc_state_set";
    const mbx::AgcRefusal why = range_refused(st, first, count, host, true);
    if (why != mbx::kAgcOk) {
        return refuse(who, why);
    }
    if (records_refused(host, (size_t)count) != mbx::kAgcOk) {
        return refuse(who, mbx::kAgcRecord);
    }
    hipError_t e = hipSuccess;
    if (count > 0) {
        e = hipMemcpyAsync(st->d_state + first, host, mbx::agc_state_bytes(count), hipMemcpyHostToDevice, (hipStream_t)stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize((hipStream_t)stream);
    }
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_agc_state_set: copy of the records", e);
}

int mbx_pcm_agc_host(const mbx_agc* agc, mbx_agc_record* state, int streams, const int32_t* stream_index, int n, int T, const int16_t* in,
                     int16_t* out) {
    const char* const who = "mbx_pcm_agc_host";
    mbx::AgcRefusal why = params_refused(agc);
    if (why == mbx::kAgcOk) {
        why = streams < 0 ? mbx::kAgcCounts : (!state && streams > 0) ? mbx::kAgcNoState : mbx::agc_rows_refused(n, T, in, out, 0u);
    }
    if (why == mbx::kAgcOk) {
        why = records_refused(state, (size_t)streams);
    }
    if (why != mbx::kAgcOk) {
        return refuse(who, why);
    }
    const mbx::AgcParams a = params_of(*agc);
    int16_t x[160];
    for (int i = 0; i < n; ++i) {
        const int64_t record = stream_index ? (int64_t)stream_index[i] : (int64_t)i;
        const bool owns = record >= 0 && record < streams;
        uint32_t gain = owns ? state[record].gain_q10 : (uint32_t)mbx::kAgcUnity, env = owns ? state[record].env : 0u;
        for (int t = 0; t < T; ++t) {
            const size_t row = ((size_t)i * (size_t)T + (size_t)t) * 160u;
            uint32_t p = 0;
            for (int k = 0; k < 160; ++k) {   // (the row read before any of it is written: out may be in)
                x[k] = in[row + k];
                const uint32_t mag = x[k] < 0 ? (uint32_t)(-(int32_t)x[k]) : (uint32_t)x[k];
                p = mag > p ? mag : p;
            }
            // THE definition: an entry outside the state is frozen at unity
            const mbx::AgcDecision d = owns ? mbx::agc_decide(p, gain, env, a) : mbx::AgcDecision{gain, env, gain, mbx::kAgcFreeze};
            for (int k = 0; k < 160; ++k) {
                out[row + k] = mbx::agc_scaled(x[k], mbx::agc_gain_at((int32_t)gain, (int32_t)d.gain, k, a.ramp_log2));
            }
            gain = d.gain, env = d.env;
        }
        if (owns) {
            state[record] = mbx_agc_record{(uint16_t)gain, (uint16_t)env};
        }
    }
    return 0;
}

int mbx_pcm_agc(const mbx_agc* agc, mbx_agc_state* state, const int32_t* d_stream, int n, int T, const int16_t* d_in, int16_t* d_out, void* stream) {
    const char* const who = "mbx_pcm_agc";
    const mbx::AgcRefusal why = mbx::agc_launch_refused(agc != nullptr, agc ? agc->target_peak : 0u, agc ? agc->floor_peak : 0u, agc ? agc->min_gain_q10 : 0u,
                                                        agc ? agc->max_gain_q10 : 0u, agc ? agc->ramp_log2 : 0u, agc ? agc->zero : 0u, state != nullptr, n, T,
                                                        d_in, d_out);
    if (why != mbx::kAgcOk) {
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
    hipLaunchKernelGGL(mbx::pcm_agc_kernel, dim3(mbx::agc_grid((size_t)n)), dim3(mbx::kAgcBlock), 0, (hipStream_t)stream, params_of(*agc), state->d_state,
                       state->streams, d_stream, n, T, d_in, d_out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", "pcm_agc_kernel", e);
}

}  // extern "C"
