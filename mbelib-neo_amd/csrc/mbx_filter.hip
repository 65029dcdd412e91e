// mbx_filter.hip -- filtered rows (include/mbx_filter.h): a per-stream cascade of 1 .. 4 second-order sections over the int16 rows a step
// wrote, in ONE launch behind the step and in front of the gain, with one 32-byte state record per stream kept on the device between
// calls.  The arithmetic and the checks are mbx_filter_plan.h, host-only and shared with the host definition below.
//
// The two rules of mbx_agc.hip shape the launch.  REPLAY: a captured graph that holds one call must advance the state once per replay,
// so the filter travels BY VALUE in the kernel arguments (20 int16: there is no filter object on the device) and nothing about the
// state is decided on the host -- the kernel reads the record of the last frame and writes the record of this one IN PLACE.
// OWNERSHIP: no wave reads a record another wave writes -- an entry (a stream's T rows) belongs to ONE LANE, which loads its record as
// two 16-byte pieces and stores it as two, once, behind the last row.
//
// pcm_filter_kernel<S>.  The recurrence is serial over the 160 T samples of an entry and over the sections, and the saved fraction and
// the clamp make it non-associative: no scan is bit-exact.  The parallelism is the entries: A LANE PER ENTRY, a workgroup of one wave
// and 64 entries, S a template parameter so that the chain's state (2 + 3 S values) lives in registers under static indices.
//   IN.   The rows of frame t of the 64 entries are 1,280 16-byte pieces (320 bytes a row, contiguous where T = 1): 60 lanes load three
//         whole rows an instruction, 22 a frame, and lay them into LDS with a row stride of 81 dwords.  The pieces of frame t + 1 are
//         requested before the chain of frame t starts and wait in registers.
//   CHAIN. A lane walks its own row dword by dword: two samples in, S sections each, two samples out into the same dword.  With the
//         odd stride the 32 lanes of a half-wave read and write 32 different banks (a stride of 80 would put them on two).
//   OUT.  The same pieces, from LDS, stored as 16-byte pieces lane after lane.  Every row of the frame was read in full before any is
//         stored, and the rows requested ahead are other rows: d_out may be d_in.
// Rows beyond the last are neither loaded nor stored (a pass beyond it repeats the load of the lane's last row, and only the stores are
// conditional: the kernel says why).  An entry whose record index is outside the state runs over a zero record and stores none.
// Plain loads, plain vector stores, no atomics, no scratch.
#include <cstring>
#include <new>
#include <vector>

#include "mbx_host.h"
#include "mbx_kernels.h"
#include <mbx_filter.h>      // the public header: include/, first on the include path
#include "mbx_filter_plan.h"

namespace mbx {

static_assert(sizeof(mbx_filter) == 44 && offsetof(mbx_filter, sections) == 0 && offsetof(mbx_filter, zero) == 1 && offsetof(mbx_filter, sec) == 4
                  && sizeof(mbx_filter_section) == 10,
              "the filter is 44 bytes");
static_assert(sizeof(mbx_filter_record) == 32 && offsetof(mbx_filter_record, x1) == 0 && offsetof(mbx_filter_record, x2) == 2 && offsetof(mbx_filter_record, sec) == 4
                  && sizeof(((mbx_filter_record*)nullptr)->sec[0]) == 6 && offsetof(mbx_filter_record, zero) == 28,
              "a state record is 16 halfwords: x1, x2, (y1, y2, e) x 4, two of pad (filter_half)");
static_assert(MBX_FILTER_MAX_SECTIONS == kFilterMaxSections && MBX_FILTER_UNITY_Q14 == kFilterUnity && MBX_FILTER_COEFF_BOUND == kFilterCoeffBound,
              "one set of limits, in the public header and in mbx_filter_plan.h");
static_assert(sizeof(FilterParams) == 40 && sizeof(FilterCoeffs) == sizeof(mbx_filter_section), "the filter in the kernel arguments: 40 bytes");

constexpr int kFilterRowPieces = 320 / 16;                                            // 16-byte pieces of a row: 20
constexpr int kFilterPassRows = kFilterBlock / kFilterRowPieces;                        // rows the wave moves an instruction: 3
constexpr int kFilterPasses = (kFilterBlock + kFilterPassRows - 1) / kFilterPassRows;   // ... and instructions a frame: 22
constexpr int kFilterLdsRows = kFilterPassRows * kFilterPasses;                         // rows the passes cover: 66

// in, out: n * T rows, stream-major (16-byte aligned; out may be in); state: `streams` records of eight words, in place; d_stream: n
// entries or nullptr
template <int S>
__global__ void __launch_bounds__(kFilterBlock)
pcm_filter_kernel(FilterParams f, uint32_t* state, int streams, const int32_t* __restrict__ d_stream, int n, int T, const int16_t* in, int16_t* out) {
    __shared__ uint32_t lds[kFilterLdsRows * kFilterRowStride];   // 21,384 bytes: the rows of one frame of the 64 entries, and two the passes run over
    const uint32_t tid = threadIdx.x;
    const size_t entry0 = (size_t)blockIdx.x * kFilterBlock;                                              // (below n: the grid is no larger)
    const uint32_t live = (size_t)n - entry0 < (size_t)kFilterBlock ? (uint32_t)((size_t)n - entry0) : (uint32_t)kFilterBlock;   // entries of this workgroup
    const bool mine = tid < live;
    int32_t record = -1;
    if (mine) {
        record = d_stream ? d_stream[entry0 + tid] : (int32_t)(entry0 + tid);
    }
    const bool owns = mine && record >= 0 && record < streams;   // (an entry outside the state: a zero record, none stored)
    uint32_t w[kFilterRecordWords] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint4* const rec = reinterpret_cast<uint4*>(state) + (size_t)(owns ? record : 0) * 2u;
    if (owns) {
        const uint4 a = rec[0], b = rec[1];
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
    }
    int32_t x1 = filter_sext(filter_half(w, 0)), x2 = filter_sext(filter_half(w, 1));
    int32_t y1[kFilterMaxSections], y2[kFilterMaxSections];
    uint32_t e[kFilterMaxSections];
#pragma unroll
    for (int s = 0; s < kFilterMaxSections; ++s) {
        y1[s] = filter_sext(filter_half(w, 2 + 3 * s)), y2[s] = filter_sext(filter_half(w, 3 + 3 * s)), e[s] = filter_half(w, 4 + 3 * s);
    }
    // the pieces of a frame: lane 20 q + p (q = 0 .. 2) moves piece p of rows q, q + 3, q + 6 ... of the workgroup, 22 passes: from pass
    // to pass a lane's address moves by a uniform stride in memory and by a constant in LDS.  Loads and LDS writes are UNCONDITIONAL (no
    // branch between them, so that the 22 loads are in flight together): a pass beyond the lane's last row repeats the load of its last
    // row and lays it into one of the LDS rows 64, 65 or into a row beyond `live`, which nobody reads; the four lanes left over, and the
    // lanes of a row the workgroup does not have, repeat what a mover does.  Only the stores are conditional.
    const uint4* const in4 = reinterpret_cast<const uint4*>(in);
    uint4* const out4 = reinterpret_cast<uint4*>(out);
    const uint32_t top = live - 1u;   // the last row of the workgroup
    const uint32_t tq = tid / kFilterRowPieces, p = tid % kFilterRowPieces;
    const uint32_t within = tq < (uint32_t)kFilterPassRows ? tq : (uint32_t)kFilterPassRows - 1u;
    const uint32_t q = within < top ? within : top;   // the lane's first row: min(tq, 2, top)
    const bool mover = tq == q;                       // (the others repeat a mover's loads and LDS writes, value for value)
    const uint32_t last_pass = (top - q) / (uint32_t)kFilterPassRows;           // the last pass that finds a row of this lane
    const size_t piece0 = (entry0 + q) * (size_t)T * kFilterRowPieces + p;      // piece p of row q of the workgroup, frame 0
    const size_t pass = (size_t)kFilterPassRows * (size_t)T * kFilterRowPieces;   // ... and of row q + 3: so many pieces on
    uint32_t* const lane_lds = lds + q * kFilterRowStride + p * 4u;
    uint4 next[kFilterPasses];
#pragma unroll
    for (int k = 0; k < kFilterPasses; ++k) {
        next[k] = in4[piece0 + pass * ((uint32_t)k < last_pass ? (uint32_t)k : last_pass)];
    }
    uint32_t* const row = lds + tid * kFilterRowStride;
    for (int t = 0; t < T; ++t) {
        const size_t frame = piece0 + (size_t)t * kFilterRowPieces;
        // ---- in ----
#pragma unroll
        for (int k = 0; k < kFilterPasses; ++k) {
            uint32_t* const at = lane_lds + kFilterPassRows * kFilterRowStride * k;
            at[0] = next[k].x, at[1] = next[k].y, at[2] = next[k].z, at[3] = next[k].w;
        }
        if (t + 1 < T) {   // the next frame's rows, requested in front of this frame's chain
#pragma unroll
            for (int k = 0; k < kFilterPasses; ++k) {
                next[k] = in4[frame + kFilterRowPieces + pass * ((uint32_t)k < last_pass ? (uint32_t)k : last_pass)];
            }
        }
        __syncthreads();
        // ---- chain ----
        if (mine) {
#pragma unroll 4
            for (int k = 0; k < kFilterRowWords; ++k) {
                const uint32_t two = row[k];
                const int32_t lo = filter_chain<S>(f, filter_sext(two & 0xFFFFu), x1, x2, y1, y2, e);
                const int32_t hi = filter_chain<S>(f, filter_sext(two >> 16), x1, x2, y1, y2, e);
                row[k] = ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
            }
        }
        __syncthreads();
        // ---- out ----
#pragma unroll
        for (int k = 0; k < kFilterPasses; ++k) {
            if (mover && (uint32_t)k <= last_pass) {
                const uint32_t* const at = lane_lds + kFilterPassRows * kFilterRowStride * k;
                out4[frame + pass * k] = uint4{at[0], at[1], at[2], at[3]};
            }
        }
        __syncthreads();   // (the rows have left LDS before the next frame's are laid over them)
    }
    if (owns) {   // the record behind the last row: what the S sections moved, the rest as it was read
        const auto half = [](int32_t v) { return (uint32_t)v & 0xFFFFu; };
        uint32_t h[2 * kFilterRecordWords];
#pragma unroll
        for (int k = 0; k < 2 * kFilterRecordWords; ++k) {
            h[k] = filter_half(w, k);
        }
        h[0] = half(x1), h[1] = half(x2);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            h[2 + 3 * s] = half(y1[s]), h[3 + 3 * s] = half(y2[s]), h[4 + 3 * s] = e[s];
        }
        rec[0] = uint4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
        rec[1] = uint4{h[8] | (h[9] << 16), h[10] | (h[11] << 16), h[12] | (h[13] << 16), h[14] | (h[15] << 16)};
    }
}
template __global__ void pcm_filter_kernel<1>(FilterParams, uint32_t*, int, const int32_t*, int, int, const int16_t*, int16_t*);
template __global__ void pcm_filter_kernel<2>(FilterParams, uint32_t*, int, const int32_t*, int, int, const int16_t*, int16_t*);
template __global__ void pcm_filter_kernel<3>(FilterParams, uint32_t*, int, const int32_t*, int, int, const int16_t*, int16_t*);
template __global__ void pcm_filter_kernel<4>(FilterParams, uint32_t*, int, const int32_t*, int, int, const int16_t*, int16_t*);

}  // namespace mbx

namespace {

using mbx::refuse;

int refuse(const char* who, mbx::FilterRefusal why) {
    if (why == mbx::kFilterAlign) {
        return mbx::misaligned(who, "mbx_filter.h");
    }
    return refuse(who, mbx::filter_refusal_text(why));
}

unsigned zero_of(const mbx_filter* f) { return f ? (unsigned)(f->zero[0] | f->zero[1] | f->zero[2]) : 0u; }
const int16_t* coeffs_of(const mbx_filter* f) { return f ? &f->sec[0].b0 : nullptr; }   // (the 20 int16 of sec[4], no padding between them)

mbx::FilterRefusal params_refused(const mbx_filter* f) { return mbx::filter_refused(f != nullptr, f ? f->sections : 0u, zero_of(f), coeffs_of(f)); }

mbx::FilterParams params_of(const mbx_filter& f) {
    mbx::FilterParams p;
    for (int s = 0; s < mbx::kFilterMaxSections; ++s) {
        p.sec[s] = mbx::FilterCoeffs{f.sec[s].b0, f.sec[s].b1, f.sec[s].b2, f.sec[s].a1, f.sec[s].a2};
    }
    return p;
}

// what filter_records_refused says of n records a caller gave
mbx::FilterRefusal records_refused(const mbx_filter_record* r, size_t n) {
    std::vector<uint32_t> words(n * (size_t)mbx::kFilterRecordWords);
    if (n) {
        std::memcpy(words.data(), r, n * sizeof(mbx_filter_record));
    }
    return mbx::filter_records_refused(words.data(), n);
}

// the range of a state call, and the host memory behind it
mbx::FilterRefusal range_refused(const mbx_filter_state* st, int first, int count, const void* host, bool needs_host) {
    const mbx::FilterRefusal why = mbx::filter_range_refused(st != nullptr, st ? st->streams : 0, first, count);
    return why == mbx::kFilterOk && needs_host && !host && count > 0 ? mbx::kFilterNoHost : why;
}

// THE definition: the T rows of every entry through S sections, sample by sample
template <int S>
void host_rows(const mbx::FilterParams& f, mbx_filter_record* state, int streams, const int32_t* stream_index, int n, int T, const int16_t* in, int16_t* out) {
    for (int i = 0; i < n; ++i) {
        const int64_t record = stream_index ? (int64_t)stream_index[i] : (int64_t)i;
        const bool owns = record >= 0 && record < streams;
        mbx_filter_record r;
        std::memset(&r, 0, sizeof r);   // (an entry outside the state: a zero record, none stored)
        if (owns) {
            r = state[record];
        }
        int32_t x1 = r.x1, x2 = r.x2, y1[mbx::kFilterMaxSections], y2[mbx::kFilterMaxSections];
        uint32_t e[mbx::kFilterMaxSections];
        for (int s = 0; s < mbx::kFilterMaxSections; ++s) {
            y1[s] = r.sec[s].y1, y2[s] = r.sec[s].y2, e[s] = r.sec[s].e;
        }
        const size_t first = (size_t)i * (size_t)T * 160u;
        for (size_t k = 0; k < (size_t)T * 160u; ++k) {   // (a sample is read before it is written: out may be in)
            out[first + k] = (int16_t)mbx::filter_chain<S>(f, in[first + k], x1, x2, y1, y2, e);
        }
        if (owns && T > 0) {
            r.x1 = (int16_t)x1, r.x2 = (int16_t)x2;
            for (int s = 0; s < S; ++s) {
                r.sec[s].y1 = (int16_t)y1[s], r.sec[s].y2 = (int16_t)y2[s], r.sec[s].e = (uint16_t)e[s];
            }
            state[record] = r;
        }
    }
}

}  // namespace

extern "C" {

int mbx_filter_state_create(mbx_filter_state** out, int streams) {
    const char* const who = "mbx_filter_state_create";
    if (!out) {
        return refuse(who, "no place for the handle");
    }
    *out = nullptr;
    if (streams < 0) {
        return refuse(who, mbx::kFilterCounts);
    }
    int dev = -1;
    const int rc = mbx::ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    mbx_filter_state* st = new (std::nothrow) mbx_filter_state();
    if (!st) {
        return refuse(who, "out of memory");
    }
    st->device = dev;
    st->streams = streams;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&st->d_state), mbx::filter_alloc_bytes(streams));
    if (e == hipSuccess) {
        e = hipMemset(st->d_state, 0, mbx::filter_alloc_bytes(streams));
    }
    if (e == hipSuccess) {   // (the fill is on the null stream, and the launches that read it may be on a non-blocking one)
        e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) {
        (void)hipFree(st->d_state);
        delete st;
        return mbx::hip_failed("", "mbx_filter_state_create: the records", e);
    }
    *out = st;
    return 0;
}

int mbx_filter_state_destroy(mbx_filter_state* st) {
    if (st) {
        (void)hipFree(st->d_state);
        (void)hipGetLastError();
        delete st;
    }
    return 0;
}

int mbx_filter_state_streams(const mbx_filter_state* st) { return st ? st->streams : MBE_STATUS_INVALID_ARGUMENT; }

int mbx_filter_state_reset(mbx_filter_state* st, int first, int count, void* stream) {
    const mbx::FilterRefusal why = range_refused(st, first, count, nullptr, false);
    if (why != mbx::kFilterOk) {
        return refuse("mbx_filter_state_reset", why);
    }
    if (count == 0) {
        return 0;
    }
    const hipError_t e = hipMemsetAsync(st->d_state + (size_t)first * mbx::kFilterRecordWords, 0, mbx::filter_state_bytes(count), (hipStream_t)stream);
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_filter_state_reset: hipMemsetAsync", e);
}

int mbx_filter_state_get(const mbx_filter_state* st, int first, int count, mbx_filter_record* host, void* stream) {
    const mbx::FilterRefusal why = range_refused(st, first, count, host, true);
    if (why != mbx::kFilterOk) {
        return refuse("mbx_filter_state_get", why);
    }
    hipError_t e = hipSuccess;
    if (count > 0) {
        e = hipMemcpyAsync(host, st->d_state + (size_t)first * mbx::kFilterRecordWords, mbx::filter_state_bytes(count), hipMemcpyDeviceToHost,
                           (hipStream_t)stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize((hipStream_t)stream);
    }
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_filter_state_get: copy of the records", e);
}

int mbx_filter_state_set(mbx_filter_state* st, int first, int count, const mbx_filter_record* host, void* stream) {
    const char* const who = "mbx_filter_state_set";
    const mbx::FilterRefusal why = range_refused(st, first, count, host, true);
    if (why != mbx::kFilterOk) {
        return refuse(who, why);
    }
    if (records_refused(host, (size_t)count) != mbx::kFilterOk) {
        return refuse(who, mbx::kFilterRecord);
    }
    hipError_t e = hipSuccess;
    if (count > 0) {
        e = hipMemcpyAsync(st->d_state + (size_t)first * mbx::kFilterRecordWords, host, mbx::filter_state_bytes(count), hipMemcpyHostToDevice,
                           (hipStream_t)stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize((hipStream_t)stream);
    }
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_filter_state_set: copy of the records", e);
}

int mbx_pcm_filter_host(const mbx_filter* filter, mbx_filter_record* state, int streams, const int32_t* stream_index, int n, int T, const int16_t* in,
                        int16_t* out) {
    const char* const who = "mbx_pcm_filter_host";
    mbx::FilterRefusal why = params_refused(filter);
    if (why == mbx::kFilterOk) {
        why = streams < 0 ? mbx::kFilterCounts : (!state && streams > 0) ? mbx::kFilterNoState : mbx::filter_rows_refused(n, T, in, out, 0u);
    }
    if (why == mbx::kFilterOk) {
        why = records_refused(state, (size_t)streams);
    }
    if (why != mbx::kFilterOk) {
        return refuse(who, why);
    }
    const mbx::FilterParams f = params_of(*filter);
    switch (filter->sections) {
    case 1: host_rows<1>(f, state, streams, stream_index, n, T, in, out); break;
    case 2: host_rows<2>(f, state, streams, stream_index, n, T, in, out); break;
    case 3: host_rows<3>(f, state, streams, stream_index, n, T, in, out); break;
    default: host_rows<4>(f, state, streams, stream_index, n, T, in, out); break;   // (filter_refused: nothing else is left)
    }
    return 0;
}

int mbx_pcm_filter(const mbx_filter* filter, mbx_filter_state* state, const int32_t* d_stream, int n, int T, const int16_t* d_in, int16_t* d_out,
                   void* stream) {
    const char* const who = "mbx_pcm_filter";
    const mbx::FilterRefusal why = mbx::filter_launch_refused(filter != nullptr, filter ? filter->sections : 0u, zero_of(filter), coeffs_of(filter),
                                                              state != nullptr, n, T, d_in, d_out);
    if (why != mbx::kFilterOk) {
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
    const dim3 grid(mbx::filter_grid((size_t)n)), block(mbx::kFilterBlock);
    const mbx::FilterParams f = params_of(*filter);
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, f, state->d_state, state->streams, d_stream, n, T, d_in, d_out);
    };
    switch (filter->sections) {
    case 1: launch(mbx::pcm_filter_kernel<1>); break;
    case 2: launch(mbx::pcm_filter_kernel<2>); break;
    case 3: launch(mbx::pcm_filter_kernel<3>); break;
    default: launch(mbx::pcm_filter_kernel<4>); break;   // (filter_refused: nothing else is left)
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", "pcm_filter_kernel", e);
}

}  // extern "C"
