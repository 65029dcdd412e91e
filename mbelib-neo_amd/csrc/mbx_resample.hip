// mbx_resample.hip -- wide rows (include/mbx_resample.h): the int16 rows of a step, or the bus rows of a mix-down, upsampled by L = 2, 3,
// 4 or 6 through a polyphase FIR interpolator with the caller's taps, in ONE launch, with one 64-byte history record per row kept on
// the device between calls.  The arithmetic and the checks are mbx_resample_plan.h, host-only and shared with the host definition below.
//
// The two rules of mbx_agc.hip shape the launch.  REPLAY: a captured graph that holds one call must advance the state once per replay,
// so the filter travels BY VALUE in the kernel arguments (96 packed dwords, as burst_gather_groups_kernel takes its descriptors: there
// is no filter object on the device) and nothing about the state is decided on the host -- the kernel reads the record of the last
// frame and writes the record of this one IN PLACE.  OWNERSHIP: no wave reads a record another wave writes -- four lanes of the
// workgroup that holds frame 0 of an entry each load 16 bytes of its record and then store those 16 bytes, fetched from the tail of the
// entry's LAST row in d_in; the lanes of the last row store nothing of it.  d_in is never written by the launch, so the order of the
// rows does not matter.
//
// pcm_resample_kernel<L>.  ROWS, not entries, are mapped to lanes: rows are independent once their history is known, and the history
// of frame t > 0 is the 64 bytes in front of the row in d_in.  A workgroup of 256 lanes takes 16 consecutive rows.
//   IN.   The 16 rows are 5,120 contiguous bytes: 320 16-byte pieces, lane after lane, into the rows' windows in LDS -- x_ext[-32 .. 159]
//         of a row is 96 dwords, 6 KiB a workgroup.  The first 64 lanes also bring the 16 histories, four 16-byte pieces each.
//   SUM.  The lane map of pcm_agc_kernel: 16 LANES PER ROW of TEN INPUT SAMPLES each, 4 rows per 64-lane wave.  Behind one barrier
//         a lane reads its samples and the K - 1 earlier ones from the window.  The sum over the taps runs two taps an instruction
//         (v_dot2_i32_i16, no saturation) in a run-time loop over K / 2: for the pair k = 2 kk a lane holds the six window dwords that
//         cover x_ext[10 j - k - 2 .. 10 j + 9 - k].  An odd sample n finds its pair (x_ext[n - k - 1], x_ext[n - k]) as one of them; an
//         even n finds it across two, REALIGNED IN REGISTERS by one v_alignbit_b32.  From kk to kk + 1 both sets slide by one dword: one
//         LDS read and one realignment per pair of taps, against 10 L dot products.  The L tap dwords of a pair are uniform: scalar
//         loads from the kernel arguments.  10 L accumulators per lane; the outputs are rounded, clamped and packed two a dword
//         (v_cvt_pk_i16_i32 saturates).
//   OUT.  A lane's 10 L outputs are 20 L bytes at a 20 L-byte pitch: stored from the lanes, a wave's store instruction would touch 64
//         cache lines (the first build did, and ran at half the bytes per second of this one: EXPERIMENTS "Wide rows").  So the
//         workgroup's 16 wide rows, 5,120 L contiguous bytes, are laid out in LDS -- over the windows, which nobody reads any more behind
//         a second barrier -- and leave as 320 L 16-BYTE STORES, lane after lane, a wave writing 1,024 contiguous bytes an instruction.
// Rows beyond the last load and store nothing, and their lanes still reach the barriers.  Plain loads, plain vector stores, no
// atomics, no scratch.
#include <new>

#include "mbx_host.h"
#include "mbx_kernels.h"
#include <mbx_resample.h>   // the public header: include/, first on the include path
#include "mbx_resample_plan.h"

namespace mbx {

static_assert(sizeof(mbx_resample) == 4 + 2 * MBX_RESAMPLE_MAX_TAPS && offsetof(mbx_resample, L) == 0 && offsetof(mbx_resample, K) == 1
                  && offsetof(mbx_resample, zero) == 2 && offsetof(mbx_resample, taps) == 4,
              "the resampler is 388 bytes");
static_assert(sizeof(mbx_resample_record) == 64, "a state record is 32 samples, 16 dwords");
static_assert(MBX_RESAMPLE_MAX_TAPS == kResampleMaxTaps && MBX_RESAMPLE_UNITY_Q14 == kResampleUnity && MBX_RESAMPLE_HISTORY == kResampleHistory,
              "one set of limits, in the public header and in mbx_resample_plan.h");
static_assert(kResampleLanes * kResampleSamples == 160 && kResampleSamples % 2 == 0 && 64 % kResampleLanes == 0 && kResampleBlock % 64 == 0, "the lane map");
static_assert(sizeof(ResampleTaps) == 4 * kResamplePairs + 4, "the filter in the kernel arguments: 388 bytes");

constexpr int kResampleRows = kResampleBlock / kResampleLanes;   // rows of a workgroup: 16
constexpr int kResampleRowPieces = 320 / 16;                     // 16-byte pieces of a row in: 20 (of a row out: 20 L)
constexpr int kResampleRecordPieces = 64 / 16;                   // ... and of a record: 4
static_assert(kResampleWindowWords % 4 == 0 && kResampleRecordWords % 4 == 0, "a window and the row inside it begin on 16 bytes");
static_assert(kResampleRows * kResampleRecordPieces <= 64, "the histories of a workgroup are the work of its first wave");

// two rounded samples as one dword: (acc + 8192) >> 14 each, then the saturating pack
__device__ __forceinline__ uint32_t resample_pack2(int32_t lo, int32_t hi) {
    typedef short resample_i16x2 __attribute__((ext_vector_type(2)));
    const resample_i16x2 y = __builtin_amdgcn_cvt_pk_i16((lo + kResampleRound) >> 14, (hi + kResampleRound) >> 14);
    return __builtin_bit_cast(uint32_t, y);
}

// in: rows = n * T rows of 160, stream-major (16-byte aligned); out: as many rows of 160 L (16-byte aligned, apart from in);
// state: `streams` records of 16 dwords, in place; d_stream: the record of every entry, or nullptr
template <int L>
__global__ void __launch_bounds__(kResampleBlock)
pcm_resample_kernel(ResampleTaps f, uint32_t* state, int streams, const int32_t* __restrict__ d_stream, uint32_t rows, uint32_t T,
                    const int16_t* __restrict__ in, int16_t* __restrict__ out) {
    // the windows of the 16 rows (6 KiB), and behind the sums the 16 wide rows (5,120 L bytes: more, whatever L is)
    static_assert(kResampleRows * kResampleWindowWords * 4 <= kResampleRows * 320 * L, "the wide rows cover the windows");
    __shared__ uint4 lds[kResampleRows * kResampleRowPieces * L];
    uint32_t* const words = reinterpret_cast<uint32_t*>(lds);
    const uint32_t tid = threadIdx.x;
    const uint32_t row0 = blockIdx.x * (uint32_t)kResampleRows;                                       // (below rows: the grid is no larger)
    const uint32_t live = rows - row0 < (uint32_t)kResampleRows ? rows - row0 : (uint32_t)kResampleRows;   // rows of this workgroup
    // ---- in ----
    const uint4* const in4 = reinterpret_cast<const uint4*>(in) + (size_t)row0 * kResampleRowPieces;
    for (uint32_t c = tid; c < live * kResampleRowPieces; c += kResampleBlock) {
        const uint32_t r = c / kResampleRowPieces, piece = c % kResampleRowPieces;
        lds[r * (kResampleWindowWords / 4) + kResampleRecordPieces + piece] = in4[c];
    }
    if (tid < live * kResampleRecordPieces) {
        const uint32_t r = tid / kResampleRecordPieces, piece = tid % kResampleRecordPieces;
        const uint32_t row = row0 + r, entry = row / T, t = row - entry * T;
        uint4 hist = {0u, 0u, 0u, 0u};
        if (t > 0) {   // the tail of the row in front, which is a row of the same entry
            hist = *(in4 + (size_t)r * kResampleRowPieces - kResampleRecordPieces + piece);
        } else {
            const int32_t record = d_stream ? d_stream[entry] : (int32_t)entry;
            if (record >= 0 && record < streams) {   // (an entry outside the state: a zero history, no record touched)
                uint4* const rec = reinterpret_cast<uint4*>(state) + (size_t)record * kResampleRecordPieces + piece;
                hist = *rec;
                // the record behind the call: the last 32 samples of the entry's last row
                const uint4* const last = reinterpret_cast<const uint4*>(in) + ((size_t)entry * T + (T - 1u)) * kResampleRowPieces;
                *rec = last[kResampleRowPieces - kResampleRecordPieces + piece];
            }
        }
        lds[r * (kResampleWindowWords / 4) + piece] = hist;
    }
    __syncthreads();
    // ---- sum ----
    // window dword d holds x_ext[2 d - 32], x_ext[2 d - 31].  For the pair of taps k = 2 kk, D[d] is window dword 5 j + 15 - kk + d:
    // x_ext[10 j - k - 2 + 2 d] and the sample behind it; S[m] is (high of D[m], low of D[m + 1]).
    const int j = (int)(tid % kResampleLanes);
    const uint32_t* const w = words + (tid / kResampleLanes) * kResampleWindowWords;
    const int base = j * (kResampleSamples / 2) + kResampleRecordWords - 1;
    uint32_t D[kResampleSamples / 2 + 1], S[kResampleSamples / 2];
#pragma unroll
    for (int d = 1; d <= kResampleSamples / 2; ++d) {
        D[d] = w[base + d];
    }
#pragma unroll
    for (int m = 1; m < kResampleSamples / 2; ++m) {
        S[m] = __builtin_amdgcn_alignbit(D[m + 1], D[m], 16);
    }
    int32_t acc[kResampleSamples][L];
#pragma unroll
    for (int i = 0; i < kResampleSamples; ++i) {
#pragma unroll
        for (int p = 0; p < L; ++p) {
            acc[i][p] = 0;
        }
    }
    for (int kk = 0; kk < f.half; ++kk) {
        D[0] = w[base - kk];   // (kk <= 15: never below the lane's first dword of the window)
        S[0] = __builtin_amdgcn_alignbit(D[1], D[0], 16);
#pragma unroll
        for (int p = 0; p < L; ++p) {
            const uint32_t h = f.pair[kk * L + p];
#pragma unroll
            for (int i = 0; i < kResampleSamples; i += 2) {
                acc[i][p] = resample_dot2(S[i / 2], h, acc[i][p]);                // an even n: its pair lies across two dwords
                acc[i + 1][p] = resample_dot2(D[i / 2 + 1], h, acc[i + 1][p]);    // an odd n: its pair is a dword of the window
            }
        }
#pragma unroll
        for (int d = kResampleSamples / 2; d >= 1; --d) {
            D[d] = D[d - 1];
        }
#pragma unroll
        for (int m = kResampleSamples / 2 - 1; m >= 1; --m) {
            S[m] = S[m - 1];
        }
    }
    __syncthreads();   // (every window has been read: the wide rows go over them)
    // ---- out ----
    uint32_t* const y = words + (tid / kResampleLanes) * (80 * L) + j * (5 * L);   // the lane's 10 L outputs in its row of 160 L
#pragma unroll
    for (int q = 0; q < 5 * L; ++q) {   // outputs 2 q and 2 q + 1 of the lane: sample (2 q) / L at phase (2 q) % L, and the next
        y[q] = resample_pack2(acc[(2 * q) / L][(2 * q) % L], acc[(2 * q + 1) / L][(2 * q + 1) % L]);
    }
    __syncthreads();
    uint4* const out4 = reinterpret_cast<uint4*>(out) + (size_t)row0 * (kResampleRowPieces * L);
    for (uint32_t c = tid; c < live * (uint32_t)(kResampleRowPieces * L); c += kResampleBlock) {
        out4[c] = lds[c];
    }
}
template __global__ void pcm_resample_kernel<2>(ResampleTaps, uint32_t*, int, const int32_t*, uint32_t, uint32_t, const int16_t*, int16_t*);
template __global__ void pcm_resample_kernel<3>(ResampleTaps, uint32_t*, int, const int32_t*, uint32_t, uint32_t, const int16_t*, int16_t*);
template __global__ void pcm_resample_kernel<4>(ResampleTaps, uint32_t*, int, const int32_t*, uint32_t, uint32_t, const int16_t*, int16_t*);
template __global__ void pcm_resample_kernel<6>(ResampleTaps, uint32_t*, int, const int32_t*, uint32_t, uint32_t, const int16_t*, int16_t*);

}  // namespace mbx

namespace {

using mbx::refuse;

int refuse(const char* who, mbx::ResampleRefusal why) {
    if (why == mbx::kResampleAlign) {
        return mbx::misaligned(who, "mbx_resample.h");
    }
    return refuse(who, mbx::resample_refusal_text(why));
}

mbx::ResampleRefusal filter_refused(const mbx_resample* rs) {
    return mbx::resample_refused(rs != nullptr, rs ? rs->L : 0u, rs ? rs->K : 0u, rs ? (unsigned)(rs->zero[0] | rs->zero[1]) : 0u, rs ? rs->taps : nullptr);
}

// the range of a state call, and the host memory behind it
mbx::ResampleRefusal range_refused(const mbx_resample_state* st, int first, int count, const void* host, bool needs_host) {
    const mbx::ResampleRefusal why = mbx::resample_range_refused(st != nullptr, st ? st->streams : 0, first, count);
    return why == mbx::kResampleOk && needs_host && !host && count > 0 ? mbx::kResampleNoHost : why;
}

}  // namespace

extern "C" {

int mbx_resample_state_create(mbx_resample_state** out, int streams) {
    const char* const who = "mbx_resample_state_create";
    if (!out) {
        return refuse(who, "no place for the handle");
    }
    *out = nullptr;
    if (streams < 0) {
        return refuse(who, mbx::kResampleCounts);
    }
    int dev = -1;
    const int rc = mbx::ready_device(&dev);
    if (rc < 0) {
        return rc;
    }
    mbx_resample_state* st = new (std::nothrow) mbx_resample_state();
    if (!st) {
        return refuse(who, "out of memory");
    }
    st->device = dev;
    st->streams = streams;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&st->d_state), mbx::resample_alloc_bytes(streams));
    if (e == hipSuccess) {
        e = hipMemset(st->d_state, 0, mbx::resample_alloc_bytes(streams));
    }
    if (e == hipSuccess) {   // (the fill is on the null stream, and the launches that read it may be on a non-blocking one)
        e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess) {
        (void)hipFree(st->d_state);
        delete st;
        return mbx::hip_failed("", "mbx_resample_state_create: the records", e);
    }
    *out = st;
    return 0;
}

int mbx_resample_state_destroy(mbx_resample_state* st) {
    if (st) {
        (void)hipFree(st->d_state);
        (void)hipGetLastError();
        delete st;
    }
    return 0;
}

int mbx_resample_state_streams(const mbx_resample_state* st) { return st ? st->streams : MBE_STATUS_INVALID_ARGUMENT; }

int mbx_resample_state_reset(mbx_resample_state* st, int first, int count, void* stream) {
    const mbx::ResampleRefusal why = range_refused(st, first, count, nullptr, false);
    if (why != mbx::kResampleOk) {
        return refuse("mbx_resample_state_reset", why);
    }
    if (count == 0) {
        return 0;
    }
    const hipError_t e = hipMemsetAsync(st->d_state + (size_t)first * mbx::kResampleRecordWords, 0, mbx::resample_state_bytes(count), (hipStream_t)stream);
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_resample_state_reset: hipMemsetAsync", e);
}

int mbx_resample_state_get(const mbx_resample_state* st, int first, int count, mbx_resample_record* host, void* stream) {
    const mbx::ResampleRefusal why = range_refused(st, first, count, host, true);
    if (why != mbx::kResampleOk) {
        return refuse("mbx_resample_state_get", why);
    }
    hipError_t e = hipSuccess;
    if (count > 0) {
        e = hipMemcpyAsync(host, st->d_state + (size_t)first * mbx::kResampleRecordWords, mbx::resample_state_bytes(count), hipMemcpyDeviceToHost,
                           (hipStream_t)stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize((hipStream_t)stream);
    }
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_resample_state_get: copy of the records", e);
}

int mbx_resample_state_set(mbx_resample_state* st, int first, int count, const mbx_resample_record* host, void* stream) {
    const mbx::ResampleRefusal why = range_refused(st, first, count, host, true);
    if (why != mbx::kResampleOk) {
        return refuse("mbx_resample_state_set", why);
    }
    hipError_t e = hipSuccess;
    if (count > 0) {   // (every int16 is a sample: no record is refused)
        e = hipMemcpyAsync(st->d_state + (size_t)first * mbx::kResampleRecordWords, host, mbx::resample_state_bytes(count), hipMemcpyHostToDevice,
                           (hipStream_t)stream);
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize((hipStream_t)stream);
    }
    return e == hipSuccess ? 0 : mbx::hip_failed("", "mbx_resample_state_set: copy of the records", e);
}

int mbx_pcm_resample_host(const mbx_resample* rs, mbx_resample_record* records, int streams, const int32_t* stream_index, int n, int T, const int16_t* in,
                          int16_t* out) {
    const char* const who = "mbx_pcm_resample_host";
    mbx::ResampleRefusal why = filter_refused(rs);
    if (why == mbx::kResampleOk) {
        why = streams < 0 ? mbx::kResampleCounts : (!records && streams > 0) ? mbx::kResampleNoState : mbx::resample_rows_refused(n, T, rs->L, in, out, 0u);
    }
    if (why != mbx::kResampleOk) {
        return refuse(who, why);
    }
    const int L = rs->L;
    const mbx::ResampleTaps f = mbx::resample_pack(rs->taps, L, rs->K);
    int16_t x_ext[mbx::kResampleHistory + 160];
    for (int i = 0; i < n; ++i) {
        const int64_t record = stream_index ? (int64_t)stream_index[i] : (int64_t)i;
        const bool owns = record >= 0 && record < streams;
        for (int k = 0; k < mbx::kResampleHistory; ++k) {   // where the tail of a row lies (an entry outside the state: a zero history)
            x_ext[160 + k] = owns ? records[record].hist[k] : (int16_t)0;
        }
        for (int t = 0; t < T; ++t) {
            const size_t row = (size_t)i * (size_t)T + (size_t)t;
            for (int k = 0; k < mbx::kResampleHistory; ++k) {   // the tail of the window of the row in front is the history of this one
                x_ext[k] = x_ext[160 + k];
            }
            for (int k = 0; k < 160; ++k) {
                x_ext[mbx::kResampleHistory + k] = in[row * 160u + k];
            }
            for (int m = 0; m < 160; ++m) {
                for (int p = 0; p < L; ++p) {
                    out[(row * 160u + (size_t)m) * (size_t)L + (size_t)p] = mbx::resample_sample(f, L, p, x_ext + mbx::kResampleHistory + m);   // THE definition
                }
            }
        }
        if (owns && T > 0) {
            for (int k = 0; k < mbx::kResampleHistory; ++k) {
                records[record].hist[k] = x_ext[160 + k];
            }
        }
    }
    return 0;
}

int mbx_pcm_resample(const mbx_resample* rs, mbx_resample_state* state, const int32_t* d_stream, int n, int T, const int16_t* d_in, int16_t* d_out,
                     void* stream) {
    const char* const who = "mbx_pcm_resample";
    const mbx::ResampleRefusal why = mbx::resample_launch_refused(rs != nullptr, rs ? rs->L : 0u, rs ? rs->K : 0u, rs ? (unsigned)(rs->zero[0] | rs->zero[1]) : 0u,
                                                                  rs ? rs->taps : nullptr, state != nullptr, n, T, d_in, d_out);
    if (why != mbx::kResampleOk) {
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
    const uint32_t rows = (uint32_t)((size_t)n * (size_t)T);
    const dim3 grid(mbx::resample_grid(rows)), block(mbx::kResampleBlock);
    const mbx::ResampleTaps f = mbx::resample_pack(rs->taps, rs->L, rs->K);
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, f, state->d_state, state->streams, d_stream, rows, (uint32_t)T, d_in, d_out);
    };
    switch (rs->L) {
    case 2: launch(mbx::pcm_resample_kernel<2>); break;
    case 3: launch(mbx::pcm_resample_kernel<3>); break;
    case 4: launch(mbx::pcm_resample_kernel<4>); break;
    default: launch(mbx::pcm_resample_kernel<6>); break;   // (resample_L_ok: nothing else is left)
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : mbx::hip_failed("", "pcm_resample_kernel", e);
}

}  // extern "C"
